// What the library derives from a scene description on the HOST, before anything is uploaded (pt_scene_records.cpp: no HIP call in it).
// Internal: not installed.
#pragma once
#include <string>
#include <vector>
#include "../../include/pt_api.h"
#include "pt_device.h"

// Everything pt_set_scene derives from a pt_SceneDesc: validation, the per-instance records (transforms, inverse, TLAS flags of
// src/accelstruct.cpp:144-149), the texture records and the compact alpha view of the materials with their opacity maps.  Shared with the test
// hook pt_debug_scene_records (CPU tests run the product's traversal on exactly these records).
struct SceneRecords {
  std::vector<InstanceRec> inst;
  uint64_t                 triTotal = 0;
  std::vector<float>       primBound;  // per prim-mesh: max |coordinate| of its vertices
  std::vector<TexRec>      texRecs;    // >= 1 (a 1x1 white default when the scene has no texture, src/scene.cpp:513-519)
  size_t                   texels = 0; // texels of the RGBA8 pool
  std::vector<AlphaMat>    alphaMats;
  std::vector<uint32_t>    alphaMaps;
  // interleaved texture groups (pt_device.h TexRec::tiled): the pool holds every texture in its plain form first, then the groups
  struct TexGroup {
    int      tex[4];  // texture ids in layer order (-1: unused layer)
    int      layers;
    uint32_t offset;  // first texel word of the group in the pool
  };
  std::vector<TexGroup> groups;
  std::vector<uint4>    matLines;  // PT_MAT_LINE_QUADS per material (pt_device.h mat_line_pack)
};
int build_scene_records(const pt_SceneDesc* d, SceneRecords& R, std::string& err, int texTile, int texGroups);
// the texels of an image in the storage order its record says (row-major source -> row-major or block-linear, pt_device.h tex_index)
void store_texture(uint32_t* dst, const TexRec& tr, const void* rgba8RowMajor);
// the texels of a group: texel (x, y) of layer l at tex_index(...) x layers + l
void store_group(uint32_t* dst, const SceneRecords::TexGroup& g, const std::vector<TexRec>& texRecs, const pt_SceneDesc* d);

// fills the per-instance part of an InstanceRec that depends on the node's world matrix (pt_set_scene, pt_update_instances); false: singular
bool set_instance_transform(InstanceRec& I, const float* m, uint32_t materialFlags);
// object-space padding of the two-level walk (TlasLeaf::padC0 / padC1) for an instance of a mesh whose |coordinates| are <= Bo
void two_level_pad(const InstanceRec& I, float Bo, float& c0, float& c1);
// first bounce handed to k_tail (flush_pending's launch-policy decision on plain numbers; maxDepth: never)
int tail_from_depth(double paths, int maxDepth, int tailBelow, const double* ratio, int numObserved);
