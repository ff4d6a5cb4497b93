// Puts a refitted structure (tests/cpp/refit_host.cpp rfh_refit on a harness dump) into a scene of the host harness, so that the harness's own walks
// (th_candidates of tests/cpp/trace_host.cpp) run on it (tests/test_refit_host.py).
//   rfh_scene_set_flat  into the scene the dump was taken from, with the deformed vertices; the brute-force list is made again from them by the harness's
//                       own world_record.  Array sizes must be the scene's: nothing is resized, the pointers the walks hold stay valid.
//   rfh_scene_set_two   the refitted bottom-level arrays (merged structure and BLASes) into the harness scene of the DEFORMED scene, whose instance
//                       hierarchy, padding constants, vertices and brute-force list are already those of the deformed vertices -- what pt_refit_accel
//                       leaves: kept bottom-level topology under an instance hierarchy built again.  The leaves name their BLAS by the node bases of
//                       the structure that was refitted.
#include "th_scene.h"

extern "C" int rfh_scene_set_flat(void* p, uint32_t numVertices, const float* vertexWords, uint32_t numNodes, const uint32_t* wideWords, uint32_t numSlots, const uint32_t* triWords,
                                  const uint32_t* alphaWords, const uint32_t* cnodeWords)
{
  Scene* s = static_cast<Scene*>(p);
  if(!s || size_t(numVertices) * 2 != s->vertices.size() || numNodes != s->flat.wide.size() || numSlots != s->flat.tris.size() || s->flatAlpha.size() < numSlots ||
     (cnodeWords && s->flatCNodes.size() != numNodes))
    return -1;
  std::memcpy(s->vertices.data(), vertexWords, sizeof(float4) * s->vertices.size());
  std::memcpy(s->flat.wide.data(), wideWords, sizeof(WideNode) * numNodes);
  std::memcpy(s->flat.tris.data(), triWords, sizeof(TriRec) * numSlots);
  std::memcpy(s->flatAlpha.data(), alphaWords, sizeof(AlphaRec) * numSlots);
  if(cnodeWords)
    std::memcpy(s->flatCNodes.data(), cnodeWords, sizeof(CompactNode) * numNodes);
  size_t w = 0;
  for(uint32_t i = 0; i < s->inst.size(); ++i)
    for(uint32_t k = 0; k < s->inst[i].triCount; ++k)
      s->world[w++] = world_record(*s, s->inst[i], i, k, s->inst[i].triBase + k);
  return 0;
}

extern "C" int rfh_scene_set_two(void* p, uint32_t numNodes, const uint32_t* wideWords, uint32_t numSlots, const uint32_t* triWords, const uint32_t* alphaWords, const uint32_t* cnodeWords,
                                 uint32_t numInst, const uint32_t* instNodeBase)
{
  Scene* s = static_cast<Scene*>(p);
  if(!s || numInst != s->inst.size() || numSlots != s->blasTris.size() || (cnodeWords == nullptr) != (s->dsTwo.cnodes == nullptr))
    return -1;
  for(const TlasLeaf& l : s->tlasLeaves)  // every BLAS a leaf will name lies inside the refitted node array
    if(l.inst != PT_INST_MERGED && l.inst < numInst && instNodeBase[l.inst] >= numNodes)
      return -2;
  const WideNode* w = reinterpret_cast<const WideNode*>(wideWords);
  const TriRec*   t = reinterpret_cast<const TriRec*>(triWords);
  const AlphaRec* a = reinterpret_cast<const AlphaRec*>(alphaWords);
  s->blasWide.assign(w, w + numNodes);
  s->blasTris.assign(t, t + numSlots);
  s->blasAlpha.assign(a, a + numSlots);
  if(s->blasAlpha.empty())
    s->blasAlpha.emplace_back();
  s->dsTwo.wide = s->blasWide.data(); s->dsTwo.tris = s->blasTris.data(); s->dsTwo.alphaRecs = s->blasAlpha.data();
  if(cnodeWords)
  {
    const CompactNode* c = reinterpret_cast<const CompactNode*>(cnodeWords);
    s->blasCNodes.assign(c, c + numNodes);
    s->dsTwo.cnodes = s->blasCNodes.data();
  }
  for(TlasLeaf& l : s->tlasLeaves)
    if(l.inst != PT_INST_MERGED && l.inst < numInst)
      l.nodeBase = instNodeBase[l.inst];
  s->instNodeBase.assign(instNodeBase, instNodeBase + numInst);
  return 0;
}
