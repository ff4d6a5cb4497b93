// Motion of moving instances through the C++ shim (include/pt_renderer.hpp renderInstancePlane / setInstancePlane / readInstancePlane /
// temporalAccumulateMoving) against the C ABI: compiles, links with libptmi.so and, with a GPU, renders the instance plane of a quad, slides the quad
// within its own plane with updateInstances and accumulates twice -- the moving form keeps the quad's history, the static form fed the same calls keeps
// only part of it, and with a plane that names no node the moving form is the static one.  Without a GPU setup() must fail loudly (no fallback).
#include <cstdio>
#include <cstring>
#include <vector>
#include "stage/shim_common.h"

int main()
{
  ptmi::HipPathTracer r;
  r.setup(0);
  if(!r.ok())
    return shim_no_device(r);
  const float pos[12] = {-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0}, nrm[12] = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
  const float tan[16] = {1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1}, uv[8] = {0, 0, 1, 0, 1, 1, 0, 1};
  float       col[16];
  for(float& c : col) c = 1.f;
  pt_VertexAttributes v[4];
  pt_pack_vertices(4, pos, nrm, tan, uv, col, v);
  uint32_t             idx[6] = {0, 1, 2, 0, 2, 3};
  pt_PrimMesh          pm{0, 4, 0, 6, 0};
  pt_Node              nd{};
  for(int i = 0; i < 4; ++i) nd.worldMatrix[i * 5] = 1.f;
  pt_GltfShadeMaterial m{};
  m.pbrBaseColorFactor[0] = m.pbrBaseColorFactor[1] = m.pbrBaseColorFactor[2] = 0.5f;
  m.pbrBaseColorFactor[3] = 1.f;
  m.pbrBaseColorTexture = m.pbrMetallicRoughnessTexture = m.emissiveTexture = m.normalTexture = m.transmissionTexture = m.clearcoatTexture = m.clearcoatRoughnessTexture = m.thicknessTexture = -1;
  m.pbrRoughnessFactor = 1.f; m.ior = 1.5f; m.doubleSided = 0; m.attenuationDistance = 3.4e38f;
  m.attenuationColor[0] = m.attenuationColor[1] = m.attenuationColor[2] = 1.f;
  for(int i = 0; i < 4; ++i) m.uvTransform[i * 5] = 1.f;
  pt_SceneDesc sd{v, 4, idx, 6, &pm, 1, &nd, 1, &m, 1, nullptr, 0, nullptr, 0};
  const int    W = 40, H = 24;
  const size_t n = size_t(W) * H;
  r.create({uint32_t(W), uint32_t(H)}, &sd);
  if(!r.ok())
  {
    std::printf("ERROR create: %s\n", r.lastError().c_str());
    return 4;
  }
  pt_TemporalParams p{};
  p.depthTol = 0.05f, p.normalDist2 = 0.05f, p.maxHistory = 8.f;
  const float    eye[3] = {0, 0, 3}, center[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  pt_SceneCamera cam{};
  if(pt_camera_lookat(eye, center, up, 60.f, float(W) / float(H), &cam) != PT_OK || pt_camera_world_to_clip(eye, center, up, 60.f, float(W) / float(H), p.worldToClip) != PT_OK)
    return 5;
  r.setCamera(cam);
  std::vector<uint32_t> ids(n, 7u), back(n);
  if(r.readInstancePlane(ids.data()) || r.status() != PT_ERR_STATE)  // no plane yet
    return 6;
  std::vector<float> img(n * 4), hn[2] = {std::vector<float>(n), std::vector<float>(n)}, hc(n * 4), none(n * 4), stat(n * 4);
  const size_t       mid = size_t(H / 2) * W + W / 2;
  // form 0: the moving form; form 1: pt_temporal_accumulate fed the same calls
  for(int form = 0; form < 2; ++form)
  {
    r.temporalReset();
    for(int k = 0; k < 2; ++k)
    {
      nd.worldMatrix[12] = 0.35f * float(k);  // the quad slides along x, within its own plane
      r.updateInstances(&nd, 1);
      if(!r.ok() || !r.renderInstancePlane(PT_GUIDES_NORMAL | PT_GUIDES_DEPTH, 50.f) || !r.readInstancePlane(ids.data()))
      {
        std::printf("ERROR renderInstancePlane %d: %s\n", k, r.lastError().c_str());
        return 7;
      }
      if(ids[mid] != 0u || ids[0] != PT_INSTANCE_NONE)
      {
        std::printf("ERROR instance plane: middle %u, corner %u\n", ids[mid], ids[0]);
        return 8;
      }
      shim_image(img, k);
      r.writeAccum(img.data());
      if(!(form == 0 ? r.temporalAccumulateMoving(p) : r.temporalAccumulate(p)) || !r.readTemporalHistory(hc.data(), hn[form].data()))
      {
        std::printf("ERROR accumulate form %d round %d: %s\n", form, k, r.lastError().c_str());
        return 9;
      }
    }
  }
  // every pixel of the moved quad whose point was on screen before kept its history in the moving form; the static form lost the strip the quad newly covers
  size_t quad = 0, keptMoving = 0, keptStatic = 0;
  for(size_t i = 0; i < n; ++i)
    if(ids[i] == 0u)
      quad++, keptMoving += hn[0][i] == 2.f, keptStatic += hn[1][i] == 2.f;
  if(quad < 50 || keptMoving != quad || keptStatic >= keptMoving || hn[0][mid] != 2.f)
  {
    std::printf("ERROR lengths: %zu pixels of the quad, %zu kept moving, %zu kept static\n", quad, keptMoving, keptStatic);
    return 10;
  }
  // a plane that names no node: the moving form is the static one -- the same two calls, then a third in either form
  std::fill(back.begin(), back.end(), 0x7fffffffu);
  if(!r.setInstancePlane(back.data()) || !r.readInstancePlane(ids.data()) || ids[mid] != 0x7fffffffu)
  {
    std::printf("ERROR setInstancePlane: %s\n", r.lastError().c_str());
    return 11;
  }
  for(int form = 0; form < 2; ++form)
  {
    r.temporalReset();
    for(int k = 0; k < 3; ++k)
    {
      shim_image(img, k);
      r.writeAccum(img.data());
      if(!(k == 2 && form == 0 ? r.temporalAccumulateMoving(p, none.data()) : r.temporalAccumulate(p, stat.data())))
        return 12;
    }
  }
  if(std::memcmp(none.data(), stat.data(), n * 16) != 0)
    return 13;
  if(!r.setInstancePlane(nullptr) || r.temporalAccumulateMoving(p) || r.status() != PT_ERR_STATE)
    return 14;
  std::printf("OK\n");
  return 0;
}
