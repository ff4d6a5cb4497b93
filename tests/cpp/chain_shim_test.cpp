// The chained guide pass of the C++ shim (include/pt_renderer.hpp renderGuidesChain / readGuideChain) against the C ABI: compiles, links with libptmi.so and,
// with a GPU, renders the planes of a mirror quad that shows a diffuse quad behind the camera, on both structures, checks the middle pixel and a corner,
// and prints checksums of the planes and the link plane; tests/test_chain_shim.py runs the same round through the Python route and compares.  Without a
// GPU setup() must fail loudly (no fallback).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "stage/shim_common.h"

static pt_GltfShadeMaterial material(float r, float g, float b, float metallic, float roughness)
{
  pt_GltfShadeMaterial m{};
  m.pbrBaseColorFactor[0] = r; m.pbrBaseColorFactor[1] = g; m.pbrBaseColorFactor[2] = b; m.pbrBaseColorFactor[3] = 1.f;
  m.pbrBaseColorTexture = m.pbrMetallicRoughnessTexture = m.emissiveTexture = m.normalTexture = m.transmissionTexture = m.clearcoatTexture = m.clearcoatRoughnessTexture = m.thicknessTexture = -1;
  m.pbrMetallicFactor = metallic; m.pbrRoughnessFactor = roughness; m.ior = 1.5f; m.doubleSided = 0; m.attenuationDistance = 3.4e38f;
  m.attenuationColor[0] = m.attenuationColor[1] = m.attenuationColor[2] = 1.f;
  for(int i = 0; i < 4; ++i) m.uvTransform[i * 5] = 1.f;
  return m;
}

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
  pt_VertexAttributes v[8];
  pt_pack_vertices(4, pos, nrm, tan, uv, col, v);
  pt_pack_vertices(4, pos, nrm, tan, uv, col, v + 4);
  uint32_t    idx[12] = {0, 1, 2, 0, 2, 3, 0, 1, 2, 0, 2, 3};
  pt_PrimMesh pm[2]   = {{0, 4, 0, 6, 0}, {4, 4, 6, 6, 1}};
  // node 0: the mirror, the quad as it is (z = 0, facing +z).  node 1: the diffuse quad, four times the size, turned about y to face -z, at z = 5
  pt_Node nd[2]{};
  for(int i = 0; i < 4; ++i) nd[0].worldMatrix[i * 5] = 1.f;
  nd[0].primMesh = 0;
  nd[1].worldMatrix[0] = -4.f; nd[1].worldMatrix[5] = 4.f; nd[1].worldMatrix[10] = -4.f; nd[1].worldMatrix[15] = 1.f; nd[1].worldMatrix[14] = 5.f;
  nd[1].primMesh = 1;
  pt_GltfShadeMaterial m[2] = {material(0.9f, 0.8f, 0.7f, 1.f, 0.f), material(0.2f, 0.4f, 0.6f, 0.f, 1.f)};
  pt_SceneDesc         sd{v, 8, idx, 12, pm, 2, nd, 2, m, 2, nullptr, 0, nullptr, 0};
  const int            W = 24, H = 16;
  const size_t         n = size_t(W) * H;
  r.create({uint32_t(W), uint32_t(H)}, &sd);
  if(!r.ok())
  {
    std::printf("ERROR create: %s\n", r.lastError().c_str());
    return 4;
  }
  const pt_GuideChain chain{4u, 0.05f, 0.9f, 0.9f, 0u};
  std::vector<uint32_t> links(n);
  if(r.renderGuidesChain(chain) || r.status() != PT_ERR_STATE)  // before a camera exists
    return 5;
  const float    eye[3] = {0, 0, 3}, center[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  pt_SceneCamera cam{};
  if(pt_camera_lookat(eye, center, up, 60.f, float(W) / float(H), &cam) != PT_OK)
    return 6;
  r.setCamera(cam);
  if(r.readGuideChain(links.data()) || r.status() != PT_ERR_STATE)  // no chained pass yet
    return 7;
  pt_GuideChain bad = chain;
  bad.maxLinks      = PT_GUIDE_CHAIN_MAX_LINKS + 1;
  if(r.renderGuidesChain(bad) || r.status() != PT_ERR_INVALID)
    return 8;
  unsigned long long sums[2][4];
  for(int mode : {PT_ACCEL_FLAT, PT_ACCEL_TWO_LEVEL})
  {
    r.setAccelMode(mode);
    std::vector<float> a(n * 4, -1.f), nr(n * 4, -1.f), d(n * 4, -1.f);
    if(!r.renderGuidesChain(chain, PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH, 50.f) || !r.readDenoiseGuides(a.data(), nr.data(), d.data()) || !r.readGuideChain(links.data()))
    {
      std::printf("ERROR renderGuidesChain / readGuideChain mode %d: %s\n", mode, r.lastError().c_str());
      return 9;
    }
    const size_t mid = size_t(H / 2) * W + W / 2, corner = 0;  // the mirror covers the middle of the image; the corners see past it
    const bool   hitOk = links[mid] == 1u && std::fabs(a[4 * mid] - 0.9f * 0.2f) < 1e-6f && std::fabs(a[4 * mid + 1] - 0.8f * 0.4f) < 1e-6f && std::fabs(a[4 * mid + 2] - 0.7f * 0.6f) < 1e-6f &&
                       std::fabs(nr[4 * mid] - 0.5f) < 1e-6f && std::fabs(nr[4 * mid + 1] - 0.5f) < 1e-6f && std::fabs(nr[4 * mid + 2]) < 1e-6f && std::fabs(d[4 * mid] - 8.f) < 5e-2f;
    const bool   missOk = links[corner] == (1u << 8) && a[4 * corner] == 0.f && a[4 * corner + 3] == 1.f && nr[4 * corner + 3] == 1.f && d[4 * corner] == 50.f;
    if(!hitOk || !missOk)
    {
      std::printf("ERROR mode %d: middle word %u albedo %.3f %.3f %.3f normal %.3f %.3f %.3f depth %.3f; corner word %u depth %.3f\n", mode, links[mid], a[4 * mid], a[4 * mid + 1],
                  a[4 * mid + 2], nr[4 * mid], nr[4 * mid + 1], nr[4 * mid + 2], d[4 * mid], links[corner], d[4 * corner]);
      return 10;
    }
    const int k = mode == PT_ACCEL_FLAT ? 0 : 1;
    sums[k][0] = fnv(a.data(), n * 16); sums[k][1] = fnv(nr.data(), n * 16); sums[k][2] = fnv(d.data(), n * 16); sums[k][3] = fnv(links.data(), n * 4);
  }
  std::printf("OK albedo=%016llx normal=%016llx depth=%016llx links=%016llx albedo2=%016llx normal2=%016llx depth2=%016llx links2=%016llx\n", sums[0][0], sums[0][1], sums[0][2],
              sums[0][3], sums[1][0], sums[1][1], sums[1][2], sums[1][3]);
  return 0;
}
