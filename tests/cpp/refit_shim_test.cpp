// The deforming meshes of the C++ shim (include/pt_renderer.hpp updateVertices / refitAccel) against the C ABI: compiles, links with libptmi.so and, with a
// GPU, renders two frames of a quad under a small environment after its four vertices moved and the structure was refitted, in both modes, and prints the
// checksums of the images (tests/test_refit_shim.py compares them with the Python route's on the same scene).  In between it checks the stale state: a
// frame is refused until the refit.  Without a GPU setup() must fail loudly (no fallback).
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
  const float nrm[12] = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
  const float tan[16] = {1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1}, uv[8] = {0, 0, 1, 0, 1, 1, 0, 1};
  float       pos[12] = {-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0};
  float       col[16];
  for(float& c : col) c = 1.f;
  pt_VertexAttributes v[4];
  pt_pack_vertices(4, pos, nrm, tan, uv, col, v);
  uint32_t             idx[6] = {0, 1, 2, 0, 2, 3};
  pt_PrimMesh          pm{0, 4, 0, 6, 0};
  pt_Node              nd{};
  for(int i = 0; i < 4; ++i) nd.worldMatrix[i * 5] = 1.f;
  pt_GltfShadeMaterial m{};
  m.pbrBaseColorFactor[0] = 0.75f; m.pbrBaseColorFactor[1] = 0.5f; m.pbrBaseColorFactor[2] = 0.25f;
  m.pbrBaseColorFactor[3] = 1.f;
  m.pbrBaseColorTexture = m.pbrMetallicRoughnessTexture = m.emissiveTexture = m.normalTexture = m.transmissionTexture = m.clearcoatTexture = m.clearcoatRoughnessTexture = m.thicknessTexture = -1;
  m.pbrRoughnessFactor = 1.f; m.ior = 1.5f; m.doubleSided = 0; m.attenuationDistance = 3.4e38f;
  m.attenuationColor[0] = m.attenuationColor[1] = m.attenuationColor[2] = 1.f;
  for(int i = 0; i < 4; ++i) m.uvTransform[i * 5] = 1.f;
  pt_SceneDesc sd{v, 4, idx, 6, &pm, 1, &nd, 1, &m, 1, nullptr, 0, nullptr, 0};
  r.refitAccel();
  if(r.status() != PT_ERR_STATE)  // nothing to refit yet
  {
    std::printf("ERROR refitAccel before create: status %d\n", r.status());
    return 4;
  }
  const ptmi::Extent2D size{32, 32};
  r.create(size, &sd);
  std::vector<float> env(8 * 4 * 4);
  for(int i = 0; i < 32; ++i)
  {
    env[4 * i] = float(i % 5 + 1) * 0.25f; env[4 * i + 1] = float(i % 3 + 1) * 0.25f; env[4 * i + 2] = float(i % 7 + 1) * 0.125f; env[4 * i + 3] = 1.f;
  }
  float integral = 0.f, average = 0.f;
  r.setEnvironment(env.data(), 8, 4, &integral, &average);
  const float    eye[3] = {0, 0, 3}, center[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  pt_SceneCamera cam{};
  if(pt_camera_lookat(eye, center, up, 60.f, 1.f, &cam) != PT_OK)
    return 6;
  r.setCamera(cam);
  pt_RtxState st{};
  st.maxDepth = 3; st.maxSamples = 1; st.fireflyClampThreshold = 100.f; st.hdrMultiplier = 1.f; st.maxHeatmap = 65000;
  // the deformed quad: smaller, tilted, one corner pulled towards the camera
  const float moved[12] = {-0.75f, -0.5f, 0.25f, 0.5f, -0.75f, -0.125f, 0.75f, 0.5f, 0.5f, -0.5f, 0.75f, 0.f};
  pt_VertexAttributes v2[4];
  pt_pack_vertices(4, moved, nrm, tan, uv, col, v2);
  unsigned long long sums[2] = {0, 0};
  for(int mode : {PT_ACCEL_FLAT, PT_ACCEL_TWO_LEVEL})
  {
    r.setAccelMode(mode);
    r.create(size, &sd);  // the undeformed quad again, and its structure built in this mode
    r.updateVertices(0, 4, v2);
    st.frame = 0;
    r.setPushContants(st);
    r.run(size);
    if(r.status() != PT_ERR_STATE || r.lastError().find("refit") == std::string::npos)
    {
      std::printf("ERROR mode %d: a frame on a stale structure: status %d (%s)\n", mode, r.status(), r.lastError().c_str());
      return 7;
    }
    const pt_RefitInfo info = r.refitAccel();
    if(r.status() != PT_OK || info.slotsWritten != 2 || info.nodesWritten != 1 || !(info.costBefore > 0.0) || !(info.costAfter > 0.0) || info.costAfter >= info.costBefore)
    {
      std::printf("ERROR mode %d: refitAccel status %d slots %u nodes %u cost %g -> %g (%s)\n", mode, r.status(), info.slotsWritten, info.nodesWritten, info.costBefore, info.costAfter,
                  r.lastError().c_str());
      return 8;
    }
    std::vector<float> img(32 * 32 * 4);
    for(int f = 0; f < 2; ++f)
    {
      st.frame = f;
      r.setPushContants(st);
      r.run(size);
    }
    r.readAccum(img.data());
    if(r.status() != PT_OK)
    {
      std::printf("ERROR mode %d: frames after the refit: %s\n", mode, r.lastError().c_str());
      return 9;
    }
    sums[mode == PT_ACCEL_TWO_LEVEL] = fnv(img.data(), img.size() * 4);
  }
  std::printf("OK flat=%016llx two=%016llx\n", sums[0], sums[1]);
  return 0;
}
