// The path queries of the C++ shim (include/pt_renderer.hpp tracePaths / tracePathsDevice) against the C ABI: compiles, links with libptmi.so and, with
// a GPU, asks for the radiance along a few rays at a quad under a small environment -- through host arrays and through device memory of the caller's
// own (hipMalloc) -- with the same records, whose checksum it prints (tests/test_paths_shim.py compares it with the Python route's on the same scene).
// Without a GPU setup() must fail loudly (no fallback).
#include <hip/hip_runtime_api.h>
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
  m.pbrBaseColorFactor[0] = 0.75f; m.pbrBaseColorFactor[1] = 0.5f; m.pbrBaseColorFactor[2] = 0.25f;
  m.pbrBaseColorFactor[3] = 1.f;
  m.pbrBaseColorTexture = m.pbrMetallicRoughnessTexture = m.emissiveTexture = m.normalTexture = m.transmissionTexture = m.clearcoatTexture = m.clearcoatRoughnessTexture = m.thicknessTexture = -1;
  m.pbrRoughnessFactor = 1.f; m.ior = 1.5f; m.doubleSided = 0; m.attenuationDistance = 3.4e38f;
  m.attenuationColor[0] = m.attenuationColor[1] = m.attenuationColor[2] = 1.f;
  for(int i = 0; i < 4; ++i) m.uvTransform[i * 5] = 1.f;
  pt_SceneDesc sd{v, 4, idx, 6, &pm, 1, &nd, 1, &m, 1, nullptr, 0, nullptr, 0};
  // towards the quad's front, its other triangle, past it (a miss: the environment), at its back (culled: a miss), and an invalid ray
  const pt_Ray rays[5] = {{{0.5f, -0.5f, 3}, 10.f, {0, 0, -1}, 1u}, {{-0.5f, 0.5f, 3}, 10.f, {0, 0, -1}, 2u}, {{3, 3, 3}, 10.f, {0, 0, -1}, 3u},
                          {{0.5f, -0.5f, -3}, 10.f, {0, 0, 1}, 4u}, {{0, 0, 3}, 10.f, {0, 0, 0}, 5u}};
  pt_RtxState  st{};
  st.maxDepth = 4; st.maxSamples = 3; st.fireflyClampThreshold = 100.f; st.hdrMultiplier = 1.f; st.maxHeatmap = 65000;
  pt_PathResult none{};
  if(r.tracePaths(st, 1, rays, &none) || r.status() != PT_ERR_STATE)  // before a scene exists
  {
    std::printf("ERROR tracePaths before create: status %d\n", r.status());
    return 4;
  }
  r.create({64, 64}, &sd);
  // an 8 x 4 environment: texel i is ((i % 5 + 1) / 4, (i % 3 + 1) / 4, (i % 7 + 1) / 8, 1)
  std::vector<float> env(8 * 4 * 4);
  for(int i = 0; i < 32; ++i)
  {
    env[4 * i] = float(i % 5 + 1) * 0.25f; env[4 * i + 1] = float(i % 3 + 1) * 0.25f; env[4 * i + 2] = float(i % 7 + 1) * 0.125f; env[4 * i + 3] = 1.f;
  }
  float integral = 0.f, average = 0.f;
  r.setEnvironment(env.data(), 8, 4, &integral, &average);
  if(r.tracePaths(st, 1, rays, &none) || r.status() != PT_ERR_STATE)  // before a camera exists
  {
    std::printf("ERROR tracePaths before setCamera: status %d\n", r.status());
    return 5;
  }
  const float    eye[3] = {0, 0, 3}, center[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  pt_SceneCamera cam{};
  if(pt_camera_lookat(eye, center, up, 60.f, 1.f, &cam) != PT_OK)
    return 6;
  r.setCamera(cam);
  unsigned long long sums[2] = {0, 0};
  for(int mode : {PT_ACCEL_FLAT, PT_ACCEL_TWO_LEVEL})
  {
    r.setAccelMode(mode);
    pt_PathResult host[5], dev[5];
    std::memset(host, 0xAB, sizeof(host));
    if(!r.tracePaths(st, 5, rays, host))
    {
      std::printf("ERROR tracePaths mode %d: %s\n", mode, r.lastError().c_str());
      return 7;
    }
    pt_Ray*        dRays    = nullptr;
    pt_PathResult* dResults = nullptr;
    if(hipMalloc((void**)&dRays, sizeof(rays)) != hipSuccess || hipMalloc((void**)&dResults, sizeof(dev)) != hipSuccess || hipMemcpy(dRays, rays, sizeof(rays), hipMemcpyHostToDevice) != hipSuccess)
      return 8;
    const bool ok = r.tracePathsDevice(st, 5, dRays, dResults) && hipMemcpy(dev, dResults, sizeof(dev), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(dRays);
    (void)hipFree(dResults);
    if(!ok || std::memcmp(host, dev, sizeof(host)) != 0)
    {
      std::printf("ERROR tracePathsDevice mode %d differs (%s)\n", mode, r.lastError().c_str());
      return 9;
    }
    const bool good = host[0].status == PT_RAY_HIT && host[1].status == PT_RAY_HIT && host[2].status == 0 && host[3].status == 0 && host[4].status == PT_RAY_INVALID && host[4].seed == 5u &&
                      host[4].closestRays == 0 && host[4].radiance[0] == 0.f && host[0].firstT > 2.99f && host[0].firstT < 3.01f && host[2].firstT == 0.f && host[2].closestRays == 3 &&
                      host[2].seed == 3u && host[2].radiance[0] > 0.f && host[0].closestRays >= 3 && host[0].closestRays <= 6 && host[0].radiance[0] >= 0.f && host[0].seed != 1u;
    if(!good)
    {
      std::printf("ERROR mode %d: status %u %u %u %u %u firstT %.3f rays %u %u radiance %.3f %.3f\n", mode, host[0].status, host[1].status, host[2].status, host[3].status, host[4].status,
                  host[0].firstT, host[0].closestRays, host[2].closestRays, host[0].radiance[0], host[2].radiance[0]);
      return 10;
    }
    sums[mode == PT_ACCEL_TWO_LEVEL] = fnv(host, sizeof(host));
  }
  st.maxSamples = 0;
  if(r.tracePaths(st, 5, rays, &none) || r.status() != PT_ERR_INVALID)
    return 11;
  std::printf("OK flat=%016llx two=%016llx\n", sums[0], sums[1]);
  return 0;
}
