// The gather queries of the C++ shim (include/pt_renderer.hpp gatherIrradiance / gatherProbes / gatherDevice) against the C ABI: compiles, links with
// libptmi.so and, with a GPU, gathers at a few points above, beside and behind a quad under a small environment -- through host arrays and through
// device memory of the caller's own (hipMalloc) -- with the same records, whose checksums it prints (tests/test_gather_shim.py compares them with the
// Python route's on the same scene).  Without a GPU setup() must fail loudly (no fallback).
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
  // above the quad looking down at it (every sample hits), on the quad looking up (none does), beside it, behind it (culled), and an invalid point
  const pt_GatherPoint pts[5] = {{{0, 0, 0.01f}, 1u, {0, 0, -2}, 0u}, {{0.5f, 0.5f, 0}, 2u, {0, 0, 1}, 0u}, {{3, 3, 1}, 3u, {-1, -1, -0.5f}, 0u},
                                 {{0, 0, -1}, 4u, {0, 0, 1}, 0u}, {{0, 0, 1}, 5u, {0, 0, 0}, 0u}};
  pt_RtxState st{};
  st.maxDepth = 4; st.maxSamples = 8; st.fireflyClampThreshold = 100.f; st.hdrMultiplier = 1.f; st.maxHeatmap = 65000;
  pt_GatherResult none{};
  if(r.gatherIrradiance(st, 1, pts, &none) || r.status() != PT_ERR_STATE)  // before a scene exists
  {
    std::printf("ERROR gatherIrradiance before create: status %d\n", r.status());
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
  const float    eye[3] = {0, 0, 3}, center[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  pt_SceneCamera cam{};
  if(pt_camera_lookat(eye, center, up, 60.f, 1.f, &cam) != PT_OK)
    return 6;
  r.setCamera(cam);
  unsigned long long sums[2][2] = {{0, 0}, {0, 0}};
  for(int mode : {PT_ACCEL_FLAT, PT_ACCEL_TWO_LEVEL})
  {
    r.setAccelMode(mode);
    pt_GatherResult host[5], dev[5];
    pt_ProbeResult  probes[5], dprobes[5];
    std::memset(host, 0xAB, sizeof(host));
    std::memset(probes, 0xAB, sizeof(probes));
    if(!r.gatherIrradiance(st, 5, pts, host) || !r.gatherProbes(st, 5, pts, probes))
    {
      std::printf("ERROR gather mode %d: %s\n", mode, r.lastError().c_str());
      return 7;
    }
    pt_GatherPoint* dPts = nullptr;
    void *          dA = nullptr, *dB = nullptr;
    if(hipMalloc((void**)&dPts, sizeof(pts)) != hipSuccess || hipMalloc(&dA, sizeof(dev)) != hipSuccess || hipMalloc(&dB, sizeof(dprobes)) != hipSuccess ||
       hipMemcpy(dPts, pts, sizeof(pts), hipMemcpyHostToDevice) != hipSuccess)
      return 8;
    const bool ok = r.gatherDevice(st, PT_GATHER_HEMISPHERE, 5, dPts, dA) && r.gatherDevice(st, PT_GATHER_SPHERE, 5, dPts, dB) &&
                    hipMemcpy(dev, dA, sizeof(dev), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(dprobes, dB, sizeof(dprobes), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(dPts);
    (void)hipFree(dA);
    (void)hipFree(dB);
    if(!ok || std::memcmp(host, dev, sizeof(host)) != 0 || std::memcmp(probes, dprobes, sizeof(probes)) != 0)
    {
      std::printf("ERROR gatherDevice mode %d differs (%s)\n", mode, r.lastError().c_str());
      return 9;
    }
    const bool good = host[0].hitFraction == 1.f && host[1].hitFraction == 0.f && host[3].hitFraction == 0.f && host[1].irradiance[0] > 0.f && host[1].closestRays == 8 &&
                      host[4].status == PT_RAY_INVALID && host[4].seed == 5u && host[4].closestRays == 0 && host[4].irradiance[0] == 0.f && host[0].status == 0 && host[0].seed != 1u &&
                      probes[4].status == 0 && probes[4].closestRays >= 8 && probes[4].sh[0][0] > 0.f && probes[3].hitFraction == 0.f && probes[0]._pad == 0;
    if(!good)
    {
      std::printf("ERROR mode %d: hitFraction %.3f %.3f %.3f status %u %u irradiance %.3f sh %.3f\n", mode, host[0].hitFraction, host[1].hitFraction, host[3].hitFraction, host[4].status,
                  probes[4].status, host[1].irradiance[0], probes[4].sh[0][0]);
      return 10;
    }
    sums[mode == PT_ACCEL_TWO_LEVEL][0] = fnv(host, sizeof(host));
    sums[mode == PT_ACCEL_TWO_LEVEL][1] = fnv(probes, sizeof(probes));
  }
  if(r.gatherDevice(st, 2u, 5, pts, &none) || r.status() != PT_ERR_INVALID)  // an unknown kind
    return 11;
  std::printf("OK flat=%016llx two=%016llx flat_probes=%016llx two_probes=%016llx\n", sums[0][0], sums[1][0], sums[0][1], sums[1][1]);
  return 0;
}
