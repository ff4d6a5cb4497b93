// The ray queries of the C++ shim (include/pt_renderer.hpp traceRays / traceRaysDevice) against the C ABI: compiles, links with libptmi.so and, with a
// GPU, traces a few rays at a quad -- through host arrays and through device memory of the caller's own (hipMalloc) -- with the same results.
// Without a GPU setup() must fail loudly (no fallback).
#include <hip/hip_runtime_api.h>
#include <cmath>
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
  m.pbrBaseColorFactor[0] = m.pbrBaseColorFactor[1] = m.pbrBaseColorFactor[2] = 0.8f;
  m.pbrBaseColorFactor[3] = 1.f;
  m.pbrBaseColorTexture = m.pbrMetallicRoughnessTexture = m.emissiveTexture = m.normalTexture = m.transmissionTexture = m.clearcoatTexture = m.clearcoatRoughnessTexture = m.thicknessTexture = -1;
  m.pbrRoughnessFactor = 1.f; m.ior = 1.5f; m.doubleSided = 0; m.attenuationDistance = 3.4e38f;
  m.attenuationColor[0] = m.attenuationColor[1] = m.attenuationColor[2] = 1.f;
  for(int i = 0; i < 4; ++i) m.uvTransform[i * 5] = 1.f;
  pt_SceneDesc sd{v, 4, idx, 6, &pm, 1, &nd, 1, &m, 1, nullptr, 0, nullptr, 0};
  pt_Ray one{{0, 0, 3}, 10.f, {0, 0, -1}, 7u};
  pt_RayHit none{};
  if(r.traceRays(PT_RAYS_NEAREST, 1, &one, &none) || r.status() != PT_ERR_STATE)  // before a scene exists
  {
    std::printf("ERROR traceRays before create: status %d\n", r.status());
    return 4;
  }
  r.create({64, 64}, &sd);
  for(int mode : {PT_ACCEL_FLAT, PT_ACCEL_TWO_LEVEL})
  {
    r.setAccelMode(mode);
    // towards the quad's front (hit in triangle 0: x > y), its other triangle, past it, at its back (culled; the picker's ray still hits), and an invalid ray
    const pt_Ray rays[5] = {{{0.5f, -0.5f, 3}, 10.f, {0, 0, -1}, 1u}, {{-0.5f, 0.5f, 3}, 10.f, {0, 0, -1}, 2u}, {{3, 3, 3}, 10.f, {0, 0, -1}, 3u},
                            {{0.5f, -0.5f, -3}, 10.f, {0, 0, 1}, 4u}, {{0, 0, 3}, 10.f, {0, 0, 0}, 5u}};
    for(int kind : {PT_RAYS_CLOSEST, PT_RAYS_OCCLUDED, PT_RAYS_NEAREST, PT_RAYS_CANDIDATES})
    {
      const uint32_t hpr = kind == PT_RAYS_CANDIDATES ? 2u : 1u;
      std::vector<pt_RayHit> host(5 * hpr), dev(5 * hpr);
      if(!r.traceRays(kind, 5, rays, host.data(), hpr))
      {
        std::printf("ERROR traceRays kind %d: %s\n", kind, r.lastError().c_str());
        return 5;
      }
      pt_Ray*    dRays = nullptr;
      pt_RayHit* dHits = nullptr;
      if(hipMalloc((void**)&dRays, sizeof(rays)) != hipSuccess || hipMalloc((void**)&dHits, sizeof(pt_RayHit) * dev.size()) != hipSuccess ||
         hipMemcpy(dRays, rays, sizeof(rays), hipMemcpyHostToDevice) != hipSuccess)
        return 6;
      const bool ok = r.traceRaysDevice(kind, 5, dRays, dHits, hpr) && hipMemcpy(dev.data(), dHits, sizeof(pt_RayHit) * dev.size(), hipMemcpyDeviceToHost) == hipSuccess;
      (void)hipFree(dRays);
      (void)hipFree(dHits);
      if(!ok || std::memcmp(host.data(), dev.data(), sizeof(pt_RayHit) * dev.size()) != 0)
      {
        std::printf("ERROR traceRaysDevice kind %d mode %d differs (%s)\n", kind, mode, r.lastError().c_str());
        return 7;
      }
      const pt_RayHit *h0 = &host[0], *h1 = &host[hpr], *h2 = &host[2 * hpr], *h3 = &host[3 * hpr], *h4 = &host[4 * hpr];
      const bool back = kind == PT_RAYS_NEAREST;  // every triangle counts for the picker's ray only
      bool       good = h0->status == PT_RAY_HIT && h1->status == PT_RAY_HIT && h2->status == 0 && h3->status == (back ? PT_RAY_HIT : 0u) && h4->status == PT_RAY_INVALID && h4->seed == 5u;
      if(kind != PT_RAYS_OCCLUDED)
        good = good && std::fabs(h0->t - 3.f) < 1e-5f && h0->instanceID == 0 && h0->instanceCustomIndex == 0 && h0->primitiveID == 0 && h1->primitiveID == 1 && h2->instanceID == 0xffffffffu && h2->primitiveID == -1 &&
               std::fabs(h0->u + h0->v - 0.75f) < 1e-5f;
      if(kind == PT_RAYS_CANDIDATES)
        good = good && host[1].status == 0 && host[1].primitiveID == -1;
      if(!good)
      {
        std::printf("ERROR kind %d mode %d: status %u %u %u %u %u t %.3f prim %d %d\n", kind, mode, h0->status, h1->status, h2->status, h3->status, h4->status, h0->t, h0->primitiveID, h1->primitiveID);
        return 8;
      }
    }
  }
  std::printf("OK\n");
  return 0;
}
