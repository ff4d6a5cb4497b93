// The temporal stage of the C++ shim (include/pt_renderer.hpp temporalAccumulate / temporalReset / readTemporalHistory / denoiseHistory /
// tonemapHistory) against the C ABI: compiles, links with libptmi.so and, with a GPU, runs one round -- two cameras, two images, planes installed by
// the caller -- and prints checksums of everything it reads back; tests/test_temporal_shim.py runs the same round through the Python route and
// compares.  Without a GPU setup() must fail loudly (no fallback).
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
  const int    W = 40, H = 24;
  const size_t n = size_t(W) * H;
  r.create({uint32_t(W), uint32_t(H)});
  pt_TemporalParams p{};
  p.depthTol = 0.05f, p.normalDist2 = 0.05f, p.maxHistory = 8.f;
  if(r.temporalAccumulate(p) || r.status() != PT_ERR_STATE)  // before a camera exists
  {
    std::printf("ERROR temporalAccumulate before setCamera: status %d\n", r.status());
    return 4;
  }
  std::vector<float> normal(n * 4), depth(n * 4, 0.f), img(n * 4), out(n * 4), hc(n * 4), hn(n), den(n * 4);
  shim_planes(W, H, normal, depth);
  if(!r.setDenoiseGuides(nullptr, normal.data(), depth.data()))
    return 5;
  const float up[3] = {0, 1, 0};
  for(int k = 0; k < 2; ++k)
  {
    const float    eye[3] = {0.05f * float(k), 0, 5}, center[3] = {0.05f * float(k), 0, 0};
    pt_SceneCamera cam{};
    if(pt_camera_lookat(eye, center, up, 60.f, float(W) / float(H), &cam) != PT_OK || pt_camera_world_to_clip(eye, center, up, 60.f, float(W) / float(H), p.worldToClip) != PT_OK)
      return 6;
    r.setCamera(cam);
    shim_image(img, k);
    r.writeAccum(img.data());
    if(!r.temporalAccumulate(p, k == 1 ? out.data() : nullptr))
    {
      std::printf("ERROR temporalAccumulate %d: %s\n", k, r.lastError().c_str());
      return 7;
    }
  }
  const pt_DenoiseParams dp{2, 1.0f, {1.0f, 0.3f, 0.5f}, 0u};
  const pt_Tonemapper tm = shim_tonemapper();
  std::vector<uint8_t> shown(n * 4), filtered(n * 4);
  if(!r.readTemporalHistory(hc.data(), hn.data()) || !r.denoiseHistory(dp, den.data()) || !r.tonemapHistory(nullptr, tm, shown.data()) || !r.tonemapHistory(&dp, tm, filtered.data()))
  {
    std::printf("ERROR reading the history: %s\n", r.lastError().c_str());
    return 8;
  }
  if(std::memcmp(out.data(), hc.data(), n * 16) != 0)
    return 9;
  if(!r.temporalReset() || r.readTemporalHistory(hc.data(), hn.data()) || r.status() != PT_ERR_STATE)
    return 10;
  std::printf("OK colour=%016llx length=%016llx denoised=%016llx shown=%016llx filtered=%016llx\n", fnv(out.data(), n * 16), fnv(hn.data(), n * 4), fnv(den.data(), n * 16),
              fnv(shown.data(), n * 4), fnv(filtered.data(), n * 4));
  return 0;
}
