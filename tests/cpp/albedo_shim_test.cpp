// The demodulated history of the C++ shim (include/pt_renderer.hpp temporalDemodulate) against the C ABI: compiles, links with libptmi.so and, with a
// GPU, runs one round -- the setting and tracking on, three images of a static camera, all three planes installed by the caller -- and prints checksums of
// everything it reads back; tests/test_albedo_shim.py runs the same round through the Python route and compares.  Without a GPU setup() must fail loudly
// (no fallback).
#include <cstdio>
#include <cstring>
#include <vector>
#include "stage/shim_common.h"

// guide plane 0 of the round: 0.25 + ((7 x + 3 y) mod 13) / 16 in every channel (exact in fp32), alpha 1
static void albedo_plane(int W, int H, std::vector<float>& a)
{
  for(int y = 0; y < H; ++y)
    for(int x = 0; x < W; ++x)
    {
      float* p = &a[(size_t(y) * W + x) * 4];
      p[0] = p[1] = p[2] = 0.25f + float((7 * x + 3 * y) % 13) * 0.0625f;
      p[3] = 1.0f;
    }
}

int main()
{
  ptmi::HipPathTracer r;
  r.setup(0);
  if(!r.ok())
    return shim_no_device(r);
  const int    W = 40, H = 24;
  const size_t n = size_t(W) * H;
  r.create({uint32_t(W), uint32_t(H)});
  const pt_SvgfParams    sp{3, 4.0f, 1.0e-4f, {1.0e15f, 0.3f, 0.5f}, 2.5f, 0u};
  const pt_DenoiseParams dp{2, 0.5f, {1.0e15f, 0.3f, 0.5f}, 0u};
  std::vector<float>     albedo(n * 4), normal(n * 4), depth(n * 4, 0.f), img(n * 4), hist(n * 4), length(n), filtered(n * 4), denoised(n * 4), v(n);
  if(!r.temporalDemodulate(true) || !r.trackMoments(true))
    return 4;
  shim_planes(W, H, normal, depth);
  albedo_plane(W, H, albedo);
  const float       up[3] = {0, 1, 0}, eye[3] = {0, 0, 5}, center[3] = {0, 0, 0};
  pt_TemporalParams p{};
  p.depthTol = 0.05f, p.normalDist2 = 0.05f, p.maxHistory = 8.f;
  pt_SceneCamera cam{};
  if(pt_camera_lookat(eye, center, up, 60.f, float(W) / float(H), &cam) != PT_OK || pt_camera_world_to_clip(eye, center, up, 60.f, float(W) / float(H), p.worldToClip) != PT_OK)
    return 5;
  r.setCamera(cam);
  shim_image(img, 0);
  r.writeAccum(img.data());
  if(!r.setDenoiseGuides(nullptr, normal.data(), depth.data()))
    return 6;
  if(r.temporalAccumulate(p) || r.status() != PT_ERR_STATE)  // the setting is on and plane 0 is missing
  {
    std::printf("ERROR temporalAccumulate without the albedo: status %d\n", r.status());
    return 7;
  }
  if(!r.setDenoiseGuides(albedo.data(), normal.data(), depth.data()))
    return 8;
  for(int k = 0; k < 3; ++k)
  {
    shim_image(img, k);
    r.writeAccum(img.data());
    if(!r.temporalAccumulate(p))
    {
      std::printf("ERROR temporalAccumulate %d: %s\n", k, r.lastError().c_str());
      return 9;
    }
  }
  const pt_Tonemapper  tm = shim_tonemapper();
  std::vector<uint8_t> shown(n * 4), shownHistory(n * 4);
  if(!r.readTemporalHistory(hist.data(), length.data()) || !r.svgfHistory(sp, filtered.data(), v.data()) || !r.tonemapSvgf(sp, tm, shown.data())
     || !r.denoiseHistory(dp, denoised.data()) || !r.tonemapHistory(nullptr, tm, shownHistory.data()))
  {
    std::printf("ERROR reading the remodulated history: %s\n", r.lastError().c_str());
    return 10;
  }
  pt_DenoiseParams twice = dp;
  twice.flags            = PT_DENOISE_DEMODULATE;
  if(r.denoiseHistory(twice, denoised.data()) || r.status() != PT_ERR_STATE)  // already demodulated
    return 11;
  if(!r.temporalDemodulate(false) || r.readTemporalHistory(hist.data(), nullptr) || r.status() != PT_ERR_STATE)  // the change dropped the history
    return 12;
  std::printf("OK history=%016llx length=%016llx filtered=%016llx variance=%016llx shown=%016llx denoised=%016llx shownHistory=%016llx\n", fnv(hist.data(), n * 16),
              fnv(length.data(), n * 4), fnv(filtered.data(), n * 16), fnv(v.data(), n * 4), fnv(shown.data(), n * 4), fnv(denoised.data(), n * 16), fnv(shownHistory.data(), n * 4));
  return 0;
}
