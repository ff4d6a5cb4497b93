// The responsive history of the C++ shim (include/pt_renderer.hpp temporalFast, readTemporalFast) against the C ABI: compiles, links with libptmi.so and,
// with a GPU, runs one round -- the setting on, four images of a static camera of which the last is three times as bright -- and prints checksums of
// everything it reads back; tests/test_fast_shim.py runs the same round through the Python route and compares.  Without a GPU setup() must fail loudly
// (no fallback).
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
  std::vector<float> normal(n * 4), depth(n * 4, 0.f), img(n * 4), out(n * 4), hist(n * 4), length(n), fast(n * 4), fastLength(n);
  pt_FastParams      fp{2.0f, 1.0f, 2, 0u};
  pt_FastParams      bad = fp;
  bad.radius          = 4;
  if(r.temporalFast(&bad) || r.status() != PT_ERR_INVALID)  // refused, and the setting stays off
  {
    std::printf("ERROR temporalFast with radius 4: status %d\n", r.status());
    return 4;
  }
  if(!r.temporalFast(&fp))
    return 5;
  shim_planes(W, H, normal, depth);
  const float       up[3] = {0, 1, 0}, eye[3] = {0, 0, 5}, center[3] = {0, 0, 0};
  pt_TemporalParams p{};
  p.depthTol = 0.05f, p.normalDist2 = 0.05f, p.maxHistory = 8.f;
  pt_SceneCamera cam{};
  if(pt_camera_lookat(eye, center, up, 60.f, float(W) / float(H), &cam) != PT_OK || pt_camera_world_to_clip(eye, center, up, 60.f, float(W) / float(H), p.worldToClip) != PT_OK)
    return 6;
  r.setCamera(cam);
  if(!r.setDenoiseGuides(nullptr, normal.data(), depth.data()))
    return 7;
  if(r.readTemporalFast(fast.data(), fastLength.data()) || r.status() != PT_ERR_STATE)  // no history yet
    return 8;
  for(int k = 0; k < 4; ++k)
  {
    shim_image(img, k);
    if(k == 3)
      for(float& v : img)
        v *= 3.0f;
    r.writeAccum(img.data());
    if(!r.temporalAccumulate(p, out.data()))
    {
      std::printf("ERROR temporalAccumulate %d: %s\n", k, r.lastError().c_str());
      return 9;
    }
  }
  const pt_Tonemapper  tm = shim_tonemapper();
  std::vector<uint8_t> shown(n * 4);
  if(!r.readTemporalHistory(hist.data(), length.data()) || !r.readTemporalFast(fast.data(), fastLength.data()) || !r.tonemapHistory(nullptr, tm, shown.data()))
  {
    std::printf("ERROR reading the histories: %s\n", r.lastError().c_str());
    return 10;
  }
  if(std::memcmp(out.data(), hist.data(), n * 16) != 0)  // the returned image is the clamped history
    return 11;
  fp.sigmaScale = 3.0f;
  if(!r.temporalFast(&fp) || !r.readTemporalFast(nullptr, fastLength.data()))  // new parameters keep the history
    return 12;
  if(!r.temporalFast(nullptr) || r.readTemporalHistory(hist.data(), nullptr) || r.status() != PT_ERR_STATE)  // off: the change dropped the history
    return 13;
  std::printf("OK returned=%016llx length=%016llx fast=%016llx fastLength=%016llx shown=%016llx\n", fnv(out.data(), n * 16), fnv(length.data(), n * 4), fnv(fast.data(), n * 16),
              fnv(fastLength.data(), n * 4), fnv(shown.data(), n * 4));
  return 0;
}
