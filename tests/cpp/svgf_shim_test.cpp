// The variance-guided filter of the C++ shim (include/pt_renderer.hpp trackMoments / readTemporalMoments / svgfVariance / svgfHistory / tonemapSvgf)
// against the C ABI: compiles, links with libptmi.so and, with a GPU, runs one round -- tracking on, three images of a static camera, planes installed
// by the caller -- and prints checksums of everything it reads back; tests/test_svgf_shim.py runs the same round through the Python route and compares.
// Without a GPU setup() must fail loudly (no fallback).
#include <cstdio>
#include <cstring>
#include <vector>
#include "pt_renderer.hpp"

static unsigned long long fnv(const void* p, size_t bytes)
{
  unsigned long long   h = 1469598103934665603ull;
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for(size_t i = 0; i < bytes; ++i)
    h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

int main()
{
  ptmi::HipPathTracer r;
  r.setup(0);
  if(!r.ok())
  {
    std::printf("NO_DEVICE status=%d msg=%s\n", r.status(), r.lastError().c_str());
    return r.status() == PT_ERR_NO_DEVICE ? 0 : 3;
  }
  const int    W = 40, H = 24;
  const size_t n = size_t(W) * H;
  r.create({uint32_t(W), uint32_t(H)});
  const pt_SvgfParams sp{3, 4.0f, 1.0e-4f, {1.0f, 0.3f, 0.5f}, 2.5f, 0u};
  std::vector<float>  normal(n * 4), depth(n * 4, 0.f), img(n * 4), filtered(n * 4), m(n * 2), v0(n), v(n);
  if(r.svgfVariance(sp, v0.data()) || r.status() != PT_ERR_STATE)  // there is no history
  {
    std::printf("ERROR svgfVariance without a history: status %d\n", r.status());
    return 4;
  }
  if(r.trackMoments(true) == false)
    return 5;
  for(int y = 0; y < H; ++y)
    for(int x = 0; x < W; ++x)
    {
      const size_t at = (size_t(y) * W + x) * 4;
      normal[at] = 0.5f, normal[at + 1] = 0.5f, normal[at + 2] = 1.f, normal[at + 3] = 1.f;
      depth[at] = 4.f + float((x * 3 + y * 5) % 16) * 0.125f;
    }
  if(!r.setDenoiseGuides(nullptr, normal.data(), depth.data()))
    return 6;
  const float       up[3] = {0, 1, 0}, eye[3] = {0, 0, 5}, center[3] = {0, 0, 0};
  pt_TemporalParams p{};
  p.depthTol = 0.05f, p.normalDist2 = 0.05f, p.maxHistory = 8.f;
  pt_SceneCamera cam{};
  if(pt_camera_lookat(eye, center, up, 60.f, float(W) / float(H), &cam) != PT_OK || pt_camera_world_to_clip(eye, center, up, 60.f, float(W) / float(H), p.worldToClip) != PT_OK)
    return 7;
  r.setCamera(cam);
  for(int k = 0; k < 3; ++k)
  {
    for(size_t i = 0; i < n * 4; ++i)
      img[i] = float((i * (37u + 4u * unsigned(k))) % 101u) / 50.f;
    r.writeAccum(img.data());
    if(!r.temporalAccumulate(p))
    {
      std::printf("ERROR temporalAccumulate %d: %s\n", k, r.lastError().c_str());
      return 8;
    }
  }
  pt_Tonemapper tm{};
  tm.brightness = 1.f, tm.contrast = 1.f, tm.saturation = 1.f, tm.vignette = 0.f, tm.avgLum = 1.f, tm.zoom = 1.f, tm.renderingRatio[0] = tm.renderingRatio[1] = 1.f;
  tm.autoExposure = 0, tm.Ywhite = 0.5f, tm.key = 0.5f, tm.dither = 1;
  std::vector<uint8_t> shown(n * 4);
  if(!r.readTemporalMoments(m.data()) || !r.svgfVariance(sp, v0.data()) || !r.svgfHistory(sp, filtered.data(), v.data()) || !r.tonemapSvgf(sp, tm, shown.data()))
  {
    std::printf("ERROR reading the filtered history: %s\n", r.lastError().c_str());
    return 9;
  }
  pt_SvgfParams bad = sp;
  bad.sigmaLum      = 0.f;
  if(r.svgfHistory(bad, filtered.data()) || r.status() != PT_ERR_INVALID)
    return 10;
  if(!r.trackMoments(false) || r.readTemporalMoments(m.data()) || r.status() != PT_ERR_STATE)  // the change dropped the history
    return 11;
  std::printf("OK moments=%016llx v0=%016llx filtered=%016llx variance=%016llx shown=%016llx\n", fnv(m.data(), n * 8), fnv(v0.data(), n * 4), fnv(filtered.data(), n * 16),
              fnv(v.data(), n * 4), fnv(shown.data(), n * 4));
  return 0;
}
