// The variance-guided filter of the C++ shim (include/pt_renderer.hpp trackMoments / readTemporalMoments / svgfVariance / svgfHistory / tonemapSvgf)
// against the C ABI: compiles, links with libptmi.so and, with a GPU, runs one round -- tracking on, three images of a static camera, planes installed
// by the caller -- and prints checksums of everything it reads back; tests/test_svgf_shim.py runs the same round through the Python route and compares.
// Without a GPU setup() must fail loudly (no fallback).
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
  const pt_SvgfParams sp{3, 4.0f, 1.0e-4f, {1.0f, 0.3f, 0.5f}, 2.5f, 0u};
  std::vector<float>  normal(n * 4), depth(n * 4, 0.f), img(n * 4), filtered(n * 4), m(n * 2), v0(n), v(n);
  if(r.svgfVariance(sp, v0.data()) || r.status() != PT_ERR_STATE)  // there is no history
  {
    std::printf("ERROR svgfVariance without a history: status %d\n", r.status());
    return 4;
  }
  if(r.trackMoments(true) == false)
    return 5;
  shim_planes(W, H, normal, depth);
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
    shim_image(img, k);
    r.writeAccum(img.data());
    if(!r.temporalAccumulate(p))
    {
      std::printf("ERROR temporalAccumulate %d: %s\n", k, r.lastError().c_str());
      return 8;
    }
  }
  const pt_Tonemapper tm = shim_tonemapper();
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
