// The host build of the guide pass: vk_raytrace_amd/csrc/pt_guides.h -- guide_pixel<TWO> / guide_ray<TWO>, what pt_render_guides' kernel runs per lane --
// compiled by g++, on the structures th_scene.h assembles.  A library of its own (tests/guides_host.py compiles and binds it); the scene handle is the
// one tests/host_harness.py TracedScene creates, the camera the one th_set_camera put into it.  tests/test_guides_host.py holds it to the oracle,
// tests/test_guides_gpu.py holds the device to it.
#include "th_walk.h"
#include "pt_guides.h"

extern "C" {

// The planes of a W x H image on the flat (two = 0) or the two-level structure; out0 / out1 / out2: W * H * 4 floats each, written only for the planes
// in `planes` (the others may be NULL).  Returns the traversal-stack overflows counted.
uint32_t gh_guides(void* p, int two, int W, int H, uint32_t planes, float miss_depth, float* out0, float* out1, float* out2)
{
  Scene*             s = static_cast<Scene*>(p);
  const DeviceScene& S = two ? s->dsTwo : s->dsFlat;
  float* const       out[PT_DENOISE_GUIDES] = {out0, out1, out2};
  return for_each_ray((long long)W * H, 64, nullptr, [&](WalkCtx& c, long long i) {
    const int  px = int(i % W), py = int(i / W);
    GuidePixel g;
    if(two)
      guide_pixel<true>(S, W, H, px, py, planes, miss_depth, c.stack.data(), &c.cnt, g);
    else
      guide_pixel<false>(S, W, H, px, py, planes, miss_depth, c.stack.data(), &c.cnt, g);
    for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
      if(planes & (1u << j))
        std::memcpy(out[j] + size_t(i) * 4, &g.plane[j], 16);
  });
}

// Per pixel (row-major) of a W x H image on the flat structure: the camera ray (org, dir: W * H * 3 floats) and the RNG state before and after the
// closest-hit walk.  Returns the traversal-stack overflows counted.
uint32_t gh_rays(void* p, int W, int H, float* org, float* dir, uint32_t* seed_after_camera, uint32_t* seed_after_walk)
{
  Scene* s = static_cast<Scene*>(p);
  return for_each_ray((long long)W * H, 64, nullptr, [&](WalkCtx& c, long long i) {
    const GuideRay g = guide_ray<false>(s->dsFlat, W, H, int(i % W), int(i / W), c.stack.data(), &c.cnt);
    org[3 * i] = g.org.x; org[3 * i + 1] = g.org.y; org[3 * i + 2] = g.org.z;
    dir[3 * i] = g.dir.x; dir[3 * i + 1] = g.dir.y; dir[3 * i + 2] = g.dir.z;
    seed_after_camera[i] = g.seedCamera;
    seed_after_walk[i]   = g.seedWalk;
  });
}
}
