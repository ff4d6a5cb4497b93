// The host build of the motion of moving instances: vk_raytrace_amd/csrc/pt_motion.h -- the motion table and temporal_pixel_moving,
// what pt_temporal_accumulate_moving's kernels run per lane -- and instance_pixel<TWO> of pt_guides.h, what pt_render_instance_plane's kernel runs per
// lane, compiled by g++.  A library of its own (tests/motion_host.py compiles and binds it); the instance pass works on the scene handle a
// tests/host_harness.py TracedScene creates, like tests/cpp/guides_host.cpp.  tests/test_motion_model.py holds the table and the pixel to a float64 model,
// tests/test_instances_host.py the instance plane to the oracle; tests/test_motion_gpu.py and tests/test_instances_gpu.py hold the device to this build.
#include "th_walk.h"
#include "pt_guides.h"
#include "stage/history_step.h"

extern "C" {

// motion_table: hist / cur hold n instances of PT_MOTION_INSTANCE_WORDS words; out: n records of 28 words (toPrev[12], normalToPrev[12], moved, 3 of padding)
void mh_table(const float* hist, const float* cur, uint32_t n, void* out)
{
  static_assert(sizeof(MotionRec) == 28 * 4, "the record as tests/motion_host.py reads it");
  motion_table(hist, cur, n, static_cast<MotionRec*>(out));
}

// pt_temporal_accumulate_moving on the host: th_temporal's call (tests/cpp/temporal_host.cpp) with the instance plane (w * h words), which this form
// requires, the table (read only with a history) and, with hist_moments / out_moments, the moments image of pt_temporal_track_moments.
int mh_temporal_moving(const HistoryCall* q) { return q ? history_step(*q, q->ids != nullptr) : PT_ERR_INVALID; }

// pt_render_instance_plane on the host, on the flat (two = 0) or the two-level structure: ids (W * H words) and the guide planes in `planes` (which may
// be 0; out0 / out1 / out2 as gh_guides takes them).  The harness builds its flat structure without per-slot shading lines: the node index comes from the
// TriRec there (the device's PT_TUNE shadeTris=0), and the device's default form is held to it by equality.  Returns the traversal-stack overflows counted.
uint32_t mh_instances(void* p, int two, int W, int H, uint32_t planes, float miss_depth, uint32_t* ids, float* out0, float* out1, float* out2)
{
  Scene*             s = static_cast<Scene*>(p);
  const DeviceScene& S = two ? s->dsTwo : s->dsFlat;
  float* const       out[PT_DENOISE_GUIDES] = {out0, out1, out2};
  return for_each_ray((long long)W * H, 64, nullptr, [&](WalkCtx& c, long long i) {
    const int  px = int(i % W), py = int(i / W);
    GuidePixel g;
    ids[i] = two ? instance_pixel<true>(S, W, H, px, py, planes, miss_depth, c.stack.data(), &c.cnt, g)
                 : instance_pixel<false>(S, W, H, px, py, planes, miss_depth, c.stack.data(), &c.cnt, g);
    for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
      if(planes & (1u << j))
        std::memcpy(out[j] + size_t(i) * 4, &g.plane[j], 16);
  });
}
}
