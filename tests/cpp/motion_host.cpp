// The host build of the motion of moving instances: vk_raytrace_amd/csrc/pt_motion.h -- the motion table and temporal_pixel_moving,
// what pt_temporal_accumulate_moving's kernels run per lane -- and instance_pixel<TWO> of pt_guides.h, what pt_render_instance_plane's kernel runs per
// lane, compiled by g++.  A library of its own (tests/motion_host.py compiles and binds it); the instance pass works on the scene handle a
// tests/host_harness.py TracedScene creates, like tests/cpp/guides_host.cpp.  tests/test_motion_model.py holds the table and the pixel to a float64 model,
// tests/test_instances_host.py the instance plane to the oracle; tests/test_motion_gpu.py and tests/test_instances_gpu.py hold the device to this build.
#include "th_walk.h"
#include "pt_guides.h"
#include "pt_motion.h"
#include "pt_svgf.h"

namespace {
struct MoMoments {
  const SvM* hm;
  int        w;
  SvM        histMoments(int x, int y) const { return hm[size_t(y) * size_t(w) + size_t(x)]; }
};
}  // namespace

extern "C" {

// motion_table: hist / cur hold n instances of PT_MOTION_INSTANCE_WORDS words; out: n records of 28 words (toPrev[12], normalToPrev[12], moved, 3 of padding)
void mh_table(const float* hist, const float* cur, uint32_t n, void* out)
{
  static_assert(sizeof(MotionRec) == 28 * 4, "the record as tests/motion_host.py reads it");
  motion_table(hist, cur, n, static_cast<MotionRec*>(out));
}

// pt_temporal_accumulate_moving on the host: the arguments of th_temporal (tests/cpp/temporal_host.cpp), then the instance plane (w * h words), the table
// (num_instances records as mh_table writes them; read only with a history) and, with hist_moments / out_moments, the moments image of
// pt_temporal_track_moments (both NULL: not tracked).  Any of the probe's outputs may be NULL: fxfy[2], taps[8], verdicts[4], sw, outcome, point[4]
// (P'.xyz, t_exp) per pixel, as th_temporal_probe hands them out.
int mh_temporal_moving(const float* colour, const float* normal, const float* depth, int w, int h, const float* view_inverse, const float* proj_inverse,
                       const pt_TemporalParams* params, const float* hist_colour, const float* hist_guide, const float* hist_length, const float* world_to_clip_h,
                       const float* eye_h, const uint32_t* ids, const void* table, uint32_t num_instances, const float* hist_moments, float* out_colour, float* out_guide,
                       float* out_length, float* out_moments, float* fxfy, int* taps, int* verdicts, float* sw, int* outcome, float* point)
{
  const char* why = "";
  const int   rc  = temporal_constants(params, &why);
  if(rc != PT_OK)
    return rc;
  if(!colour || !normal || !depth || !view_inverse || !proj_inverse || !ids || !out_colour || !out_guide || !out_length || w <= 0 || h <= 0
     || (hist_colour && (!hist_guide || !hist_length || !world_to_clip_h || !eye_h || (num_instances && !table) || (out_moments && !hist_moments))))
    return PT_ERR_INVALID;
  const TemporalConst k = temporal_const(view_inverse, proj_inverse, hist_colour ? world_to_clip_h : nullptr, hist_colour ? eye_h : nullptr, params);
  MoRowMajor          src{{(const DnPx*)colour, (const DnPx*)normal, (const DnPx*)depth, (const DnPx*)hist_colour, (const DnPx*)hist_guide, hist_length, w}, ids};
  const MoMoments     msrc{(const SvM*)hist_moments, w};
  const uint32_t      n = hist_colour ? num_instances : 0u;  // (as the entry point: without a history there is no table)
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      TemporalProbe     pr;
      const TemporalOut o  = temporal_pixel_moving(src, k, static_cast<const MotionRec*>(table), n, x, y, w, h, &pr);
      const size_t      at = size_t(y) * size_t(w) + size_t(x);
      std::memcpy(out_colour + 4 * at, &o.colour, sizeof(DnPx));
      std::memcpy(out_guide + 4 * at, &o.guide, sizeof(DnPx));
      out_length[at] = o.length;
      if(out_moments)
      {
        const SvM m             = svgf_moments(msrc, pr, o, src.colour(x, y));
        out_moments[2 * at]     = m.x;
        out_moments[2 * at + 1] = m.y;
      }
      if(fxfy)
        fxfy[2 * at] = pr.fx, fxfy[2 * at + 1] = pr.fy;
      for(int i = 0; i < 4; ++i)
      {
        if(taps)
          taps[8 * at + 2 * i] = pr.tapX[i], taps[8 * at + 2 * i + 1] = pr.tapY[i];
        if(verdicts)
          verdicts[4 * at + i] = pr.verdict[i];
      }
      if(sw)
        sw[at] = pr.sw;
      if(outcome)
        outcome[at] = pr.outcome;
      if(point)
        point[4 * at] = pr.P[0], point[4 * at + 1] = pr.P[1], point[4 * at + 2] = pr.P[2], point[4 * at + 3] = pr.tExp;
    }
  return PT_OK;
}

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
