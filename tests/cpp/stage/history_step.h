// One call of the history stage on the host (DESIGN.md sections 5.3 - 5.7): the pixel functions of pt_temporal.h, pt_motion.h, pt_albedo.h, pt_svgf.h and
// pt_fast.h as they stand, compiled by g++, over row-major images in ordinary memory.  The one image loop and the one statement of the argument checks
// behind the step entries of temporal_host.cpp, svgf_host.cpp, motion_host.cpp, albedo_host.cpp and fast_host.cpp, each of which includes this header
// into its one unit, adds what its form requires and calls history_step.  tests/history_host.py mirrors HistoryCall.
#pragma once
#include <cstddef>
#include <vector>
#include "pt_albedo.h"
#include "pt_fast.h"
#include "pt_motion.h"
#include "pt_svgf.h"
#include "stage_host_common.h"

// A call, by name.  Images are w * h pixels; NULL means "off" or "not asked for".
struct HistoryCall {
  // the current frame: colour, normal (guide plane 1), depth (guide plane 2) and, with pt_temporal_demodulate on, albedo (guide plane 0): 4 floats a pixel
  const float *colour, *albedo, *normal, *depth;
  int          w, h;
  const float *view_inverse, *proj_inverse;  // [16] each
  const pt_TemporalParams* params;
  // the history that is read (hist_colour NULL: a first call, and none of these is read): colour, guide [4], length [1], moments [2], the fast colour [4]
  // and length [1], and the camera it was made with: world_to_clip_h[16], eye_h[3]
  const float *hist_colour, *hist_guide, *hist_length, *hist_moments, *hist_fast, *hist_fast_length, *world_to_clip_h, *eye_h;
  // motion: the instance plane (one word a pixel; NULL: the static form) and the table, num_instances records as mh_table writes them
  const uint32_t* ids;
  const void*     table;
  uint32_t        num_instances;
  const pt_FastParams* fast;  // NULL: pt_temporal_fast off
  // the new history; unclamped: the long step's colour and length before the clamp, w * h * 5 floats (colour, then length)
  float *out_colour, *out_guide, *out_length, *out_moments, *out_fast, *out_fast_length, *unclamped;
  // the long step, looked into, per pixel: fxfy[2] (NaN where step 2 ended before they were formed), taps[8] (x, y of the four taps in tap order),
  // verdicts[4] (TemporalProbe::verdict), sw, outcome (PT_TEMPORAL_*), point[4] (P.xyz -- P' in the moving form -- and t_exp)
  float* fxfy;
  int *  taps, *verdicts;
  float* sw;
  int*   outcome;
  float* point;
};

// fast_clamp_pixel of (hc, hn) against (hf, hnf) over a w x h image into (out_colour, out_length), which may be (hc, hn): a pixel reads and writes the
// long history at itself only.  Any of the probe's outputs may be NULL: taps counted [1], mu / sigma / lo / hi [3 each], moved [1] per pixel.
static inline void clamp_image(const float* hf, const float* hnf, const float* hc, const float* hn, int w, int h, const FastConst& k, float* out_colour, float* out_length,
                               float* count = nullptr, float* mu = nullptr, float* sigma = nullptr, float* lo = nullptr, float* hi = nullptr, int* moved = nullptr)
{
  const FcRowMajor src{(const DnPx*)hf, hnf, w};
  const bool       look = count || mu || sigma || lo || hi || moved;
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      const size_t at = size_t(y) * size_t(w) + size_t(x);
      DnPx         c;
      std::memcpy(&c, hc + 4 * at, sizeof(DnPx));
      FastProbe     pr;
      const FastOut o = fast_clamp_pixel(src, k, c, hn[at], x, y, w, h, look ? &pr : nullptr);
      std::memcpy(out_colour + 4 * at, &o.colour, sizeof(DnPx));
      out_length[at] = o.length;
      if(count)
        count[at] = pr.n;
      for(int j = 0; j < 3; ++j)
      {
        if(mu)
          mu[3 * at + j] = pr.mu[j];
        if(sigma)
          sigma[3 * at + j] = pr.sigma[j];
        if(lo)
          lo[3 * at + j] = pr.lo[j];
        if(hi)
          hi[3 * at + j] = pr.hi[j];
      }
      if(moved)
        moved[at] = pr.moved;
    }
}

// The image loop: one temporal step through the reader `src`, its results into whichever of oc / og / on / om (the moments) is not NULL; probes: into
// the call's six probe outputs as well.  The static form gets a null probe where neither the moments nor a probe output is asked for.
template <bool MOVING, class Src>
static void step_image(const Src& src, const TemporalConst& k, const HistoryCall& q, float* oc, float* og, float* on, float* om, bool probes)
{
  const int                  w = q.w, h = q.h;
  const RowMajorMoments<SvM> msrc{(const SvM*)q.hist_moments, w};
  const uint32_t             n = q.hist_colour ? q.num_instances : 0u;  // (as the entry point: without a history there is no table)
  probes = probes && (q.fxfy || q.taps || q.verdicts || q.sw || q.outcome || q.point);
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      TemporalProbe pr;
      TemporalOut   o;
      if constexpr(MOVING)
        o = temporal_pixel_moving(src, k, static_cast<const MotionRec*>(q.table), n, x, y, w, h, &pr);
      else
        o = temporal_pixel(src, k, x, y, w, h, om || probes ? &pr : nullptr);
      const size_t at = size_t(y) * size_t(w) + size_t(x);
      if(oc)
        std::memcpy(oc + 4 * at, &o.colour, sizeof(DnPx));
      if(og)
        std::memcpy(og + 4 * at, &o.guide, sizeof(DnPx));
      if(on)
        on[at] = o.length;
      if(om)
      {
        const SvM m    = svgf_moments(msrc, pr, o, src.colour(x, y));  // (the reader's own colour: with the albedo, the moments are of the demodulated luminance)
        om[2 * at]     = m.x;
        om[2 * at + 1] = m.y;
      }
      if(!probes)
        continue;
      if(q.fxfy)
        q.fxfy[2 * at] = pr.fx, q.fxfy[2 * at + 1] = pr.fy;
      for(int i = 0; i < 4; ++i)
      {
        if(q.taps)
          q.taps[8 * at + 2 * i] = pr.tapX[i], q.taps[8 * at + 2 * i + 1] = pr.tapY[i];
        if(q.verdicts)
          q.verdicts[4 * at + i] = pr.verdict[i];
      }
      if(q.sw)
        q.sw[at] = pr.sw;
      if(q.outcome)
        q.outcome[at] = pr.outcome;
      if(q.point)
        q.point[4 * at] = pr.P[0], q.point[4 * at + 1] = pr.P[1], q.point[4 * at + 2] = pr.P[2], q.point[4 * at + 3] = pr.tExp;
    }
}

// ... through the reader the call's form asks for, over the history images (hc, hn) -- the long ones or the fast ones -- and the shared guide
static void step_form(const HistoryCall& q, const TemporalConst& k, const float* hc, const float* hn, float* oc, float* og, float* on, float* om, bool probes)
{
  const TpRowMajor planes{(const DnPx*)q.colour, (const DnPx*)q.normal, (const DnPx*)q.depth, (const DnPx*)hc, (const DnPx*)q.hist_guide, hn, q.w};
  const MoRowMajor moving{planes, q.ids};
  if(q.albedo && q.ids)
  {
    const AlRowMajor<MoRowMajor> mem{moving, (const DnPx*)q.albedo};
    step_image<true>(AlbedoDemod<AlRowMajor<MoRowMajor>>{mem}, k, q, oc, og, on, om, probes);
  }
  else if(q.albedo)
  {
    const AlRowMajor<TpRowMajor> mem{planes, (const DnPx*)q.albedo};
    step_image<false>(AlbedoDemod<AlRowMajor<TpRowMajor>>{mem}, k, q, oc, og, on, om, probes);
  }
  else if(q.ids)
    step_image<true>(moving, k, q, oc, og, on, om, probes);
  else
    step_image<false>(planes, k, q, oc, og, on, om, probes);
}

// pt_temporal_accumulate / pt_temporal_accumulate_moving on the host, under the settings the call names.  Returns what temporal_constants and, with
// q.fast, fast_constants return, PT_ERR_INVALID for a missing argument -- nothing is written then -- or PT_ERR_STATE where the two steps of a call with
// q.fast did not store the same guide.  With q.fast the long step writes out_colour / out_guide / out_length (/ out_moments), the fast step -- the same
// pixel function through the same reader, maxFast in the place of maxHistory, without moments -- out_fast / out_fast_length, and the clamp then runs in
// place on out_colour / out_length.  form_ok: the call has what the entry's form requires besides; checked with the other arguments.
static int history_step(const HistoryCall& q, bool form_ok = true)
{
  const char* why = "";
  int         rc  = temporal_constants(q.params, &why);
  if(rc != PT_OK)
    return rc;
  FastConst fk{};
  if(q.fast && (rc = fast_constants(q.fast, &fk, &why)) != PT_OK)
    return rc;
  if(!form_ok || !q.colour || !q.normal || !q.depth || !q.view_inverse || !q.proj_inverse || q.w <= 0 || q.h <= 0
     || (q.fast && (!q.out_colour || !q.out_guide || !q.out_length || !q.out_fast || !q.out_fast_length))
     || (q.hist_colour
         && (!q.hist_guide || !q.hist_length || !q.world_to_clip_h || !q.eye_h || (q.ids && q.num_instances && !q.table) || (q.out_moments && !q.hist_moments)
             || (q.fast && (!q.hist_fast || !q.hist_fast_length)))))
    return PT_ERR_INVALID;
  const TemporalConst k = temporal_const(q.view_inverse, q.proj_inverse, q.hist_colour ? q.world_to_clip_h : nullptr, q.hist_colour ? q.eye_h : nullptr, q.params);
  step_form(q, k, q.hist_colour, q.hist_length, q.out_colour, q.out_guide, q.out_length, q.out_moments, true);
  if(!q.fast)
    return PT_OK;
  const size_t       px = size_t(q.w) * size_t(q.h);
  std::vector<float> guide2(4 * px);  // the fast step's Hg': the same bits, checked below
  TemporalConst      kf = k;
  kf.maxHistory         = fk.maxFast;
  step_form(q, kf, q.hist_fast, q.hist_fast_length, q.out_fast, guide2.data(), q.out_fast_length, nullptr, false);
  if(std::memcmp(guide2.data(), q.out_guide, sizeof(float) * 4 * px) != 0)
    return PT_ERR_STATE;  // the two steps store the same guide
  if(q.unclamped)
  {
    std::memcpy(q.unclamped, q.out_colour, sizeof(float) * 4 * px);
    std::memcpy(q.unclamped + 4 * px, q.out_length, sizeof(float) * px);
  }
  clamp_image(q.out_fast, q.out_fast_length, q.out_colour, q.out_length, q.w, q.h, fk, q.out_colour, q.out_length);
  return PT_OK;
}

extern "C" {
// sizeof(HistoryCall), then the offset of each field in declaration order: what tests/history_host.py's Call is held to.  Returns how many there are;
// the first cap of them are written.
int hs_call_layout(size_t* out, int cap)
{
#define HS_AT(f) offsetof(HistoryCall, f)
  const size_t layout[] = {sizeof(HistoryCall), HS_AT(colour), HS_AT(albedo), HS_AT(normal), HS_AT(depth), HS_AT(w), HS_AT(h), HS_AT(view_inverse), HS_AT(proj_inverse),
                           HS_AT(params), HS_AT(hist_colour), HS_AT(hist_guide), HS_AT(hist_length), HS_AT(hist_moments), HS_AT(hist_fast), HS_AT(hist_fast_length),
                           HS_AT(world_to_clip_h), HS_AT(eye_h), HS_AT(ids), HS_AT(table), HS_AT(num_instances), HS_AT(fast), HS_AT(out_colour), HS_AT(out_guide),
                           HS_AT(out_length), HS_AT(out_moments), HS_AT(out_fast), HS_AT(out_fast_length), HS_AT(unclamped), HS_AT(fxfy), HS_AT(taps), HS_AT(verdicts),
                           HS_AT(sw), HS_AT(outcome), HS_AT(point)};
#undef HS_AT
  const int n = int(sizeof(layout) / sizeof(layout[0]));
  for(int i = 0; i < n && i < cap; ++i)
    out[i] = layout[i];
  return n;
}
}
