// The host build of the responsive history: vk_raytrace_amd/csrc/pt_fast.h -- the refusals with their texts and fast_clamp_pixel,
// what k_fast_clamp runs per lane -- behind the two temporal steps of a call, which are the pixel functions of pt_temporal.h, pt_motion.h, pt_albedo.h and
// pt_svgf.h as they stand, compiled by g++.  A library of its own (tests/fast_host.py compiles and binds it).  tests/test_fast_model.py holds it to the
// parent's host builds bit for bit and to the float64 model; tests/test_fast_gpu.py holds the device to this build.
#include <cstring>
#include <vector>
#include "pt_albedo.h"
#include "pt_fast.h"
#include "pt_motion.h"
#include "pt_svgf.h"

namespace {
struct FhMoments {
  const SvM* hm;
  int        w;
  SvM        histMoments(int x, int y) const { return hm[size_t(y) * size_t(w) + size_t(x)]; }
};
void put_why(const char* why, char* out, int cap)
{
  if(out && cap > 0)
  {
    std::strncpy(out, why, size_t(cap) - 1);
    out[cap - 1] = 0;
  }
}

// one temporal step over the whole image through the reader `src`; table == NULL: the static form; out_moments == NULL: without moments
template <class Src>
void step(const Src& src, const TemporalConst& k, const MotionRec* table, uint32_t n, bool moving, const FhMoments& msrc, int w, int h, float* out_colour, float* out_guide,
          float* out_length, float* out_moments)
{
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      TemporalProbe pr;
      const TemporalOut o  = moving ? temporal_pixel_moving(src, k, table, n, x, y, w, h, &pr) : temporal_pixel(src, k, x, y, w, h, &pr);
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
    }
}
}  // namespace

extern "C" {

// fast_constants: (status, reason)
int fh_constants(const pt_FastParams* p, char* why_out, int cap)
{
  const char* why = "";
  FastConst   k;
  const int   rc = fast_constants(p, &k, &why);
  put_why(why, why_out, cap);
  return rc;
}
// fast_need_history
int fh_need_history(int hist_fast, char* why_out, int cap)
{
  const char* why = "";
  const int   rc  = fast_need_history(hist_fast != 0, &why);
  put_why(why, why_out, cap);
  return rc;
}

// The clamp alone over a w x h image: fast_clamp_pixel of (hc, hn) against (hf, hnf) into out_colour / out_length (which may not alias the inputs).
// Any of the probe's outputs may be NULL: taps counted [1], mu / sigma / lo / hi [3 each], moved [1] per pixel.
int fh_clamp(const float* hf, const float* hnf, const float* hc, const float* hn, int w, int h, const pt_FastParams* fast, float* out_colour, float* out_length, float* count,
             float* mu, float* sigma, float* lo, float* hi, int* moved)
{
  const char* why = "";
  FastConst   k;
  const int   rc = fast_constants(fast, &k, &why);
  if(rc != PT_OK)
    return rc;
  if(!hf || !hnf || !hc || !hn || !out_colour || !out_length || w <= 0 || h <= 0)
    return PT_ERR_INVALID;
  const FcRowMajor src{(const DnPx*)hf, hnf, w};
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      const size_t at = size_t(y) * size_t(w) + size_t(x);
      DnPx         c;
      std::memcpy(&c, hc + 4 * at, sizeof(DnPx));
      FastProbe     pr;
      const FastOut o = fast_clamp_pixel(src, k, c, hn[at], x, y, w, h, &pr);
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
  return PT_OK;
}

// pt_temporal_accumulate / pt_temporal_accumulate_moving with pt_temporal_fast on, on the host: the arguments of ah_temporal (tests/cpp/albedo_host.cpp;
// albedo == NULL: pt_temporal_demodulate off) with the fast parameters after the temporal ones and the fast history (hist_fast, hist_fast_length) after
// the long one.  The long step writes out_colour / out_guide / out_length (/ out_moments), the fast step -- the same pixel function through the same
// reader, maxFast in the place of maxHistory, without moments -- out_fast / out_fast_length, and the clamp then runs in place on out_colour / out_length.
// unclamped (may be NULL): the long step's colour and length before the clamp, w * h * 5 floats (colour, then length).
int fh_step(const float* colour, const float* albedo, const float* normal, const float* depth, int w, int h, const float* view_inverse, const float* proj_inverse,
            const pt_TemporalParams* params, const pt_FastParams* fast, const float* hist_colour, const float* hist_guide, const float* hist_length, const float* hist_fast,
            const float* hist_fast_length, const float* world_to_clip_h, const float* eye_h, const uint32_t* ids, const void* table, uint32_t num_instances,
            const float* hist_moments, float* out_colour, float* out_guide, float* out_length, float* out_fast, float* out_fast_length, float* out_moments, float* unclamped)
{
  const char* why = "";
  int         rc  = temporal_constants(params, &why);
  if(rc != PT_OK)
    return rc;
  FastConst fk;
  rc = fast_constants(fast, &fk, &why);
  if(rc != PT_OK)
    return rc;
  if(!colour || !normal || !depth || !view_inverse || !proj_inverse || !out_colour || !out_guide || !out_length || !out_fast || !out_fast_length || w <= 0 || h <= 0
     || (hist_colour && (!hist_guide || !hist_length || !hist_fast || !hist_fast_length || !world_to_clip_h || !eye_h || (ids && num_instances && !table) || (out_moments && !hist_moments))))
    return PT_ERR_INVALID;
  const size_t        px = size_t(w) * size_t(h);
  const TemporalConst k  = temporal_const(view_inverse, proj_inverse, hist_colour ? world_to_clip_h : nullptr, hist_colour ? eye_h : nullptr, params);
  TemporalConst       kf = k;
  kf.maxHistory          = fk.maxFast;
  const uint32_t   n     = hist_colour ? num_instances : 0u;  // (as the entry point: without a history there is no table)
  const MotionRec* tab   = static_cast<const MotionRec*>(table);
  const FhMoments  msrc{(const SvM*)hist_moments, w};
  const bool       moving = ids != nullptr;
  std::vector<uint32_t> none(moving ? 0 : px, PT_INSTANCE_NONE);  // (the static form never asks for an instance)
  const uint32_t*  plane = moving ? ids : none.data();
  std::vector<float> guide2(4 * px);  // the fast step's Hg': the same bits, checked below
  for(int pass = 0; pass < 2; ++pass)
  {
    const bool       isFast = pass == 1;
    const TpRowMajor planes{(const DnPx*)colour, (const DnPx*)normal, (const DnPx*)depth, (const DnPx*)(isFast ? hist_fast : hist_colour), (const DnPx*)hist_guide,
                            isFast ? hist_fast_length : hist_length, w};
    const MoRowMajor mem{planes, plane};
    float *const oc = isFast ? out_fast : out_colour, *const og = isFast ? guide2.data() : out_guide, *const on = isFast ? out_fast_length : out_length;
    float* const om = isFast ? nullptr : out_moments;
    if(albedo)
    {
      const AlRowMajor<MoRowMajor>              memA{mem, (const DnPx*)albedo};
      const AlbedoDemod<AlRowMajor<MoRowMajor>> src{memA};
      step(src, isFast ? kf : k, tab, n, moving, msrc, w, h, oc, og, on, om);
    }
    else
      step(mem, isFast ? kf : k, tab, n, moving, msrc, w, h, oc, og, on, om);
  }
  if(std::memcmp(guide2.data(), out_guide, sizeof(float) * 4 * px) != 0)
    return PT_ERR_STATE;  // the two steps store the same guide
  if(unclamped)
  {
    std::memcpy(unclamped, out_colour, sizeof(float) * 4 * px);
    std::memcpy(unclamped + 4 * px, out_length, sizeof(float) * px);
  }
  const FcRowMajor src{(const DnPx*)out_fast, out_fast_length, w};
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      const size_t at = size_t(y) * size_t(w) + size_t(x);
      DnPx         c;
      std::memcpy(&c, out_colour + 4 * at, sizeof(DnPx));
      const FastOut o = fast_clamp_pixel(src, fk, c, out_length[at], x, y, w, h, nullptr);  // in place: a pixel reads and writes the long history at itself only
      std::memcpy(out_colour + 4 * at, &o.colour, sizeof(DnPx));
      out_length[at] = o.length;
    }
  return PT_OK;
}
}
