// The host build of the demodulated history: vk_raytrace_amd/csrc/pt_albedo.h -- the reader adaptor in front of temporal_pixel,
// temporal_pixel_moving and svgf_moments, what the kernels of pt_albedo.hip run per lane, the one-pixel remodulation and the refusals with their texts --
// compiled by g++.  A library of its own (tests/albedo_host.py compiles and binds it).  tests/test_albedo_model.py holds it to the existing host builds
// fed the divided colour, bit for bit, and to the float64 model; tests/test_albedo_gpu.py holds the device to this build.
#include <cstring>
#include "pt_albedo.h"
#include "pt_motion.h"
#include "pt_svgf.h"

namespace {
struct AhMoments {
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
}  // namespace

extern "C" {

// pt_temporal_accumulate / pt_temporal_accumulate_moving with pt_temporal_demodulate on, on the host: the arguments of mh_temporal_moving
// (tests/cpp/motion_host.cpp) with the albedo plane (guide plane 0: w * h * 4 floats) after the colour.  ids == NULL: the static form (table and
// num_instances are not read).  hist_moments / out_moments both NULL: not tracked.  outcome (may be NULL): step 4's outcome per pixel.
int ah_temporal(const float* colour, const float* albedo, const float* normal, const float* depth, int w, int h, const float* view_inverse, const float* proj_inverse,
                const pt_TemporalParams* params, const float* hist_colour, const float* hist_guide, const float* hist_length, const float* world_to_clip_h, const float* eye_h,
                const uint32_t* ids, const void* table, uint32_t num_instances, const float* hist_moments, float* out_colour, float* out_guide, float* out_length,
                float* out_moments, int* outcome)
{
  const char* why = "";
  const int   rc  = temporal_constants(params, &why);
  if(rc != PT_OK)
    return rc;
  if(!colour || !albedo || !normal || !depth || !view_inverse || !proj_inverse || !out_colour || !out_guide || !out_length || w <= 0 || h <= 0
     || (hist_colour && (!hist_guide || !hist_length || !world_to_clip_h || !eye_h || (ids && num_instances && !table) || (out_moments && !hist_moments))))
    return PT_ERR_INVALID;
  const TemporalConst          k = temporal_const(view_inverse, proj_inverse, hist_colour ? world_to_clip_h : nullptr, hist_colour ? eye_h : nullptr, params);
  const TpRowMajor             planes{(const DnPx*)colour, (const DnPx*)normal, (const DnPx*)depth, (const DnPx*)hist_colour, (const DnPx*)hist_guide, hist_length, w};
  const AlRowMajor<TpRowMajor> mem{planes, (const DnPx*)albedo};
  const AlRowMajor<MoRowMajor> memMoving{{planes, ids}, (const DnPx*)albedo};
  const AlbedoDemod<AlRowMajor<TpRowMajor>> src{mem};
  const AlbedoDemod<AlRowMajor<MoRowMajor>> srcMoving{memMoving};
  const AhMoments msrc{(const SvM*)hist_moments, w};
  const uint32_t  n = hist_colour ? num_instances : 0u;  // (as the entry point: without a history there is no table)
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      TemporalProbe     pr;
      const TemporalOut o  = ids ? temporal_pixel_moving(srcMoving, k, static_cast<const MotionRec*>(table), n, x, y, w, h, &pr) : temporal_pixel(src, k, x, y, w, h, &pr);
      const size_t      at = size_t(y) * size_t(w) + size_t(x);
      std::memcpy(out_colour + 4 * at, &o.colour, sizeof(DnPx));
      std::memcpy(out_guide + 4 * at, &o.guide, sizeof(DnPx));
      out_length[at] = o.length;
      if(out_moments)
      {
        const SvM m             = svgf_moments(msrc, pr, o, src.colour(x, y));  // (the adaptor's read: the moments are of the demodulated luminance)
        out_moments[2 * at]     = m.x;
        out_moments[2 * at + 1] = m.y;
      }
      if(outcome)
        outcome[at] = pr.outcome;
    }
  return PT_OK;
}

// the remodulation of n pixels: out[i] = albedo_remodulate(x[i], albedo[i]); out may be x
void ah_remodulate(const float* x, const float* albedo, size_t n, float* out)
{
  for(size_t i = 0; i < n; ++i)
  {
    DnPx a, g;
    std::memcpy(&a, x + 4 * i, sizeof(DnPx));
    std::memcpy(&g, albedo + 4 * i, sizeof(DnPx));
    const DnPx r = albedo_remodulate(a, g);
    std::memcpy(out + 4 * i, &r, sizeof(DnPx));
  }
}

// the refusals, each with its text.  what 0: albedo_setting(a); 1: albedo_step_needs_plane(a, b); 2: albedo_need_plane(a, b); 3: albedo_denoise_flags(a, b)
int ah_refusal(int what, int a, uint32_t b, char* why_out, int cap)
{
  const char* why = "";
  const int   rc  = what == 0 ? albedo_setting(a, &why) : what == 1 ? albedo_step_needs_plane(a != 0, b, &why) : what == 2 ? albedo_need_plane(a != 0, b, &why) : albedo_denoise_flags(a != 0, b, &why);
  put_why(why, why_out, cap);
  return rc;
}
}
