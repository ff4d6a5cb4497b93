// The host build of the temporal stage: vk_raytrace_amd/csrc/pt_temporal.h compiled by g++, one whole call over row-major images in ordinary memory.
// tests/temporal_host.py compiles and binds it; tests/test_temporal_model.py holds it to a float64 model, tests/test_temporal_gpu.py holds the device to it.
#include <cstring>
#include <vector>
#include "pt_temporal.h"
#include "stage/stage_host_common.h"

namespace {
// the constants of a call; hist_colour == NULL: no history
int make_const(const float* view_inverse, const float* proj_inverse, const pt_TemporalParams* params, const float* hist_colour, const float* world_to_clip_h,
               const float* eye_h, TemporalConst& k)
{
  const char* why = "";
  const int   rc  = temporal_constants(params, &why);
  if(rc != PT_OK)
    return rc;
  if(!view_inverse || !proj_inverse || (hist_colour && (!world_to_clip_h || !eye_h)))
    return PT_ERR_INVALID;
  k = temporal_const(view_inverse, proj_inverse, hist_colour ? world_to_clip_h : nullptr, hist_colour ? eye_h : nullptr, params);
  return PT_OK;
}
}  // namespace

extern "C" {

// pt_temporal_accumulate on the host.  colour, normal (guide plane 1), depth (guide plane 2): w * h * 4 floats; the camera's inverses; the history that
// is read -- hist_colour, hist_guide (w * h * 4 floats), hist_length (w * h floats), world_to_clip_h[16], eye_h[3] -- or hist_colour == NULL for a first
// call; the three new history images out.  Returns what temporal_constants returns; nothing is written on an error.
int th_temporal(const float* colour, const float* normal, const float* depth, int w, int h, const float* view_inverse, const float* proj_inverse,
                const pt_TemporalParams* params, const float* hist_colour, const float* hist_guide, const float* hist_length, const float* world_to_clip_h,
                const float* eye_h, float* out_colour, float* out_guide, float* out_length)
{
  TemporalConst k;
  const int     rc = make_const(view_inverse, proj_inverse, params, hist_colour, world_to_clip_h, eye_h, k);
  if(rc != PT_OK)
    return rc;
  if(!colour || !normal || !depth || !out_colour || !out_guide || !out_length || w <= 0 || h <= 0 || (hist_colour && (!hist_guide || !hist_length)))
    return PT_ERR_INVALID;
  const TpRowMajor src{(const DnPx*)colour, (const DnPx*)normal, (const DnPx*)depth, (const DnPx*)hist_colour, (const DnPx*)hist_guide, hist_length, w};
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      const TemporalOut o  = temporal_pixel(src, k, x, y, w, h, nullptr);
      const size_t      at = size_t(y) * size_t(w) + size_t(x);
      std::memcpy(out_colour + 4 * at, &o.colour, sizeof(DnPx));
      std::memcpy(out_guide + 4 * at, &o.guide, sizeof(DnPx));
      out_length[at] = o.length;
    }
  return PT_OK;
}

// The same call, looked into: per pixel fxfy[2] (NaN where step 2 ended before they were formed), taps[8] (x, y of the four taps in tap order),
// verdicts[4] (TemporalProbe::verdict), sw, outcome (PT_TEMPORAL_*), point[4] (P.xyz, t_exp).  Any output may be NULL.
int th_temporal_probe(const float* colour, const float* normal, const float* depth, int w, int h, const float* view_inverse, const float* proj_inverse,
                      const pt_TemporalParams* params, const float* hist_colour, const float* hist_guide, const float* hist_length,
                      const float* world_to_clip_h, const float* eye_h, float* fxfy, int* taps, int* verdicts, float* sw, int* outcome, float* point)
{
  TemporalConst k;
  const int     rc = make_const(view_inverse, proj_inverse, params, hist_colour, world_to_clip_h, eye_h, k);
  if(rc != PT_OK)
    return rc;
  if(!colour || !normal || !depth || w <= 0 || h <= 0 || (hist_colour && (!hist_guide || !hist_length)))
    return PT_ERR_INVALID;
  const TpRowMajor src{(const DnPx*)colour, (const DnPx*)normal, (const DnPx*)depth, (const DnPx*)hist_colour, (const DnPx*)hist_guide, hist_length, w};
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      TemporalProbe pr;
      (void)temporal_pixel(src, k, x, y, w, h, &pr);
      const size_t at = size_t(y) * size_t(w) + size_t(x);
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

// temporal_constants: the status, and the static reason in why_out (why_len bytes, may be NULL)
int th_temporal_constants(const pt_TemporalParams* params, char* why_out, int why_len)
{
  const char* why = "";
  const int   rc  = temporal_constants(params, &why);
  copy_why(why, why_out, why_len);
  return rc;
}
}
