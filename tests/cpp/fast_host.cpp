// The host build of the responsive history: vk_raytrace_amd/csrc/pt_fast.h -- the refusals with their texts and fast_clamp_pixel,
// what k_fast_clamp runs per lane -- behind the two temporal steps of a call, which are the pixel functions of pt_temporal.h, pt_motion.h, pt_albedo.h and
// pt_svgf.h as they stand (stage/history_step.h), compiled by g++.  A library of its own (tests/fast_host.py compiles and binds it).
// tests/test_fast_model.py holds it to the parent's host builds bit for bit and to the float64 model; tests/test_fast_gpu.py holds the device to this build.
#include "stage/history_step.h"

extern "C" {

// fast_constants: (status, reason)
int fh_constants(const pt_FastParams* p, char* why_out, int cap)
{
  const char* why = "";
  FastConst   k;
  const int   rc = fast_constants(p, &k, &why);
  copy_why(why, why_out, cap);
  return rc;
}
// fast_need_history
int fh_need_history(int hist_fast, char* why_out, int cap)
{
  const char* why = "";
  const int   rc  = fast_need_history(hist_fast != 0, &why);
  copy_why(why, why_out, cap);
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
  clamp_image(hf, hnf, hc, hn, w, h, k, out_colour, out_length, count, mu, sigma, lo, hi, moved);
  return PT_OK;
}

// pt_temporal_accumulate / pt_temporal_accumulate_moving with pt_temporal_fast on, on the host: ah_temporal's call (tests/cpp/albedo_host.cpp; albedo ==
// NULL: pt_temporal_demodulate off) with the fast parameters, the fast history that is read and the new one, which this form requires.
int fh_step(const HistoryCall* q) { return q ? history_step(*q, q->fast && q->out_fast && q->out_fast_length) : PT_ERR_INVALID; }
}
