// The host build of the variance-guided filter: vk_raytrace_amd/csrc/pt_svgf.h compiled by g++, whole calls over row-major images in ordinary memory.
// tests/svgf_host.py compiles and binds it; tests/test_svgf_model.py holds it to a float64 model, tests/test_svgf_gpu.py holds the device to it.
#include "stage/history_step.h"

namespace {
SvRowMajor source(const float* colour, const float* const g[PT_DENOISE_GUIDES], const float* variance, const float* length, const float* moments, int w)
{
  SvRowMajor s{};
  s.c = (const DnPx*)colour;
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    s.g[j] = g ? (const DnPx*)g[j] : nullptr;
  s.v  = variance;
  s.hn = length;
  s.hm = (const SvM*)moments;
  s.w  = w;
  return s;
}
}  // namespace

extern "C" {

// pt_temporal_accumulate with tracking on, on the host: th_temporal's call (tests/cpp/temporal_host.cpp) with the moments image of the history that is
// read (w * h * 2 floats; not read for a first call) and the new one, which this form requires.
int sh_temporal_m(const HistoryCall* q) { return q ? history_step(*q, q->out_moments != nullptr) : PT_ERR_INVALID; }

// pt_svgf_variance on the host: V0 from the history's colour, length and moments and the guide planes (guides[j] NULL: plane j not installed)
int sh_variance(const float* hist_colour, const float* hist_length, const float* hist_moments, const float* const guides[PT_DENOISE_GUIDES], int w, int h,
                const pt_SvgfParams* params, float* out_variance)
{
  SvgfConst   k;
  const char* why = "";
  const int   rc  = svgf_constants(params, planes_of(guides), &k, &why);
  if(rc != PT_OK)
    return rc;
  if(!hist_colour || !hist_length || !hist_moments || !out_variance || w <= 0 || h <= 0)
    return PT_ERR_INVALID;
  const SvRowMajor src = source(hist_colour, guides, nullptr, hist_length, hist_moments, w);
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
      out_variance[size_t(y) * size_t(w) + size_t(x)] = svgf_variance_pixel(src, x, y, w, h, k);
  return PT_OK;
}

// ONE iteration of the filter on the host, colour and variance given directly (a test may hand in any variance plane)
int sh_iteration(const float* colour, const float* variance, const float* const guides[PT_DENOISE_GUIDES], int w, int h, const pt_SvgfParams* params,
                 int iteration, float* out_colour, float* out_variance)
{
  SvgfConst   k;
  const char* why = "";
  const int   rc  = svgf_constants(params, planes_of(guides), &k, &why);
  if(rc != PT_OK)
    return rc;
  if(!colour || !variance || !out_colour || !out_variance || w <= 0 || h <= 0 || iteration < 0 || iteration >= PT_SVGF_MAX_ITERATIONS)
    return PT_ERR_INVALID;
  const SvRowMajor src = source(colour, guides, variance, nullptr, nullptr, w);
#pragma omp parallel for schedule(static)
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      const SvOut  o  = svgf_pixel(src, x, y, w, h, iteration, k);
      const size_t at = size_t(y) * size_t(w) + size_t(x);
      std::memcpy(out_colour + 4 * at, &o.colour, sizeof(DnPx));
      out_variance[at] = o.variance;
    }
  return PT_OK;
}

// svgf_constants: the status, and the static reason in why_out (why_len bytes, may be NULL).  planes: bit j = guide plane j is installed
int sh_constants(const pt_SvgfParams* params, unsigned planes, char* why_out, int why_len)
{
  SvgfConst   k;
  const char* why = "";
  const int   rc  = svgf_constants(params, planes, &k, &why);
  copy_why(why, why_out, why_len);
  return rc;
}
}
