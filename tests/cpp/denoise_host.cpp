// The host build of the denoiser: vk_raytrace_amd/csrc/pt_denoise.h compiled by g++, the whole filter over row-major images in ordinary memory.
// tests/denoise_host.py compiles and binds it; tests/test_denoise_model.py holds it to a float64 model, tests/test_denoise_gpu.py holds the device to it.
#include <cstring>
#include <vector>
#include "stage/stage_host_common.h"

extern "C" {

// pt_denoise on the host.  colour, guides[j] (NULL: plane j unset), out: w * h * 4 floats; per_iteration_out (may be NULL): iterations * w * h * 4
// floats, the output of every iteration (demodulated when PT_DENOISE_DEMODULATE is set: the remodulation is applied to `out` only).
// Returns what denoise_constants returns (PT_OK, PT_ERR_INVALID, PT_ERR_STATE); nothing is written on an error.
int dh_denoise(const float* colour, const float* const guides[PT_DENOISE_GUIDES], int w, int h, const pt_DenoiseParams* params, float* out, float* per_iteration_out)
{
  DenoiseConst k;
  const char*  why = "";
  const int    rc  = denoise_constants(params, planes_of(guides), &k, &why);
  if(rc != PT_OK)
    return rc;
  if(!colour || !out || w <= 0 || h <= 0)
    return PT_ERR_INVALID;
  const size_t      n = size_t(w) * size_t(h);
  std::vector<DnPx> a(n), b(n);
  std::memcpy(a.data(), colour, n * sizeof(DnPx));
  const DnPx* g[PT_DENOISE_GUIDES];
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    g[j] = guides ? reinterpret_cast<const DnPx*>(guides[j]) : nullptr;
  const bool demod = (params->flags & PT_DENOISE_DEMODULATE) != 0u;
  if(demod)
    for(size_t i = 0; i < n; ++i)
      a[i] = denoise_demodulate(a[i], g[0][i]);
  for(int it = 0; it < params->iterations; ++it)
  {
    const DnRowMajor src{a.data(), {g[0], g[1], g[2]}, w};
#pragma omp parallel for schedule(static)
    for(int y = 0; y < h; ++y)
      for(int x = 0; x < w; ++x)
        b[size_t(y) * size_t(w) + size_t(x)] = denoise_pixel(src, x, y, w, h, it, k);
    a.swap(b);
    if(per_iteration_out)
      std::memcpy(per_iteration_out + size_t(it) * n * 4, a.data(), n * sizeof(DnPx));
  }
  if(demod)
    for(size_t i = 0; i < n; ++i)
      a[i] = denoise_remodulate(a[i], g[0][i]);
  std::memcpy(out, a.data(), n * sizeof(DnPx));
  return PT_OK;
}

// the fp32 constants of a call as the filter uses them: inv_c[8], inv_g[3], terms (denoise_constants)
int dh_constants(const pt_DenoiseParams* params, uint32_t planes_set, float* inv_c, float* inv_g, uint32_t* terms)
{
  DenoiseConst k;
  const char*  why = "";
  const int    rc  = denoise_constants(params, planes_set, &k, &why);
  if(rc != PT_OK)
    return rc;
  std::memcpy(inv_c, k.invC, sizeof(k.invC));
  std::memcpy(inv_g, k.invG, sizeof(k.invG));
  *terms = k.terms;
  return PT_OK;
}
}
