// What the host builds of the stage headers (denoise_host.cpp, temporal_host.cpp, svgf_host.cpp, motion_host.cpp, albedo_host.cpp, fast_host.cpp) share
// besides those headers.  The one call of the history stage they share is stage/history_step.h.
#pragma once
#include <cstdint>
#include <cstring>
#include "pt_denoise.h"

// bit j: guide plane j was handed in
static inline uint32_t planes_of(const float* const g[PT_DENOISE_GUIDES])
{
  uint32_t m = 0;
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    m |= g && g[j] ? 1u << j : 0u;
  return m;
}

// the moments image of the history that is read, row-major, as svgf_moments reads it (M: SvM of pt_svgf.h)
template <class M>
struct RowMajorMoments {
  const M* hm;
  int      w;
  M        histMoments(int x, int y) const { return hm[size_t(y) * size_t(w) + size_t(x)]; }
};

// the static reason of a *_constants call or a refusal in why_out (why_len bytes, may be NULL)
static inline void copy_why(const char* why, char* why_out, int why_len)
{
  if(why_out && why_len > 0)
  {
    std::strncpy(why_out, why, size_t(why_len) - 1);
    why_out[why_len - 1] = 0;
  }
}
