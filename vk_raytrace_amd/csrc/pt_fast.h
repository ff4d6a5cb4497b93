// The responsive history (DESIGN.md section 5.7 is the definition): with pt_temporal_fast on, a second, short history (Hf, Hnf: the temporal step as it
// stands, run with maxFast in the place of maxHistory) is kept beside the long one, and the long history the step has just written is clamped, pixel by
// pixel, to the local mean +- sigmaScale standard deviations of the short one; where the clamp moved a channel the length is cut to maxFast.  Here: what
// pt_temporal_fast refuses, with the one text of each refusal, the constants of a call, and ONE pixel of the clamp as a template over where the values
// come from.  Plain inline functions of plain values, compiled by hipcc for the device (pt_fast.hip) and by g++ for the host (tests/cpp/fast_host.cpp),
// like pt_denoise.h: -ffp-contract=off, no fast math, IEEE /, * and sqrtf only.  No float is ever converted to an integer.  No reference counterpart.
#pragma once
#include <math.h>
#include "pt_denoise.h"  // DnPx, dn_finite, dn_finite3

#define PT_FAST_MAX_RADIUS 3

// the checked parameters of a call
struct FastConst {
  float maxFast, sigmaScale;
  int   radius;
};

// PT_OK, or why the parameters cannot be used (`why`: static text).  Fills k when it is not NULL and the parameters are accepted.
PT_DN int fast_constants(const pt_FastParams* p, FastConst* k, const char** why)
{
  if(!p)
    return *why = "null parameters", PT_ERR_INVALID;
  if(!(p->maxFast >= 1.0f) || !dn_finite(p->maxFast))
    return *why = "maxFast must be at least 1 and finite", PT_ERR_INVALID;
  if(!(p->sigmaScale >= 0.0f) || !dn_finite(p->sigmaScale))
    return *why = "sigmaScale must be non-negative and finite", PT_ERR_INVALID;
  if(p->radius < 1 || p->radius > PT_FAST_MAX_RADIUS)
    return *why = "radius must be 1, 2 or 3", PT_ERR_INVALID;
  if(p->flags != 0u)
    return *why = "unknown flag bits", PT_ERR_INVALID;
  if(k)
    *k = FastConst{p->maxFast, p->sigmaScale, p->radius};
  return PT_OK;
}
// pt_read_temporal_fast on a history that has no fast images
PT_DN int fast_need_history(bool histFast, const char** why)
{
  if(!histFast)
    return *why = "the history was made with pt_temporal_fast off", PT_ERR_STATE;
  return PT_OK;
}

// A tap as the clamp takes it: the fast colour's .rgb, and in .w whether the tap counts (1) or is skipped (0) -- its length is not at least 1, or a
// channel is not finite.  The kernel stages exactly this per pixel (16 bytes); the host reader forms it on the fly.
PT_DN DnPx fast_tap(const DnPx& f, float nf)
{
  const bool counts = nf >= 1.0f && dn_finite3(f);  // (false for a NaN length)
  return DnPx{f.x, f.y, f.z, counts ? 1.0f : 0.0f};
}

struct FastOut {
  DnPx  colour;  // Hc'(p) after the clamp
  float length;  // Hn'(p) after the clamp
};
// what a test may look at besides the result (tests/cpp/fast_host.cpp); the device passes no probe
struct FastProbe {
  float n;                     // taps counted (0 where the pixel was left before the window was read)
  float mu[3], sigma[3], lo[3], hi[3];
  int   moved;                 // 1: a channel moved and the length was cut
};

PT_DN void fast_stats(float n, float s1, float s2, float k, float& mu, float& sigma, float& lo, float& hi)
{
  mu            = s1 / n;
  const float v = s2 / n - mu * mu;
  // max(v, 0) in the spelling a NaN passes through: where a tap's square overflows, s2 / n and mu mu are both +Inf, v is NaN and so are the bounds -- the
  // pixel is left untouched; v > 0 ? v : 0 would make sigma 0 of it and clamp the pixel to a mean of the order of 1e37
  sigma         = sqrtf(v < 0.0f ? 0.0f : v);
  lo            = mu - k * sigma;
  hi            = mu + k * sigma;
}
PT_DN float fast_clampf(float x, float lo, float hi)  // clampf of pt_math.h (GLSL clamp): min(max(x, lo), hi)
{
  const float a = x < lo ? lo : x;
  return hi < a ? hi : a;
}

// Pixel (px, py) of a w x h image whose long history holds colour c and length n there (Hc'(p), Hn'(p): the caller's own pixel, read and written by it
// alone).  src.tap(x, y) is fast_tap of the fast history that was just written (Hf', Hnf'), asked only for positions inside the image: every index is
// integer arithmetic and is tested against the image before use.  Taps in the order dy = -R .. R outer, dx = -R .. R inner; fp32 sums of unfused products.
template <class Src>
PT_DN FastOut fast_clamp_pixel(const Src& src, const FastConst& k, const DnPx& c, float n, int px, int py, int w, int h, FastProbe* probe)
{
  FastOut o{c, n};
  if(probe)
  {
    probe->n = 0.0f, probe->moved = 0;
    for(int j = 0; j < 3; ++j)
      probe->mu[j] = probe->sigma[j] = probe->lo[j] = probe->hi[j] = nanf("");
  }
  if(!(n >= 1.0f) || !dn_finite3(c))
    return o;
  float cnt = 0.0f, s1x = 0.0f, s1y = 0.0f, s1z = 0.0f, s2x = 0.0f, s2y = 0.0f, s2z = 0.0f;
  for(int dy = -k.radius; dy <= k.radius; ++dy)
    for(int dx = -k.radius; dx <= k.radius; ++dx)
    {
      const int qx = px + dx, qy = py + dy;
      if(qx < 0 || qx >= w || qy < 0 || qy >= h)
        continue;
      const DnPx f = src.tap(qx, qy);
      if(!(f.w > 0.0f))
        continue;  // a tap that does not count is left out of n as well
      cnt = cnt + 1.0f;
      s1x = s1x + f.x, s1y = s1y + f.y, s1z = s1z + f.z;
      s2x = s2x + f.x * f.x, s2y = s2y + f.y * f.y, s2z = s2z + f.z * f.z;
    }
  if(probe)
    probe->n = cnt;
  if(cnt < 2.0f)
    return o;
  float mu[3], sg[3], lo[3], hi[3];
  fast_stats(cnt, s1x, s2x, k.sigmaScale, mu[0], sg[0], lo[0], hi[0]);
  fast_stats(cnt, s1y, s2y, k.sigmaScale, mu[1], sg[1], lo[1], hi[1]);
  fast_stats(cnt, s1z, s2z, k.sigmaScale, mu[2], sg[2], lo[2], hi[2]);
  if(probe)
    for(int j = 0; j < 3; ++j)
      probe->mu[j] = mu[j], probe->sigma[j] = sg[j], probe->lo[j] = lo[j], probe->hi[j] = hi[j];
  if(!(dn_finite(lo[0]) && dn_finite(hi[0]) && dn_finite(lo[1]) && dn_finite(hi[1]) && dn_finite(lo[2]) && dn_finite(hi[2])))
    return o;
  o.colour.x = fast_clampf(c.x, lo[0], hi[0]);
  o.colour.y = fast_clampf(c.y, lo[1], hi[1]);
  o.colour.z = fast_clampf(c.z, lo[2], hi[2]);
  if(o.colour.x != c.x || o.colour.y != c.y || o.colour.z != c.z)
  {
    o.length = k.maxFast < n ? k.maxFast : n;  // GLSL min(Hn', maxFast)
    if(probe)
      probe->moved = 1;
  }
  return o;
}

// Src over row-major planes in ordinary memory (the host build; the device stages fast_tap of its tile in LDS)
struct FcRowMajor {
  const DnPx*  hf;
  const float* hnf;
  int          w;
  PT_DN_MEMBER DnPx tap(int x, int y) const
  {
    const size_t at = size_t(y) * size_t(w) + size_t(x);
    return fast_tap(hf[at], hnf[at]);
  }
};
