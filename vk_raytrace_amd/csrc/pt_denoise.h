// The edge-avoiding a-trous denoiser of the display path (Dammertz et al. 2010; DESIGN.md "Denoiser"): ONE output pixel of ONE iteration, the
// demodulation by the albedo guide, and what the host derives from pt_DenoiseParams.  Plain inline functions of plain values, compiled by hipcc for
// the device (pt_denoise.hip) and by g++ for the host (tests/cpp/denoise_host.cpp), like pt_query.h and pt_shade.h: -ffp-contract=off, no fast math,
// pt_exp of include/pt_fpmath.h and no other transcendental, so that the device is held bit for bit to the host build and the host build to a float64
// model of the definition.  No reference counterpart: the reference shows its accumulation image unfiltered.
//
// Where the values of a pixel come from is the caller's business (`Src`: row-major memory on the host, global memory or an LDS tile on the device);
// the arithmetic is stated here once.
#pragma once
#include <stdint.h>
#include "../../include/pt_api.h"
#include "../../include/pt_fpmath.h"

#if defined(__HIPCC__)
#define PT_DN __host__ __device__ __forceinline__
#define PT_DN_MEMBER __host__ __device__
#else
#define PT_DN static inline
#define PT_DN_MEMBER
#endif

#define PT_DENOISE_ALBEDO_FLOOR 0.001f
#define PT_DENOISE_MAX_ITERATIONS 8
#define PT_DENOISE_COLOUR_TERM 1u  // DenoiseConst::terms bit 0: the colour term; bit 1 + j: guide plane j

struct DnPx {
  float x, y, z, w;
};

// fp32 constants of one call, computed on the host: inv_c(i) = 1 / (s_i * s_i) with s_i = sigmaColor * 2^-i (the scaling is exact),
// inv_j = 1 / (sigmaGuide[j] * sigmaGuide[j])
struct DenoiseConst {
  float    invC[PT_DENOISE_MAX_ITERATIONS];
  float    invG[PT_DENOISE_GUIDES];
  uint32_t terms;
};

PT_DN bool dn_finite(float x) { return ptf_abs(x) <= 3.402823466e38f; }  // false for NaN and +-Inf
PT_DN bool dn_finite3(const DnPx& c) { return dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z); }

// PT_OK, or why the parameters cannot be used (`why`: static text).  planesSet: bit j = guide plane j is installed.  Beyond what pt_api.h lists, a sigma
// whose 1 / sigma^2 is not finite in fp32 at some iteration is refused: every weight would be NaN.
PT_DN int denoise_constants(const pt_DenoiseParams* p, uint32_t planesSet, DenoiseConst* k, const char** why)
{
  if(!p)
    return *why = "null parameters", PT_ERR_INVALID;
  if(p->iterations < 1 || p->iterations > PT_DENOISE_MAX_ITERATIONS)
    return *why = "iterations must be 1 .. 8", PT_ERR_INVALID;
  if(p->flags & ~PT_DENOISE_DEMODULATE)
    return *why = "unknown flag bits", PT_ERR_INVALID;
  if(!(p->sigmaColor >= 0.0f))
    return *why = "sigmaColor is negative or NaN", PT_ERR_INVALID;
  k->terms = 0u;
  for(int i = 0; i < PT_DENOISE_MAX_ITERATIONS; ++i)
  {
    const float s = p->sigmaColor * ptf_pow2i(-i);
    k->invC[i]    = p->sigmaColor > 0.0f ? 1.0f / (s * s) : 0.0f;
    if(i < p->iterations && !dn_finite(k->invC[i]))
      return *why = "sigmaColor is too small: 1 / sigma^2 overflows", PT_ERR_INVALID;
  }
  if(p->sigmaColor > 0.0f)
    k->terms |= PT_DENOISE_COLOUR_TERM;
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
  {
    k->invG[j] = 0.0f;
    if(!(planesSet >> j & 1u))
      continue;
    const float s = p->sigmaGuide[j];
    if(!(s > 0.0f) || !dn_finite(s))
      return *why = "sigmaGuide of an installed plane must be positive and finite", PT_ERR_INVALID;
    k->invG[j] = 1.0f / (s * s);
    if(!dn_finite(k->invG[j]))
      return *why = "sigmaGuide is too small: 1 / sigma^2 overflows", PT_ERR_INVALID;
    k->terms |= 2u << j;
  }
  if((p->flags & PT_DENOISE_DEMODULATE) && !(planesSet & 1u))
    return *why = "PT_DENOISE_DEMODULATE needs guide plane 0 (the albedo)", PT_ERR_STATE;
  return PT_OK;
}

// Demodulation: c.rgb / max(albedo.rgb, floor) before iteration 0, c.rgb * max(albedo.rgb, floor) after the last one, per channel.  A channel that is not
// finite passes through: that IS the quotient / product (Inf / a = Inf, NaN / a = NaN for the finite a >= floor), stated so that a NaN's payload does not
// depend on which operand the hardware propagates.
PT_DN float dn_albedo(float g) { return g > PT_DENOISE_ALBEDO_FLOOR ? g : PT_DENOISE_ALBEDO_FLOOR; }
PT_DN DnPx  denoise_demodulate(const DnPx& c, const DnPx& g)
{
  DnPx r = c;
  r.x    = dn_finite(c.x) ? c.x / dn_albedo(g.x) : c.x;
  r.y    = dn_finite(c.y) ? c.y / dn_albedo(g.y) : c.y;
  r.z    = dn_finite(c.z) ? c.z / dn_albedo(g.z) : c.z;
  return r;
}
PT_DN DnPx denoise_remodulate(const DnPx& c, const DnPx& g)
{
  DnPx r = c;
  r.x    = dn_finite(c.x) ? c.x * dn_albedo(g.x) : c.x;
  r.y    = dn_finite(c.y) ? c.y * dn_albedo(g.y) : c.y;
  r.z    = dn_finite(c.z) ? c.z * dn_albedo(g.z) : c.z;
  return r;
}

// |a.xyz - b.xyz|^2, summed x, y, z
PT_DN float dn_dist2(const DnPx& a, const DnPx& b)
{
  const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return (dx * dx + dy * dy) + dz * dz;
}
// the B3-spline kernel {1/16, 1/4, 3/8, 1/4, 1/16}; the products of two of its entries are exact
PT_DN float dn_h(int i) { return i == 2 ? 0.375f : (i == 1 || i == 3) ? 0.25f : 0.0625f; }

// Pixel (x, y) of iteration `iteration` (step 2^iteration) over a W x H image.  src.colour(qx, qy) is the iteration's input, src.guide(j, qx, qy) plane
// j; both are only asked for pixels inside the image, and guide j only when its term is on.  Taps run dy = -2 .. 2 (outer), dx = -2 .. 2 (inner); a tap
// outside the image or whose colour is not finite takes no part in either sum.  The exponent adds the terms that are on in the order colour, guide 0, 1,
// 2 (a term that is off is left out, not added as 0); the colour term is also off for a centre that is not finite.  Both sums are fp32 additions in tap
// order of unfused products; an empty sum of weights returns the centre unchanged.  Alpha is the centre's.
template <class Src>
PT_DN DnPx denoise_pixel(const Src& src, int x, int y, int w, int h, int iteration, const DenoiseConst& k)
{
  const int   step    = 1 << iteration;
  const DnPx  cp      = src.colour(x, y);
  const bool  colour  = (k.terms & PT_DENOISE_COLOUR_TERM) != 0u && dn_finite3(cp);
  const float invC    = k.invC[iteration];
  DnPx        gp[PT_DENOISE_GUIDES];
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    if(k.terms & (2u << j))
      gp[j] = src.guide(j, x, y);
    else
      gp[j] = DnPx{0.0f, 0.0f, 0.0f, 0.0f};
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
  for(int dy = -2; dy <= 2; ++dy)
  {
    const int qy = y + step * dy;
    if(qy < 0 || qy >= h)
      continue;
    for(int dx = -2; dx <= 2; ++dx)
    {
      const int qx = x + step * dx;
      if(qx < 0 || qx >= w)
        continue;
      const DnPx cq = src.colour(qx, qy);
      if(!dn_finite3(cq))
        continue;
      float e   = 0.0f;
      bool  any = false;
      if(colour)
      {
        e   = dn_dist2(cp, cq) * invC;
        any = true;
      }
      for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
        if(k.terms & (2u << j))
        {
          const float t = dn_dist2(gp[j], src.guide(j, qx, qy)) * k.invG[j];
          e             = any ? e + t : t;
          any           = true;
        }
      const float kk = dn_h(dx + 2) * dn_h(dy + 2);
      const float wt = any ? kk * pt_exp(-e) : kk;
      sr             = sr + wt * cq.x;
      sg             = sg + wt * cq.y;
      sb             = sb + wt * cq.z;
      sw             = sw + wt;
    }
  }
  DnPx out = cp;
  if(sw != 0.0f)
  {
    out.x = sr / sw;
    out.y = sg / sw;
    out.z = sb / sw;
  }
  return out;
}

// Src over row-major RGBA32F planes in ordinary memory (the host build; the device has its own readers with 16-byte loads)
struct DnRowMajor {
  const DnPx* c;
  const DnPx* g[PT_DENOISE_GUIDES];
  int         w;
  PT_DN_MEMBER DnPx colour(int x, int y) const { return c[size_t(y) * size_t(w) + size_t(x)]; }
  PT_DN_MEMBER DnPx guide(int j, int x, int y) const { return g[j][size_t(y) * size_t(w) + size_t(x)]; }
};
