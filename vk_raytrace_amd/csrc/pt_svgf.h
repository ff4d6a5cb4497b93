// The variance-guided filter of the history (the spatial half of SVGF, Schied et al. 2017; DESIGN.md section 5.4 is the definition): the luminance
// moments ONE pixel of pt_temporal_accumulate adds to the history, ONE pixel of the initial variance, ONE output pixel of ONE filter iteration, and
// what the host derives from pt_SvgfParams.  Plain inline functions of plain values, compiled by hipcc for the device (pt_svgf.hip) and by g++ for the
// host (tests/cpp/svgf_host.cpp), like pt_denoise.h and pt_temporal.h: -ffp-contract=off, no fast math, pt_exp of include/pt_fpmath.h, IEEE / and
// sqrtf and no other transcendental, so that the device is held bit for bit to the host build and the host build to a float64 model of the definition.
// No reference counterpart.
//
// Where the values of a pixel come from is the caller's business (`Src`: row-major memory on the host, global memory or an LDS tile on the device).
// No function here converts a float to an int: every index is integer arithmetic on the pixel position (or a tap position temporal_pixel formed and
// tested), and is tested against the image before it is used.
#pragma once
#include "pt_temporal.h"  // TemporalProbe, TemporalOut, tp_mix; through it pt_denoise.h: DnPx, dn_finite, dn_finite3, dn_dist2, dn_h

#define PT_SVGF_MAX_ITERATIONS 8
#define PT_SVGF_FLT_MAX 3.402823466e38f

struct SvM {
  float x, y;  // first and second moment of the luminance
};
struct SvOut {
  DnPx  colour;
  float variance;
};
// fp32 constants of one call: inv_j = 1 / (sigmaGuide[j] * sigmaGuide[j]); terms bit 1 + j: guide plane j (the bit numbering of DenoiseConst)
struct SvgfConst {
  float    sigmaLum, lumFloor, minTemporal;
  float    invG[PT_DENOISE_GUIDES];
  uint32_t terms;
};

PT_DN float sv_lum(const DnPx& c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
PT_DN bool  sv_usable(const DnPx& c) { return dn_finite3(c) && dn_finite(sv_lum(c)); }
// every READ of a variance goes through this; NaN, a negative value and -0 give +0, +Inf gives FLT_MAX.  Stores are raw.
PT_DN float sv_san(float v) { return v > 0.0f ? (v <= PT_SVGF_FLT_MAX ? v : PT_SVGF_FLT_MAX) : 0.0f; }

// PT_OK, or why the parameters cannot be used (`why`: static text).  planesSet: bit j = guide plane j is installed.
PT_DN int svgf_constants(const pt_SvgfParams* p, uint32_t planesSet, SvgfConst* k, const char** why)
{
  if(!p)
    return *why = "null parameters", PT_ERR_INVALID;
  if(p->iterations < 1 || p->iterations > PT_SVGF_MAX_ITERATIONS)
    return *why = "iterations must be 1 .. 8", PT_ERR_INVALID;
  if(p->flags != 0u)
    return *why = "unknown flag bits", PT_ERR_INVALID;
  if(!(p->sigmaLum > 0.0f) || !dn_finite(p->sigmaLum))
    return *why = "sigmaLum must be positive and finite", PT_ERR_INVALID;
  if(!(p->lumFloor > 0.0f) || !dn_finite(p->lumFloor))
    return *why = "lumFloor must be positive and finite", PT_ERR_INVALID;
  if(!(p->minTemporal >= 1.0f) || !dn_finite(p->minTemporal))
    return *why = "minTemporal must be at least 1 and finite", PT_ERR_INVALID;
  k->sigmaLum    = p->sigmaLum;
  k->lumFloor    = p->lumFloor;
  k->minTemporal = p->minTemporal;
  k->terms       = 0u;
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
  return PT_OK;
}

// ---- 1. moments in the history -------------------------------------------------------------------------------------------------------------------------
// Hm' of the pixel whose colour step temporal_pixel just took: `pr` and `o` are what it filled (tap positions, verdicts, fx, fy, sw, outcome; the new
// length), `c` the current pixel's colour.  The gather runs over exactly the counted taps, in tap order, with the weights of the colour step, formed
// again from fx and fy by the same expressions; src.histMoments is asked only for counted taps, which lie inside the image.
template <class Src>
PT_DN SvM svgf_moments(const Src& src, const TemporalProbe& pr, const TemporalOut& o, const DnPx& c)
{
  const float Lc = sv_lum(c);
  SvM         h{0.0f, 0.0f};
  if(pr.outcome == PT_TEMPORAL_BLEND || pr.outcome == PT_TEMPORAL_HISTORY_ONLY)
  {
    const float x0f = floorf(pr.fx), y0f = floorf(pr.fy);
    const float wx = pr.fx - x0f, wy = pr.fy - y0f;
    const float wgt[4] = {(1.0f - wx) * (1.0f - wy), wx * (1.0f - wy), (1.0f - wx) * wy, wx * wy};
    float       s1 = 0.0f, s2 = 0.0f;
    for(int i = 0; i < 4; ++i)
      if(pr.verdict[i] == 1)
      {
        const SvM m = src.histMoments(pr.tapX[i], pr.tapY[i]);
        s1          = s1 + wgt[i] * m.x;
        s2          = s2 + wgt[i] * m.y;
      }
    h.x = s1 / pr.sw;
    h.y = s2 / pr.sw;
  }
  if(pr.outcome == PT_TEMPORAL_BLEND)
  {
    const float a = 1.0f / o.length;  // the colour blend's a = 1 / Hn'
    return SvM{tp_mix(h.x, Lc, a), tp_mix(h.y, Lc * Lc, a)};
  }
  if(pr.outcome == PT_TEMPORAL_HISTORY_ONLY)
    return h;
  if(pr.outcome == PT_TEMPORAL_CURRENT)
    return SvM{Lc, Lc * Lc};
  return SvM{0.0f, 0.0f};
}

// ---- 3. initial variance -------------------------------------------------------------------------------------------------------------------------------
// V0 of pixel (x, y).  src.length / src.moments / src.colour are the history set that holds the history, src.guide(j, ...) the current guide planes
// (asked only when the term is on); all only for positions inside the image.
template <class Src>
PT_DN float svgf_variance_pixel(const Src& src, int x, int y, int w, int h, const SvgfConst& k)
{
  const float n = src.length(x, y);
  float       v = 0.0f;
  if(n >= k.minTemporal)
  {
    const SvM m = src.moments(x, y);
    v           = m.y - m.x * m.x;
  }
  else
  {
    DnPx gp[PT_DENOISE_GUIDES];
    for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
      if(k.terms & (2u << j))
        gp[j] = src.guide(j, x, y);
      else
        gp[j] = DnPx{0.0f, 0.0f, 0.0f, 0.0f};
    float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
    for(int dy = -3; dy <= 3; ++dy)
    {
      const int qy = y + dy;
      if(qy < 0 || qy >= h)
        continue;
      for(int dx = -3; dx <= 3; ++dx)
      {
        const int qx = x + dx;
        if(qx < 0 || qx >= w)
          continue;
        if(!(src.length(qx, qy) >= 1.0f) || !dn_finite3(src.colour(qx, qy)))
          continue;
        float e   = 0.0f;
        bool  any = false;
        for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
          if(k.terms & (2u << j))
          {
            const float t = dn_dist2(gp[j], src.guide(j, qx, qy)) * k.invG[j];
            e             = any ? e + t : t;
            any           = true;
          }
        const float wt = any ? pt_exp(-e) : 1.0f;
        const SvM   m  = src.moments(qx, qy);
        s1             = s1 + wt * m.x;
        s2             = s2 + wt * m.y;
        sw             = sw + wt;
      }
    }
    if(sw > 0.0f)
    {
      const float m1 = s1 / sw;
      v              = (s2 / sw - m1 * m1) * (k.minTemporal / (n >= 1.0f ? n : 1.0f));
    }
  }
  return sv_san(v);
}

// ---- 4. one filter iteration ---------------------------------------------------------------------------------------------------------------------------
// Pixel (x, y) of iteration `iteration` (step 2^iteration) over a W x H image.  src.colour / src.variance are the iteration's input, src.guide(j, ...)
// plane j; all only asked for pixels inside the image, and guide j only when its term is on.  The variance prefilter is 3 x 3 at step 1 whatever the
// iteration.  Taps run dy = -2 .. 2 (outer), dx = -2 .. 2 (inner); sums are fp32 additions in tap order of unfused products.
template <class Src>
PT_DN SvOut svgf_pixel(const Src& src, int x, int y, int w, int h, int iteration, const SvgfConst& k)
{
  const int   step  = 1 << iteration;
  const DnPx  cp    = src.colour(x, y);
  const bool  lumOn = sv_usable(cp);
  const float Lp    = sv_lum(cp);
  float       sv = 0.0f, sgs = 0.0f;
  for(int dy = -1; dy <= 1; ++dy)
  {
    const int vy = y + dy;
    if(vy < 0 || vy >= h)
      continue;
    for(int dx = -1; dx <= 1; ++dx)
    {
      const int vx = x + dx;
      if(vx < 0 || vx >= w)
        continue;
      const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
      sv            = sv + g * sv_san(src.variance(vx, vy));
      sgs           = sgs + g;
    }
  }
  const float vbar = sv / sgs;
  const float den  = k.sigmaLum * sqrtf(vbar) + k.lumFloor;  // positive; may be +Inf, never NaN
  DnPx        gp[PT_DENOISE_GUIDES];
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    if(k.terms & (2u << j))
      gp[j] = src.guide(j, x, y);
    else
      gp[j] = DnPx{0.0f, 0.0f, 0.0f, 0.0f};
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sq = 0.0f;
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
      if(!sv_usable(cq))
        continue;
      float e   = 0.0f;
      bool  any = false;
      if(lumOn)
      {
        e   = ptf_abs(Lp - sv_lum(cq)) / den;
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
      sq             = sq + (wt * wt) * sv_san(src.variance(qx, qy));
    }
  }
  SvOut out{cp, 0.0f};
  if(sw != 0.0f)
  {
    out.colour.x = sr / sw;
    out.colour.y = sg / sw;
    out.colour.z = sb / sw;
    out.variance = sq / (sw * sw);
  }
  else
    out.variance = sv_san(src.variance(x, y));
  return out;
}

// Src over row-major planes in ordinary memory (the host build; the device has its own readers)
struct SvRowMajor {
  const DnPx*  c;
  const DnPx*  g[PT_DENOISE_GUIDES];
  const float* v;   // variance (svgf_pixel)
  const float* hn;  // history length (svgf_variance_pixel)
  const SvM*   hm;  // history moments (svgf_variance_pixel, svgf_moments)
  int          w;
  PT_DN_MEMBER size_t at(int x, int y) const { return size_t(y) * size_t(w) + size_t(x); }
  PT_DN_MEMBER DnPx   colour(int x, int y) const { return c[at(x, y)]; }
  PT_DN_MEMBER DnPx   guide(int j, int x, int y) const { return g[j][at(x, y)]; }
  PT_DN_MEMBER float  variance(int x, int y) const { return v[at(x, y)]; }
  PT_DN_MEMBER float  length(int x, int y) const { return hn[at(x, y)]; }
  PT_DN_MEMBER SvM    moments(int x, int y) const { return hm[at(x, y)]; }
  PT_DN_MEMBER SvM    histMoments(int x, int y) const { return hm[at(x, y)]; }
};
