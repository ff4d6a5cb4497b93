// The demodulated history (DESIGN.md section 5.6 is the definition): with pt_temporal_demodulate on, the temporal step reads the pixel's own colour
// divided by the albedo (guide plane 0), so that the history, its moments and every variance downstream are of illumination, and the consumers of the
// history multiply their final image by the albedo again.  Here: the reader adaptor that does the division in front of temporal_pixel /
// temporal_pixel_moving / svgf_moments (pt_temporal.h, pt_motion.h, pt_svgf.h: called through it as they stand), ONE pixel of the remodulation, and what
// the entry points refuse, with the one text of each refusal.  Plain inline functions of plain values, compiled by hipcc for the device (pt_albedo.hip)
// and by g++ for the host (tests/cpp/albedo_host.cpp), like pt_denoise.h: -ffp-contract=off, no fast math, IEEE / and * only.  No reference counterpart.
#pragma once
#include "pt_denoise.h"  // DnPx, denoise_demodulate, denoise_remodulate, PT_DENOISE_ALBEDO_FLOOR

// A reader over any `Src` the temporal step takes, which has albedo(x, y) besides (guide plane 0 at the pixel itself).  colour(x, y) is the demodulated
// colour: per channel c / max(g, floor), a channel that is not finite passes through, alpha untouched.  Everything else forwards: the history's taps are
// already demodulated and are read as they are.  histMoments / instance exist where Src has them (templates: instantiated only where called).
template <class Src>
struct AlbedoDemod {
  const Src& src;
  PT_DN_MEMBER DnPx colour(int x, int y) const { return denoise_demodulate(src.colour(x, y), src.albedo(x, y)); }
  PT_DN_MEMBER DnPx normal(int x, int y) const { return src.normal(x, y); }
  PT_DN_MEMBER DnPx depth(int x, int y) const { return src.depth(x, y); }
  PT_DN_MEMBER DnPx histColour(int x, int y) const { return src.histColour(x, y); }
  PT_DN_MEMBER DnPx histGuide(int x, int y) const { return src.histGuide(x, y); }
  PT_DN_MEMBER float histLength(int x, int y) const { return src.histLength(x, y); }
  template <class S = Src>
  PT_DN_MEMBER auto histMoments(int x, int y) const -> decltype(static_cast<const S&>(src).histMoments(x, y))
  {
    return src.histMoments(x, y);
  }
  template <class S = Src>
  PT_DN_MEMBER auto instance(int x, int y) const -> decltype(static_cast<const S&>(src).instance(x, y))
  {
    return src.instance(x, y);
  }
};

// The remodulation of one pixel: x(p) * max(g_0(p), floor) per channel, a channel that is not finite passes through, alpha untouched.  `x` is the final
// image of a consumer at p, `g` guide plane 0 at the same p (never at a history position: the albedo is the current frame's).
PT_DN DnPx albedo_remodulate(const DnPx& x, const DnPx& g) { return denoise_remodulate(x, g); }

// ---- what the entry points refuse (PT_OK, or the code with `why`: static text) ------------------------------------------------------------------------
// pt_temporal_demodulate(ctx, on)
PT_DN int albedo_setting(int on, const char** why)
{
  if(on != 0 && on != 1)
    return *why = "on must be 0 or 1", PT_ERR_INVALID;
  return PT_OK;
}
// the temporal step while the setting is on.  planesSet: bit j = guide plane j is installed
PT_DN int albedo_step_needs_plane(bool setting, uint32_t planesSet, const char** why)
{
  if(setting && !(planesSet & 1u))
    return *why = "pt_temporal_demodulate is on: guide plane 0 (the albedo) must be installed to divide by", PT_ERR_STATE;
  return PT_OK;
}
// a consumer of a history that is demodulated
PT_DN int albedo_need_plane(bool demodulated, uint32_t planesSet, const char** why)
{
  if(demodulated && !(planesSet & 1u))
    return *why = "the history is demodulated (pt_temporal_demodulate): guide plane 0 (the albedo) must be installed to multiply by", PT_ERR_STATE;
  return PT_OK;
}
// pt_denoise_history: flags of its pt_DenoiseParams on a demodulated history
PT_DN int albedo_denoise_flags(bool demodulated, uint32_t flags, const char** why)
{
  if(demodulated && (flags & PT_DENOISE_DEMODULATE))
    return *why = "PT_DENOISE_DEMODULATE on a history that is already demodulated (pt_temporal_demodulate)", PT_ERR_STATE;
  return PT_OK;
}

// Src over row-major planes in ordinary memory, with the albedo plane (the host build).  Base: TpRowMajor (pt_temporal.h) or MoRowMajor (pt_motion.h).
template <class Base>
struct AlRowMajor : Base {
  const DnPx* g0;
  PT_DN_MEMBER DnPx albedo(int x, int y) const { return g0[size_t(y) * size_t(this->w) + size_t(x)]; }
};
