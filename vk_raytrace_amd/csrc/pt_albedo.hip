// The kernels of the demodulated history: the temporal step that divides the pixel's own colour by the albedo as it reads it, in
// its four forms (with and without the moments image, static and moving), and the remodulation of a consumer's final image.  The per-pixel bodies are
// pt_temporal.h, pt_motion.h and pt_svgf.h as they stand, called through the reader adaptor of pt_albedo.h; this unit holds the kernels and their
// launches.  The entry points stay where the stages have them (pt_temporal.hip, pt_svgf.hip, pt_denoise.hip).  No existing kernel is involved and none is
// compiled from other text than before.
#include "pt_stage.h"
#include "pt_albedo.h"
#include "pt_motion.h"
#include "pt_svgf.h"

// ---- the demodulating temporal step -------------------------------------------------------------------------------------------------------------------------
// k_temporal's 32 x 8 tile (pt_temporal.hip), one pixel per lane: a wave covers two rows of 32 pixels.  One 16-byte load more per pixel than the kernel
// it stands in for -- the albedo, adjacent lanes reading adjacent pixels like the colour load next to it -- and three divisions.
#define AD_TX 32
#define AD_TY 8

struct AdArgs {
  TemporalMArgs    m;  // m.hm / m.hmOut are read by the kernels with the moments image only
  TemporalConst    k;
  const float4*    g0;     // guide plane 0, the albedo
  const uint32_t*  ids;    // MOVING only
  const MotionRec* table;  // MOVING only
  uint32_t         numInstances;
};
struct AdGlobal {
  const AdArgs& a;
  __device__ size_t   at(int x, int y) const { return size_t(y) * size_t(a.m.w) + size_t(x); }
  __device__ DnPx     colour(int x, int y) const { return stage_px(a.m.c[at(x, y)]); }
  __device__ DnPx     albedo(int x, int y) const { return stage_px(a.g0[at(x, y)]); }
  __device__ DnPx     normal(int x, int y) const { return stage_px(a.m.g1[at(x, y)]); }
  __device__ DnPx     depth(int x, int y) const { return stage_px(a.m.g2[at(x, y)]); }
  __device__ DnPx     histColour(int x, int y) const { return stage_px(a.m.hc[at(x, y)]); }
  __device__ DnPx     histGuide(int x, int y) const { return stage_px(a.m.hg[at(x, y)]); }
  __device__ float    histLength(int x, int y) const { return a.m.hn[at(x, y)]; }
  __device__ uint32_t instance(int x, int y) const { return a.ids[at(x, y)]; }
  __device__ SvM      histMoments(int x, int y) const
  {
    const float2 v = a.m.hm[at(x, y)];
    return SvM{v.x, v.y};
  }
};

template <bool MOMENTS, bool MOVING>
__global__ void __launch_bounds__(AD_TX * AD_TY) k_temporal_d(AdArgs a)
{
  const int x = int(blockIdx.x) * AD_TX + int(threadIdx.x), y = int(blockIdx.y) * AD_TY + int(threadIdx.y);
  if(x >= a.m.w || y >= a.m.h)
    return;
  const AdGlobal              mem{a};
  const AlbedoDemod<AdGlobal> src{mem};
  const size_t                at = size_t(y) * size_t(a.m.w) + size_t(x);
  TemporalProbe               pr;
  TemporalProbe* const        probe = MOMENTS ? &pr : nullptr;
  TemporalOut                 o;
  if constexpr(MOVING)
    o = temporal_pixel_moving(src, a.k, a.table, a.numInstances, x, y, a.m.w, a.m.h, probe);
  else
    o = temporal_pixel(src, a.k, x, y, a.m.w, a.m.h, probe);
  if constexpr(MOMENTS)
  {
    const SvM m   = svgf_moments(src, pr, o, src.colour(x, y));  // the moments are of the demodulated luminance
    a.m.hmOut[at] = make_float2(m.x, m.y);
  }
  a.m.hcOut[at] = make_float4(o.colour.x, o.colour.y, o.colour.z, o.colour.w);
  a.m.hgOut[at] = make_float4(o.guide.x, o.guide.y, o.guide.z, o.guide.w);
  a.m.hnOut[at] = o.length;
}

void launch_temporal_d(hipStream_t stream, const TemporalMArgs& a, const TemporalConst& k, const float4* albedo, bool moving, const uint32_t* ids, const MotionRec* table,
                       uint32_t numInstances)
{
  const dim3   grid = stage_grid(a.w, a.h, AD_TX, AD_TY), block(AD_TX, AD_TY);
  const AdArgs v{a, k, albedo, ids, table, numInstances};
  if(a.hm)
  {
    if(moving)
      k_temporal_d<true, true><<<grid, block, 0, stream>>>(v);
    else
      k_temporal_d<true, false><<<grid, block, 0, stream>>>(v);
  }
  else if(moving)
    k_temporal_d<false, true><<<grid, block, 0, stream>>>(v);
  else
    k_temporal_d<false, false><<<grid, block, 0, stream>>>(v);
}

// ---- the remodulation ---------------------------------------------------------------------------------------------------------------------------------------
// One pixel per lane: 16 B of colour and 16 B of albedo in, 16 B out.  out may be c: a lane touches only its own pixel.
#define RM_BLOCK 256

__global__ void __launch_bounds__(RM_BLOCK) k_remodulate(const float4* __restrict__ albedo, const float4* c, float4* out, size_t n)
{
  const size_t i = size_t(blockIdx.x) * RM_BLOCK + threadIdx.x;
  if(i >= n)
    return;
  const DnPx r = albedo_remodulate(stage_px(c[i]), stage_px(albedo[i]));
  out[i]       = make_float4(r.x, r.y, r.z, r.w);
}

void launch_remodulate(hipStream_t stream, const float4* albedo, const float4* c, float4* out, size_t n)
{
  k_remodulate<<<uint32_t((n + RM_BLOCK - 1) / RM_BLOCK), RM_BLOCK, 0, stream>>>(albedo, c, out, n);
}

// pt_debug_albedo_time's second part: the pass over the denoiser's two images (from the first into the second, so that every run multiplies the same values)
int debug_remodulate_time(pt_context* c, int reps, float* ms_out)
{
  const char* who = "pt_debug_albedo_time";
  STAGE_TRY(stage_need_image(c, who));
  if(!c->dGuide[0].p)
    return c->fail(PT_ERR_STATE, "%s: guide plane 0 (the albedo) must be installed", who);
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = stage_pixels(c);
  for(DevBuf& b : c->dDenoise)
    STAGE_TRY(dev_alloc(c, b, sizeof(float4) * n));
  HIP_TRY(c, hipMemsetAsync(c->dDenoise[0].p, 0, sizeof(float4) * n, c->stream));  // (the denoiser's images hold nothing between calls)
  return stage_time(c, who, reps, ms_out, [&] { launch_remodulate(c->stream, (const float4*)c->dGuide[0].p, (const float4*)c->dDenoise[0].p, (float4*)c->dDenoise[1].p, n); });
}
