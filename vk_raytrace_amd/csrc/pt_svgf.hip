// pt_read_temporal_moments / pt_svgf_variance / pt_svgf_history / pt_tonemap_svgf (include/pt_api.h): the variance-guided filter of the history
// (DESIGN.md section 5.4).  The per-pixel arithmetic is pt_svgf.h; this unit holds its kernels -- the temporal kernel that also writes the moments, the
// initial variance and the filter iteration -- their launches and the entry points.  No existing kernel is involved and none is compiled from other
// text than before: the stage reads the history pt_temporal.hip keeps and the current guide planes, and writes the denoiser's two images and two
// variance planes of its own.
#include "pt_stage.h"
#include "pt_svgf.h"

// ---- the temporal step with moments --------------------------------------------------------------------------------------------------------------------
// The 32 x 8 tile of k_temporal (pt_temporal.hip), one pixel per lane; temporal_pixel as it stands, with a probe on the lane's stack that svgf_moments
// reads (after inlining only the fields it reads remain), a float2 load per counted tap and a float2 store more.
#define SVT_TX 32
#define SVT_TY 8

struct SvTemporalArgs {
  TemporalMArgs m;
  TemporalConst k;
};
struct SvTemporalGlobal {
  const TemporalMArgs& a;
  __device__ size_t at(int x, int y) const { return size_t(y) * size_t(a.w) + size_t(x); }
  __device__ DnPx   colour(int x, int y) const { return stage_px(a.c[at(x, y)]); }
  __device__ DnPx   normal(int x, int y) const { return stage_px(a.g1[at(x, y)]); }
  __device__ DnPx   depth(int x, int y) const { return stage_px(a.g2[at(x, y)]); }
  __device__ DnPx   histColour(int x, int y) const { return stage_px(a.hc[at(x, y)]); }
  __device__ DnPx   histGuide(int x, int y) const { return stage_px(a.hg[at(x, y)]); }
  __device__ float  histLength(int x, int y) const { return a.hn[at(x, y)]; }
  __device__ SvM    histMoments(int x, int y) const
  {
    const float2 v = a.hm[at(x, y)];
    return SvM{v.x, v.y};
  }
};

__global__ void __launch_bounds__(SVT_TX * SVT_TY) k_temporal_m(SvTemporalArgs a)
{
  const int x = int(blockIdx.x) * SVT_TX + int(threadIdx.x), y = int(blockIdx.y) * SVT_TY + int(threadIdx.y);
  if(x >= a.m.w || y >= a.m.h)
    return;
  const SvTemporalGlobal src{a.m};
  TemporalProbe          pr;
  const TemporalOut      o  = temporal_pixel(src, a.k, x, y, a.m.w, a.m.h, &pr);
  const SvM              m  = svgf_moments(src, pr, o, src.colour(x, y));
  const size_t           at = size_t(y) * size_t(a.m.w) + size_t(x);
  a.m.hcOut[at]             = make_float4(o.colour.x, o.colour.y, o.colour.z, o.colour.w);
  a.m.hgOut[at]             = make_float4(o.guide.x, o.guide.y, o.guide.z, o.guide.w);
  a.m.hnOut[at]             = o.length;
  a.m.hmOut[at]             = make_float2(m.x, m.y);
}

void launch_temporal_m(hipStream_t stream, const TemporalMArgs& a, const TemporalConst& k)
{
  k_temporal_m<<<stage_grid(a.w, a.h, SVT_TX, SVT_TY), dim3(SVT_TX, SVT_TY), 0, stream>>>(SvTemporalArgs{a, k});
}

// ---- initial variance and the filter iteration ---------------------------------------------------------------------------------------------------------
// The 32 x 16 tile of k_denoise, one pixel per lane.
#define SV_TX 32
#define SV_TY 16
#define SV_BLOCK (SV_TX * SV_TY)
// Steps up to this one may stage the tile of every plane plus its 2 * step halo in LDS: four 16-byte planes and the 4-byte variance plane, 68 B per
// pixel -- step 1: 36 x 20 pixels = 48 960 B; step 2: 40 x 24 pixels = 65 280 B, 256 B below what a block may claim, so nothing else static lives in
// LDS there.  The 3 x 3 prefilter's halo of 1 lies inside every tile.  Larger steps read their taps from memory.
#define SV_LDS_MAX_STEP 2
// which of them do by default: profiles/svgf_rate.txt (tools/svgf_rate.py times every choice)
#define SV_LDS_DEFAULT_STEP 2

struct SvArgs {
  const float4* c;                     // colour in: the history's colour image at iteration 0
  const float4* g[PT_DENOISE_GUIDES];  // the current guide planes
  const float*  v;                     // variance in (k_svgf)
  const float*  hn;                    // history length (k_svgf_variance)
  const float2* hm;                    // history moments (k_svgf_variance)
  float4*       out;
  float*        vOut;
  int           w, h, iteration;
  SvgfConst     k;
};

struct SvGlobal {
  const SvArgs& a;
  __device__ size_t at(int x, int y) const { return size_t(y) * size_t(a.w) + size_t(x); }
  __device__ DnPx   colour(int x, int y) const { return stage_px(a.c[at(x, y)]); }
  __device__ DnPx   guide(int j, int x, int y) const { return stage_px(a.g[j][at(x, y)]); }
  __device__ float  variance(int x, int y) const { return a.v[at(x, y)]; }
  __device__ float  length(int x, int y) const { return a.hn[at(x, y)]; }
  __device__ SvM    moments(int x, int y) const
  {
    const float2 m = a.hm[at(x, y)];
    return SvM{m.x, m.y};
  }
};
// taps read from the block's tile: plane p (0: colour, 1 + j: guide j) at tile + p * tw * th, the variance in a plane of floats of its own
struct SvTile {
  const float4* tile;
  const float*  var;
  int           ox, oy, tw, planeStride;
  __device__ DnPx  colour(int x, int y) const { return stage_px(tile[(y - oy) * tw + (x - ox)]); }
  __device__ DnPx  guide(int j, int x, int y) const { return stage_px(tile[(1 + j) * planeStride + (y - oy) * tw + (x - ox)]); }
  __device__ float variance(int x, int y) const { return var[(y - oy) * tw + (x - ox)]; }
};

// the 7 x 7 window of k_svgf_variance read from the block's tile: per pixel the guide planes, the moments, the length and whether the colour is finite (as a
// colour that is: 0 or NaN in .x) -- 64 B; (32 + 6) x (16 + 6) pixels = 53 504 B
#define SVV_R 3
struct SvVarTile {
  const float4* g;
  const float2* m;
  const float * n, *fin;
  int           ox, oy, tw, planeStride;
  __device__ int   at(int x, int y) const { return (y - oy) * tw + (x - ox); }
  __device__ DnPx  colour(int x, int y) const { return DnPx{fin[at(x, y)], 0.0f, 0.0f, 0.0f}; }
  __device__ DnPx  guide(int j, int x, int y) const { return stage_px(g[j * planeStride + at(x, y)]); }
  __device__ float length(int x, int y) const { return n[at(x, y)]; }
  __device__ SvM   moments(int x, int y) const
  {
    const float2 v = m[at(x, y)];
    return SvM{v.x, v.y};
  }
};

// STAGED: a block in which some pixel takes the spatial branch stages the tile and its halo of 3 in LDS first (after a camera move the short histories are
// the disoccluded regions, which are contiguous: most blocks have none and skip the staging, the others have mostly such pixels).  Otherwise every tap
// reads memory.  Where the values come from is all that differs: both run svgf_variance_pixel.
template <bool STAGED>
__global__ void __launch_bounds__(SV_BLOCK) k_svgf_variance(SvArgs a)
{
  const int    x = int(blockIdx.x) * SV_TX + int(threadIdx.x), y = int(blockIdx.y) * SV_TY + int(threadIdx.y);
  const bool   inside = x < a.w && y < a.h;
  const size_t self   = inside ? size_t(y) * size_t(a.w) + size_t(x) : 0;
  if constexpr(STAGED)
  {
    constexpr int TW = SV_TX + 2 * SVV_R, TH = SV_TY + 2 * SVV_R;
    __shared__ float4 tg[PT_DENOISE_GUIDES * TW * TH];
    __shared__ float2 tm[TW * TH];
    __shared__ float  tn[TW * TH], tf[TW * TH];
    const bool spatial = inside && !(a.hn[self] >= a.k.minTemporal);
    if(__syncthreads_or(spatial ? 1 : 0))
    {
      const int ox = int(blockIdx.x) * SV_TX - SVV_R, oy = int(blockIdx.y) * SV_TY - SVV_R;
      for(int t = int(threadIdx.y) * SV_TX + int(threadIdx.x); t < TW * TH; t += SV_BLOCK)
      {
        const int gx = ox + t % TW, gy = oy + t / TW;
        if(gx < 0 || gx >= a.w || gy < 0 || gy >= a.h)
          continue;  // outside the image: no tap ever asks for it
        const size_t at = size_t(gy) * size_t(a.w) + size_t(gx);
        tm[t] = a.hm[at];
        tn[t] = a.hn[at];
        tf[t] = dn_finite3(stage_px(a.c[at])) ? 0.0f : ptf_nan();
        for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
          if(a.k.terms & (2u << j))
            tg[j * TW * TH + t] = a.g[j][at];
      }
      __syncthreads();
      if(inside)
        a.vOut[self] = svgf_variance_pixel(SvVarTile{tg, tm, tn, tf, ox, oy, TW, TW * TH}, x, y, a.w, a.h, a.k);
      return;
    }
  }
  if(inside)
    a.vOut[self] = svgf_variance_pixel(SvGlobal{a}, x, y, a.w, a.h, a.k);
}

// S > 0: the iteration of step S with its tile in LDS ((SV_TX + 4 S) x (SV_TY + 4 S) pixels per plane; a guide plane whose term is off is neither
// loaded nor read).  S == 0: any step, taps from memory.  Where the values come from is all that differs: both run svgf_pixel.
template <int S>
__global__ void __launch_bounds__(SV_BLOCK) k_svgf(SvArgs a)
{
  const int x = int(blockIdx.x) * SV_TX + int(threadIdx.x), y = int(blockIdx.y) * SV_TY + int(threadIdx.y);
  if constexpr(S > 0)
  {
    constexpr int TW = SV_TX + 4 * S, TH = SV_TY + 4 * S;
    __shared__ float4 tile[(1 + PT_DENOISE_GUIDES) * TW * TH];
    __shared__ float  var[TW * TH];
    const int ox = int(blockIdx.x) * SV_TX - 2 * S, oy = int(blockIdx.y) * SV_TY - 2 * S;
    for(int t = int(threadIdx.y) * SV_TX + int(threadIdx.x); t < TW * TH; t += SV_BLOCK)
    {
      const int gx = ox + t % TW, gy = oy + t / TW;
      if(gx < 0 || gx >= a.w || gy < 0 || gy >= a.h)
        continue;  // outside the image: no tap ever asks for it
      const size_t at = size_t(gy) * size_t(a.w) + size_t(gx);
      tile[t] = a.c[at];
      var[t]  = a.v[at];
      for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
        if(a.k.terms & (2u << j))
          tile[(1 + j) * TW * TH + t] = a.g[j][at];
    }
    __syncthreads();
    if(x >= a.w || y >= a.h)
      return;
    const SvOut  r  = svgf_pixel(SvTile{tile, var, ox, oy, TW, TW * TH}, x, y, a.w, a.h, a.iteration, a.k);
    const size_t at = size_t(y) * size_t(a.w) + size_t(x);
    a.out[at]       = make_float4(r.colour.x, r.colour.y, r.colour.z, r.colour.w);
    a.vOut[at]      = r.variance;
  }
  else
  {
    if(x >= a.w || y >= a.h)
      return;
    const SvOut  r  = svgf_pixel(SvGlobal{a}, x, y, a.w, a.h, a.iteration, a.k);
    const size_t at = size_t(y) * size_t(a.w) + size_t(x);
    a.out[at]       = make_float4(r.colour.x, r.colour.y, r.colour.z, r.colour.w);
    a.vOut[at]      = r.variance;
  }
}

static dim3 sv_grid(const SvArgs& a) { return stage_grid(a.w, a.h, SV_TX, SV_TY); }

static void launch_svgf_iteration(hipStream_t stream, const SvArgs& a, int ldsMaxStep)
{
  const dim3 grid = sv_grid(a), block(SV_TX, SV_TY);
  const int  step = 1 << a.iteration;
  if(step == 1 && ldsMaxStep >= 1)
    k_svgf<1><<<grid, block, 0, stream>>>(a);
  else if(step == 2 && ldsMaxStep >= 2)
    k_svgf<2><<<grid, block, 0, stream>>>(a);
  else
    k_svgf<0><<<grid, block, 0, stream>>>(a);
}

// Everything the entry points check, then the filter's buffers; the arguments every kernel of the call shares in `a`.  Nothing is launched here.
static int prepare_svgf(pt_context* c, const char* who, const pt_SvgfParams* p, SvArgs& a)
{
  STAGE_TRY(stage_need_image(c, who));
  STAGE_TRY(stage_need_history(c, who, true));
  const char* why = "";
  const int   rc  = svgf_constants(p, guide_planes_set(c), &a.k, &why);
  if(rc != PT_OK)
    return c->fail(rc, "%s: %s", who, why);
  HIP_TRY(c, hipSetDevice(c->device));
  for(int s = 0; s < 2; ++s)
  {
    STAGE_TRY(dev_alloc(c, c->dDenoise[s], sizeof(float4) * stage_pixels(c)));
    STAGE_TRY(dev_alloc(c, c->dSvgfVar[s], sizeof(float) * stage_pixels(c)));
  }
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    a.g[j] = (const float4*)c->dGuide[j].p;
  a.c         = (const float4*)c->hist.colour[c->hist.rd()].p;
  a.hn        = (const float*)c->hist.length[c->hist.rd()].p;
  a.hm        = (const float2*)c->hist.moments[c->hist.rd()].p;
  a.v         = nullptr;
  a.out       = nullptr;
  a.vOut      = nullptr;
  a.w         = c->width;
  a.h         = c->height;
  a.iteration = 0;
  return PT_OK;
}
// V0 into variance plane 0, enqueued on the context's stream; staged unless pt_debug_svgf_lds says 0
static void enqueue_variance(pt_context* c, SvArgs a)
{
  a.vOut = (float*)c->dSvgfVar[0].p;
  if(c->svgfLdsMaxStep == 0)
    k_svgf_variance<false><<<sv_grid(a), dim3(SV_TX, SV_TY), 0, c->stream>>>(a);
  else
    k_svgf_variance<true><<<sv_grid(a), dim3(SV_TX, SV_TY), 0, c->stream>>>(a);
}
// iterations first .. last - 1 behind V0; the colour of iteration 0 is the history's, later ones ping-pong the denoiser's two images, the variance
// ping-pongs the two planes (a tap reads positions other lanes write: never in place).  Returns where the last one wrote.
static void enqueue_iterations(pt_context* c, SvArgs a, int iterations, const float4*& colour, const float*& variance)
{
  float4* const cb[2]      = {(float4*)c->dDenoise[0].p, (float4*)c->dDenoise[1].p};
  float* const  vb[2]      = {(float*)c->dSvgfVar[0].p, (float*)c->dSvgfVar[1].p};
  const int     ldsMaxStep = stage_lds_step(c->svgfLdsMaxStep, SV_LDS_DEFAULT_STEP);
  for(int i = 0; i < iterations; ++i)
  {
    a.v         = vb[i & 1];
    a.vOut      = vb[(i & 1) ^ 1];
    a.out       = cb[i & 1];
    a.iteration = i;
    launch_svgf_iteration(c->stream, a, ldsMaxStep);
    a.c = a.out;
  }
  colour   = a.c;
  variance = a.vOut;
}
// On a demodulated history (section 5.6) the image after the last iteration is multiplied by guide plane 0, in place: it is one of the denoiser's two
// (iterations >= 1).  The variance stays in demodulated units.
static int enqueue_svgf(pt_context* c, const char* who, const pt_SvgfParams* p, const float4*& colour, const float*& variance)
{
  SvArgs a;
  STAGE_TRY(stage_need_albedo(c, who));  // (no history: not demodulated, and prepare_svgf says so)
  STAGE_TRY(prepare_svgf(c, who, p, a));
  enqueue_variance(c, a);
  enqueue_iterations(c, a, p->iterations, colour, variance);
  if(c->hist.demodulated)
    launch_remodulate(c->stream, a.g[0], colour, const_cast<float4*>(colour), stage_pixels(c));
  HIP_TRY(c, hipGetLastError());
  return PT_OK;
}

extern "C" {

int pt_read_temporal_moments(pt_context* c, float* m_out)
{
  CTX_CHECK(c);
  if(!m_out)
    return c->fail(PT_ERR_INVALID, "pt_read_temporal_moments: null");
  STAGE_TRY(stage_need_history(c, "pt_read_temporal_moments", true));
  HIP_TRY(c, hipSetDevice(c->device));
  return stage_read(c, {{m_out, c->hist.moments[c->hist.rd()].p, sizeof(float2) * stage_pixels(c)}});
}

int pt_svgf_variance(pt_context* c, const pt_SvgfParams* p, float* variance_out)
{
  CTX_CHECK(c);
  if(!p || !variance_out)
    return c->fail(PT_ERR_INVALID, "pt_svgf_variance: null");
  SvArgs a;
  STAGE_TRY(prepare_svgf(c, "pt_svgf_variance", p, a));
  enqueue_variance(c, a);
  HIP_TRY(c, hipGetLastError());
  return stage_read(c, {{variance_out, c->dSvgfVar[0].p, sizeof(float) * stage_pixels(c)}});
}

int pt_svgf_history(pt_context* c, const pt_SvgfParams* p, float* out, float* variance_out)
{
  CTX_CHECK(c);
  if(!p || !out)
    return c->fail(PT_ERR_INVALID, "pt_svgf_history: null");
  const float4* img = nullptr;
  const float*  var = nullptr;
  STAGE_TRY(enqueue_svgf(c, "pt_svgf_history", p, img, var));
  return stage_read(c, {{out, img, sizeof(float4) * stage_pixels(c)}, {variance_out, var, sizeof(float) * stage_pixels(c)}});
}

int pt_tonemap_svgf(pt_context* c, const pt_SvgfParams* p, const pt_Tonemapper* tm, uint8_t* out)
{
  CTX_CHECK(c);
  if(!p || !tm || !out)
    return c->fail(PT_ERR_INVALID, "pt_tonemap_svgf: null");
  const float4* img = nullptr;
  const float*  var = nullptr;
  STAGE_TRY(enqueue_svgf(c, "pt_tonemap_svgf", p, img, var));
  return stage_show(c, tm, img, out);
}

// Test and measurement access (not part of pt_api.h): the largest step whose iteration stages its tile in LDS, 0 .. SV_LDS_MAX_STEP (0: every iteration
// and the initial variance read their taps from memory; negative: back to the default).  Results do not depend on it.  Returns the value in force.
__attribute__((visibility("default"))) int pt_debug_svgf_lds(pt_context* c, int maxStep)
{
  CTX_CHECK(c);
  c->svgfLdsMaxStep = stage_lds_clamp(maxStep, SV_LDS_MAX_STEP);
  return stage_lds_step(c->svgfLdsMaxStep, SV_LDS_DEFAULT_STEP);
}

// Measurement access (not part of pt_api.h; tools/svgf_rate.py): one part of pt_svgf_history enqueued `reps` times between two events on the context's
// stream, after one untimed run of the whole filter (so that every plane a part reads holds what the filter leaves there) -- milliseconds per run in
// *ms_out, without any copy.  what: -2 the whole filter (V0 and params->iterations iterations); -1 k_svgf_variance alone; i >= 0: iteration i alone
// (i < params->iterations), reading the history's colour and variance plane 0 whatever i is.  Synchronous.
__attribute__((visibility("default"))) int pt_debug_svgf_time(pt_context* c, const pt_SvgfParams* p, int what, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!p || !ms_out || reps < 1 || what < -2 || what >= PT_SVGF_MAX_ITERATIONS)
    return c->fail(PT_ERR_INVALID, "pt_debug_svgf_time: null, reps < 1 or no such part");
  SvArgs a;
  STAGE_TRY(prepare_svgf(c, "pt_debug_svgf_time", p, a));
  if(what >= p->iterations)
    return c->fail(PT_ERR_INVALID, "pt_debug_svgf_time: iteration %d of %d", what, p->iterations);
  const float4* img = nullptr;
  const float*  var = nullptr;
  const int     ldsMaxStep = stage_lds_step(c->svgfLdsMaxStep, SV_LDS_DEFAULT_STEP);
  SvArgs        one        = a;  // a single iteration: in from the history and plane 0, out to the denoiser's image 1 and plane 1
  one.v         = (const float*)c->dSvgfVar[0].p;
  one.vOut      = (float*)c->dSvgfVar[1].p;
  one.out       = (float4*)c->dDenoise[1].p;
  one.iteration = what < 0 ? 0 : what;
  const auto whole = [&] {
    enqueue_variance(c, a);
    enqueue_iterations(c, a, p->iterations, img, var);
  };
  const auto part = [&] {
    if(what == -2)
      whole();
    else if(what == -1)
      enqueue_variance(c, a);
    else
      launch_svgf_iteration(c->stream, one, ldsMaxStep);
  };
  // untimed: the whole filter, and before single iterations V0 again, which plane 0 then holds
  return stage_time(c, "pt_debug_svgf_time", reps, ms_out, part, [&] {
    whole();
    if(what >= 0)
      enqueue_variance(c, a);
  });
}

}  // extern "C"
