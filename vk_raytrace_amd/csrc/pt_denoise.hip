// pt_set_denoise_guides / pt_denoise / pt_tonemap_denoised (include/pt_api.h): the edge-avoiding a-trous denoiser as a stage of its own between the
// accumulation image and the display pass.  The per-pixel arithmetic is pt_denoise.h; this unit holds its kernels, their launches and the entry points.
// No existing kernel is involved: the stage reads the row-major image the display pass already produces (untile_to_rowmajor) and guide planes the
// caller installed, and writes to buffers of its own.
#include "pt_stage.h"

// One block filters a DN_TX x DN_TY tile of the image, one pixel per lane: a wave covers two rows of 32 pixels, so that adjacent lanes read adjacent
// 16-byte pixels (512 contiguous bytes per row and plane).
#define DN_TX 32
#define DN_TY 16
#define DN_BLOCK (DN_TX * DN_TY)
// Steps up to this one stage the tile of every plane plus its 2 * step halo in LDS; larger steps read their taps from memory (the taps of one lane are
// then 2^i pixels apart and a tile would mostly hold pixels nobody in the block asks for: 3x the tile at step 4, and with four planes more than the
// 64 KB a block may claim).  Step 2 with four planes: 40 x 24 pixels x 64 B = 60 KB, two blocks per CU.
#define DN_LDS_MAX_STEP 2
// which of them do by default: profiles/denoise_rate.txt (tools/denoise_rate.py times every choice)
#define DN_LDS_DEFAULT_STEP 2

struct DnArgs {
  const float4* c;
  const float4* g[PT_DENOISE_GUIDES];
  float4*       out;
  int           w, h, iteration;
  DenoiseConst  k;
};

// taps read from memory, one 16-byte load per plane
struct DnGlobal {
  const DnArgs& a;
  __device__ DnPx colour(int x, int y) const { return stage_px(a.c[size_t(y) * size_t(a.w) + size_t(x)]); }
  __device__ DnPx guide(int j, int x, int y) const { return stage_px(a.g[j][size_t(y) * size_t(a.w) + size_t(x)]); }
};
// taps read from the block's tile: plane p (0: colour, 1 + j: guide j) at tile + p * tw * th, pixel (ox, oy) of the image first
struct DnTile {
  const float4* tile;
  int           ox, oy, tw, planeStride;
  __device__ DnPx colour(int x, int y) const { return stage_px(tile[(y - oy) * tw + (x - ox)]); }
  __device__ DnPx guide(int j, int x, int y) const { return stage_px(tile[(1 + j) * planeStride + (y - oy) * tw + (x - ox)]); }
};

// S > 0: the iteration of step S with its tile in LDS ((DN_TX + 4 S) x (DN_TY + 4 S) pixels per plane; a plane whose term is off is neither loaded
// nor read).  S == 0: any step, taps from memory.  Where the values come from is all that differs: both run denoise_pixel.
template <int S>
__global__ void __launch_bounds__(DN_BLOCK) k_denoise(DnArgs a)
{
  const int x = int(blockIdx.x) * DN_TX + int(threadIdx.x), y = int(blockIdx.y) * DN_TY + int(threadIdx.y);
  if constexpr(S > 0)
  {
    constexpr int TW = DN_TX + 4 * S, TH = DN_TY + 4 * S;
    __shared__ float4 tile[(1 + PT_DENOISE_GUIDES) * TW * TH];
    const int ox = int(blockIdx.x) * DN_TX - 2 * S, oy = int(blockIdx.y) * DN_TY - 2 * S;
    for(int t = int(threadIdx.y) * DN_TX + int(threadIdx.x); t < TW * TH; t += DN_BLOCK)
    {
      const int gx = ox + t % TW, gy = oy + t / TW;
      if(gx < 0 || gx >= a.w || gy < 0 || gy >= a.h)
        continue;  // outside the image: no tap ever asks for it
      const size_t at = size_t(gy) * size_t(a.w) + size_t(gx);
      tile[t] = a.c[at];
      for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
        if(a.k.terms & (2u << j))
          tile[(1 + j) * TW * TH + t] = a.g[j][at];
    }
    __syncthreads();
    if(x >= a.w || y >= a.h)
      return;
    const DnPx r = denoise_pixel(DnTile{tile, ox, oy, TW, TW * TH}, x, y, a.w, a.h, a.iteration, a.k);
    a.out[size_t(y) * size_t(a.w) + size_t(x)] = make_float4(r.x, r.y, r.z, r.w);
  }
  else
  {
    if(x >= a.w || y >= a.h)
      return;
    const DnPx r = denoise_pixel(DnGlobal{a}, x, y, a.w, a.h, a.iteration, a.k);
    a.out[size_t(y) * size_t(a.w) + size_t(x)] = make_float4(r.x, r.y, r.z, r.w);
  }
}

// out = c / max(albedo, floor) (REMOD: c * max(albedo, floor)); out may be c
template <bool REMOD>
__global__ void __launch_bounds__(256) k_modulate(const float4* __restrict__ albedo, const float4* c, float4* out, size_t n)
{
  const size_t i = size_t(blockIdx.x) * 256u + threadIdx.x;
  if(i >= n)
    return;
  const DnPx r = REMOD ? denoise_remodulate(stage_px(c[i]), stage_px(albedo[i])) : denoise_demodulate(stage_px(c[i]), stage_px(albedo[i]));
  out[i]       = make_float4(r.x, r.y, r.z, r.w);
}

static void launch_iteration(hipStream_t stream, const DnArgs& a, int ldsMaxStep)
{
  const dim3 grid = stage_grid(a.w, a.h, DN_TX, DN_TY), block(DN_TX, DN_TY);
  const int  step = 1 << a.iteration;
  if(step == 1 && ldsMaxStep >= 1)
    k_denoise<1><<<grid, block, 0, stream>>>(a);
  else if(step == 2 && ldsMaxStep >= 2)
    k_denoise<2><<<grid, block, 0, stream>>>(a);
  else
    k_denoise<0><<<grid, block, 0, stream>>>(a);
}

// Everything the entry points check, then the row-major accumulation image enqueued on the context's stream behind the frames rendered so far
// (untile == false: the caller filters another image, the history of pt_temporal.hip, and the accumulation image is not asked for)
static int prepare_denoise(pt_context* c, const char* who, const pt_DenoiseParams* p, DenoiseConst& k, bool untile = true)
{
  STAGE_TRY(stage_need_image(c, who));
  const char* why = "";
  const int   rc  = denoise_constants(p, guide_planes_set(c), &k, &why);
  if(rc != PT_OK)
    return c->fail(rc, "%s: %s", who, why);
  STAGE_TRY(stage_need_full_image(c, who));
  HIP_TRY(c, hipSetDevice(c->device));
  for(DevBuf& b : c->dDenoise)
    STAGE_TRY(dev_alloc(c, b, sizeof(float4) * stage_pixels(c)));
  return untile ? untile_to_rowmajor(c) : PT_OK;
}
// The filter over the row-major image `src`, enqueued on the context's stream; returns the filtered row-major image (one of the denoiser's two, valid until the next call)
static const float4* enqueue_filter(pt_context* c, const float4* src, const pt_DenoiseParams* p, const DenoiseConst& k)
{
  const size_t  n      = stage_pixels(c);
  float4* const buf[2] = {(float4*)c->dDenoise[0].p, (float4*)c->dDenoise[1].p};
  const float4* cur    = src;
  const bool    demod  = (p->flags & PT_DENOISE_DEMODULATE) != 0u;
  const auto    blocks = uint32_t((n + 255u) / 256u);
  if(demod)
  {
    k_modulate<false><<<blocks, 256, 0, c->stream>>>((const float4*)c->dGuide[0].p, cur, buf[0], n);
    cur = buf[0];
  }
  DnArgs a;
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    a.g[j] = (const float4*)c->dGuide[j].p;
  a.w = c->width;
  a.h = c->height;
  a.k = k;
  const int ldsMaxStep = stage_lds_step(c->denoiseLdsMaxStep, DN_LDS_DEFAULT_STEP);
  for(int i = 0; i < p->iterations; ++i)
  {
    a.c         = cur;
    a.out       = cur == buf[0] ? buf[1] : buf[0];
    a.iteration = i;
    launch_iteration(c->stream, a, ldsMaxStep);
    cur = a.out;
  }
  if(demod)  // in place: `cur` is one of the denoiser's own images
    k_modulate<true><<<blocks, 256, 0, c->stream>>>((const float4*)c->dGuide[0].p, cur, const_cast<float4*>(cur), n);
  return cur;
}
static int enqueue_denoise(pt_context* c, const char* who, const pt_DenoiseParams* p, const float4*& result)
{
  DenoiseConst k;
  STAGE_TRY(prepare_denoise(c, who, p, k));
  result = enqueue_filter(c, (const float4*)c->dRowMajor.p, p, k);
  HIP_TRY(c, hipGetLastError());
  return PT_OK;
}
// ... of the history's colour image (pt_temporal.hip) instead of the accumulation image; p == NULL (pt_tonemap_history): no spatial filter, the
// history itself.  Reads the history and the current guide planes; writes the denoiser's own images only.
static int enqueue_denoise_history(pt_context* c, const char* who, const pt_DenoiseParams* p, const float4*& result)
{
  STAGE_TRY(stage_need_image(c, who));
  STAGE_TRY(stage_need_history(c, who, false));
  const float4* hist = (const float4*)c->hist.colour[c->hist.rd()].p;
  // a demodulated history: the final image is multiplied by guide plane 0 -- the filtered one in place (it is one of the
  // denoiser's two: iterations >= 1), the history itself into the denoiser's first image
  const bool    remod  = c->hist.demodulated;
  const float4* albedo = (const float4*)c->dGuide[0].p;
  STAGE_TRY(stage_need_albedo(c, who));
  const char* why = "";
  if(p && albedo_denoise_flags(remod, p->flags, &why) != PT_OK)
    return c->fail(PT_ERR_STATE, "%s: %s", who, why);
  if(!p)
  {
    HIP_TRY(c, hipSetDevice(c->device));
    result = hist;
    if(remod)
    {
      STAGE_TRY(dev_alloc(c, c->dDenoise[0], sizeof(float4) * stage_pixels(c)));
      launch_remodulate(c->stream, albedo, hist, (float4*)c->dDenoise[0].p, stage_pixels(c));
      HIP_TRY(c, hipGetLastError());
      result = (const float4*)c->dDenoise[0].p;
    }
    return PT_OK;
  }
  DenoiseConst k;
  STAGE_TRY(prepare_denoise(c, who, p, k, false));
  result = enqueue_filter(c, hist, p, k);
  if(remod)
    launch_remodulate(c->stream, albedo, result, const_cast<float4*>(result), stage_pixels(c));
  HIP_TRY(c, hipGetLastError());
  return PT_OK;
}

extern "C" {

int pt_set_denoise_guides(pt_context* c, const float* const planes[PT_DENOISE_GUIDES])
{
  CTX_CHECK(c);
  if(!planes)
    return c->fail(PT_ERR_INVALID, "pt_set_denoise_guides: null");
  STAGE_TRY(stage_need_image(c, "pt_set_denoise_guides"));
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = sizeof(float4) * stage_pixels(c);
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
  {
    if(!planes[j])
    {
      dev_free(c->dGuide[j]);
      continue;
    }
    STAGE_TRY(dev_alloc(c, c->dGuide[j], bytes));
    HIP_TRY(c, hipMemcpyAsync(c->dGuide[j].p, planes[j], bytes, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

int pt_denoise(pt_context* c, const pt_DenoiseParams* p, float* out)
{
  CTX_CHECK(c);
  if(!p || !out)
    return c->fail(PT_ERR_INVALID, "pt_denoise: null");
  const float4* img = nullptr;
  STAGE_TRY(enqueue_denoise(c, "pt_denoise", p, img));
  return stage_read(c, {{out, img, sizeof(float4) * stage_pixels(c)}});
}

int pt_tonemap_denoised(pt_context* c, const pt_DenoiseParams* p, const pt_Tonemapper* tm, uint8_t* out)
{
  CTX_CHECK(c);
  if(!p || !tm || !out)
    return c->fail(PT_ERR_INVALID, "pt_tonemap_denoised: null");
  const float4* img = nullptr;
  STAGE_TRY(enqueue_denoise(c, "pt_tonemap_denoised", p, img));
  return stage_show(c, tm, img, out);
}

int pt_denoise_history(pt_context* c, const pt_DenoiseParams* p, float* out)
{
  CTX_CHECK(c);
  if(!p || !out)
    return c->fail(PT_ERR_INVALID, "pt_denoise_history: null");
  const float4* img = nullptr;
  STAGE_TRY(enqueue_denoise_history(c, "pt_denoise_history", p, img));
  return stage_read(c, {{out, img, sizeof(float4) * stage_pixels(c)}});
}

int pt_tonemap_history(pt_context* c, const pt_DenoiseParams* p, const pt_Tonemapper* tm, uint8_t* out)
{
  CTX_CHECK(c);
  if(!tm || !out)
    return c->fail(PT_ERR_INVALID, "pt_tonemap_history: null");
  const float4* img = nullptr;
  STAGE_TRY(enqueue_denoise_history(c, "pt_tonemap_history", p, img));
  return stage_show(c, tm, img, out);
}

// Test and measurement access (not part of pt_api.h): the largest step whose iteration stages its tile in LDS, 0 .. DN_LDS_MAX_STEP (0: every
// iteration reads its taps from memory; negative: back to the default).  Results do not depend on it.  Returns the value in force.
__attribute__((visibility("default"))) int pt_debug_denoise_lds(pt_context* c, int maxStep)
{
  CTX_CHECK(c);
  c->denoiseLdsMaxStep = stage_lds_clamp(maxStep, DN_LDS_MAX_STEP);
  return stage_lds_step(c->denoiseLdsMaxStep, DN_LDS_DEFAULT_STEP);
}

// Measurement access (not part of pt_api.h; tools/denoise_rate.py): the filter of pt_denoise enqueued `reps` times between two events on the context's
// stream, after one untimed run -- milliseconds per run in *ms_out, without the untile pass before it and without any copy.  Synchronous.
__attribute__((visibility("default"))) int pt_debug_denoise_time(pt_context* c, const pt_DenoiseParams* p, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!ms_out || reps < 1)
    return c->fail(PT_ERR_INVALID, "pt_debug_denoise_time: null or reps < 1");
  DenoiseConst k;
  STAGE_TRY(prepare_denoise(c, "pt_debug_denoise_time", p, k));
  return stage_time(c, "pt_debug_denoise_time", reps, ms_out, [&] { (void)enqueue_filter(c, (const float4*)c->dRowMajor.p, p, k); });
}

}  // extern "C"
