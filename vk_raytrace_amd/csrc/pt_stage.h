// The scaffold the image stages of the display path share (pt_denoise.hip, pt_guides.hip, pt_temporal.hip, pt_svgf.hip): what their entry points check
// before they launch, with the one text of each refusal; how they hand planes back; the display tail; the device-event timing of the pt_debug_*_time
// entries.  Host code, but for stage_px.  Internal: not installed.  The kernels, their argument structures and their launches stay in the stage's own unit.
#pragma once
#include <initializer_list>
#include "pt_context.h"
#include "pt_denoise.h"  // DnPx
#include "pt_albedo.h"   // what a demodulated history refuses, with the texts

#define STAGE_TRY(call)    \
  do                       \
  {                        \
    const int rc_ = (call); \
    if(rc_ != PT_OK)       \
      return rc_;          \
  } while(0)

// a pixel as the kernels load it (16 bytes), as the per-pixel headers take it
PT_DN DnPx stage_px(const float4& v) { return DnPx{v.x, v.y, v.z, v.w}; }

// ---- preconditions: PT_OK, or PT_ERR_STATE with the reason in pt_last_error; `who` (the entry point) is its leading word --------------------------------
static inline int stage_need_image(pt_context* c, const char* who) { return c->width == 0 ? c->fail(PT_ERR_STATE, "%s before pt_resize", who) : PT_OK; }
static inline int stage_need_full_image(pt_context* c, const char* who)
{
  if(c->nranks > 1 && !c->haveFull)
    return c->fail(PT_ERR_STATE, "%s: rank %d of %d holds only its own tiles; gather the image first", who, c->rank, c->nranks);
  return PT_OK;
}
static inline int stage_need_history(pt_context* c, const char* who, bool moments)
{
  if(!c->hist.have)
    return c->fail(PT_ERR_STATE, "%s: there is no history (no pt_temporal_accumulate since pt_resize / pt_temporal_reset)", who);
  if(moments && !c->hist.hasMoments)
    return c->fail(PT_ERR_STATE, "%s: the history was made without moments (pt_temporal_track_moments)", who);
  return PT_OK;
}

static inline uint32_t guide_planes_set(const pt_context* c);  // (under "small things")
// a consumer of the history: this history is demodulated and guide plane 0, which its final image is multiplied by, is missing
static inline int stage_need_albedo(pt_context* c, const char* who)
{
  const char* why = "";
  const int   rc  = albedo_need_plane(c->hist.demodulated, guide_planes_set(c), &why);
  return rc != PT_OK ? c->fail(rc, "%s: %s", who, why) : PT_OK;
}

// ---- small things -----------------------------------------------------------------------------------------------------------------------------------------
static inline uint32_t guide_planes_set(const pt_context* c)  // bit j: guide plane j is installed
{
  uint32_t m = 0;
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    m |= c->dGuide[j].p ? 1u << j : 0u;
  return m;
}
static inline size_t stage_pixels(const pt_context* c) { return size_t(c->width) * size_t(c->height); }
static inline dim3   stage_grid(int w, int h, int tx, int ty) { return dim3((w + tx - 1) / tx, (h + ty - 1) / ty); }
// The largest step whose iteration stages its tile in LDS, as a context keeps it (negative: the measured default): the value in force, and what
// pt_debug_*_lds stores -- 0 .. limit, or -1
static inline int stage_lds_step(int setting, int dflt) { return setting < 0 ? dflt : setting; }
static inline int stage_lds_clamp(int maxStep, int limit) { return maxStep < 0 ? -1 : maxStep > limit ? limit : maxStep; }

// frees what the stages keep per image size: the denoiser's images, the guide planes, the history and the filter's variance planes
static inline void stages_release(pt_context* c)
{
  for(DevBuf& b : c->dDenoise)
    dev_free(b);
  for(DevBuf& b : c->dGuide)
    dev_free(b);
  dev_free(c->dInstPlane);
  dev_free(c->dMotionTable);
  dev_free(c->dChainPlane);
  for(DevBuf& b : c->dSvgfVar)
    dev_free(b);
  c->hist.release();
}

// ---- handing results back -----------------------------------------------------------------------------------------------------------------------------------
struct StageCopy {
  void*       dst;  // host; NULL: not asked for
  const void* src;  // device
  size_t      bytes;
};
// the copies enqueued on the context's stream behind what the call launched, then everything waited for
static inline int stage_read(pt_context* c, std::initializer_list<StageCopy> copies)
{
  for(const StageCopy& k : copies)
    if(k.dst)
      HIP_TRY(c, hipMemcpyAsync(k.dst, k.src, k.bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_all(c));
  return check_traversal(c);
}
// the display pass over the row-major `image` (accumulation size) instead of the accumulation image: mip chain, tonemap, the bytes in `out`
static inline int stage_show(pt_context* c, const pt_Tonemapper* tm, const float4* image, uint8_t* out)
{
  MipView mv{};
  STAGE_TRY(display_levels(c, image, c->width, c->height, (tm->autoExposure & 1) != 0, mv));
  STAGE_TRY(display_finish(c, tm, mv, c->width, c->height, out));
  HIP_TRY(c, sync_all(c));
  return check_traversal(c);
}

// ---- timing (the pt_debug_*_time entries) -------------------------------------------------------------------------------------------------------------------
// warm() once, untimed; then enqueue() `reps` times between two events on the context's stream: milliseconds per run in *ms_out.  Synchronous.  The caller
// has checked its arguments (reps >= 1, ms_out) and its state; both callables only enqueue on c->stream.
template <class Enqueue, class Warm>
static int stage_time(pt_context* c, const char* who, int reps, float* ms_out, Enqueue enqueue, Warm warm)
{
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_TRY(c, hipEventCreate(&ev[0]));
  if(hipEventCreate(&ev[1]) != hipSuccess)
  {
    (void)hipEventDestroy(ev[0]);
    return c->fail(PT_ERR_HIP, "%s: hipEventCreate", who);
  }
  warm();
  hipError_t e = hipEventRecord(ev[0], c->stream);
  for(int i = 0; i < reps && e == hipSuccess; ++i)
    enqueue();
  if(e == hipSuccess) e = hipGetLastError();
  if(e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
  if(e == hipSuccess) e = sync_all(c);
  float ms = 0.0f;
  if(e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  if(e != hipSuccess)
    return c->fail(PT_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  *ms_out = ms / float(reps);
  return check_traversal(c);
}
// ... where the untimed run is one run of what is timed
template <class Enqueue>
static int stage_time(pt_context* c, const char* who, int reps, float* ms_out, Enqueue enqueue)
{
  return stage_time(c, who, reps, ms_out, enqueue, enqueue);
}
