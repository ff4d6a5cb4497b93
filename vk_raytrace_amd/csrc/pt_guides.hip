// pt_render_guides / pt_read_denoise_guides (include/pt_api.h): the denoiser's guide planes rendered on the device in one first-hit pass.  The
// per-pixel body is pt_guides.h; this unit holds its kernel, the launch and the entry points.  No existing kernel is involved: the pass walks the
// structures the frames walk, with the functions the frames' kernels are made of, and writes only the context's guide planes.
#include "pt_stage.h"
#include "pt_guides.h"

// Waves per SIMD the kernel is compiled for, flat / two-level: k_query's (pt_query.hip), kept after timing the neighbours -- flat 4 / 5 / 6 waves
// 0.84 / 0.81 / 0.96 ms, two-level 3 / 4 / 5 waves 1.39 / 1.37 / 1.76 ms at 1080p (profiles/guides_rate.txt; DESIGN.md section 5.2 has the registers
// of each).  -DPT_GUIDES_WAVES=n / -DPT_GUIDES_WAVES_TWO=n build another.
#ifndef PT_GUIDES_WAVES
#define PT_GUIDES_WAVES 5
#endif
#ifndef PT_GUIDES_WAVES_TWO
#define PT_GUIDES_WAVES_TWO 4
#endif
#define GUIDES_TILE 8  // a block of TRACE_BLOCK lanes covers GUIDES_TILE x GUIDES_TILE pixels: coherent primary rays, like the reference's 8 x 8 workgroup
static_assert(GUIDES_TILE * GUIDES_TILE == TRACE_BLOCK, "one pixel per lane");

struct GuideArgs {
  float4*  plane[PT_DENOISE_GUIDES];  // row-major w x h; read only for the planes in `planes`
  int      w, h;
  uint32_t planes;  // PT_GUIDES_*
  float    missDepth;
};

// grid = ceil(w / 8) x ceil(h / 8) blocks of 64 lanes; lane l of block (bx, by) is pixel (8 bx + (l & 7), 8 by + (l >> 3)).  A pixel writes 16 bytes
// per selected plane and nothing else.
template <bool TWO>
__global__ void __launch_bounds__(TRACE_BLOCK, TWO ? PT_GUIDES_WAVES_TWO : PT_GUIDES_WAVES) k_guides(DeviceScene S, GuideArgs a, Counters* counters)
{
  __shared__ uint32_t stack[STACK_LDS * TRACE_BLOCK];
  const int           x = int(blockIdx.x) * GUIDES_TILE + int(threadIdx.x & 7u), y = int(blockIdx.y) * GUIDES_TILE + int(threadIdx.x >> 3);
  if(x >= a.w || y >= a.h)
    return;
  GuidePixel px;
  guide_pixel<TWO>(S, a.w, a.h, x, y, a.planes, a.missDepth, stack + threadIdx.x, counters, px);
  const size_t at = size_t(y) * size_t(a.w) + size_t(x);
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    if(a.planes & (1u << j))
      a.plane[j][at] = px.plane[j];
}

static void launch_guides(pt_context* c, const GuideArgs& a)
{
  const dim3 grid = stage_grid(a.w, a.h, GUIDES_TILE, GUIDES_TILE);
  if(c->scene.twoLevel)
    k_guides<true><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, a, (Counters*)c->dCounters.p);
  else
    k_guides<false><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, a, (Counters*)c->dCounters.p);
  c->renderedSinceCheck = true;  // the walks count into the same counter as the frames' (check_traversal)
}

// Everything pt_render_guides checks, then the selected planes allocated; nothing is launched
static int prepare_guides(pt_context* c, const char* who, uint32_t planes, float missDepth, GuideArgs& a)
{
  if(planes == 0u || (planes & ~(PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH)))
    return c->fail(PT_ERR_INVALID, "%s: planes = 0x%x (a non-empty mask of PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH)", who, planes);
  if(!(fabsf(missDepth) <= 3.402823466e38f))  // NaN, +-Inf
    return c->fail(PT_ERR_INVALID, "%s: miss_depth is not finite", who);
  if(!c->haveScene || !c->haveAccel)
    return c->fail(PT_ERR_STATE, "%s %s", who, c->no_accel());
  if(!c->haveCamera)
    return c->fail(PT_ERR_STATE, "%s before pt_set_camera", who);
  STAGE_TRY(stage_need_image(c, who));
  HIP_TRY(c, hipSetDevice(c->device));
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
  {
    if(planes & (1u << j))
      STAGE_TRY(dev_alloc(c, c->dGuide[j], sizeof(float4) * stage_pixels(c)));
    a.plane[j] = (float4*)c->dGuide[j].p;
  }
  a.w         = c->width;
  a.h         = c->height;
  a.planes    = planes;
  a.missDepth = missDepth;
  return PT_OK;
}

extern "C" {

int pt_render_guides(pt_context* c, uint32_t planes, float miss_depth)
{
  CTX_CHECK(c);
  GuideArgs a;
  STAGE_TRY(prepare_guides(c, "pt_render_guides", planes, miss_depth, a));
  // frames handed to pt_render_frame stay pending and frames in flight keep running on their slots' streams: the pass shares nothing with them
  // but the scene, which it only reads, and the overflow counter, which both only add to
  launch_guides(c, a);
  HIP_TRY(c, hipGetLastError());
  return PT_OK;
}

int pt_read_denoise_guides(pt_context* c, float* const planes_out[PT_DENOISE_GUIDES])
{
  CTX_CHECK(c);
  if(!planes_out)
    return c->fail(PT_ERR_INVALID, "pt_read_denoise_guides: null");
  STAGE_TRY(stage_need_image(c, "pt_read_denoise_guides"));
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    if(planes_out[j] && !c->dGuide[j].p)
      return c->fail(PT_ERR_STATE, "pt_read_denoise_guides: guide plane %d is not installed", j);
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = sizeof(float4) * stage_pixels(c);
  static_assert(PT_DENOISE_GUIDES == 3, "one copy per plane");
  return stage_read(c, {{planes_out[0], c->dGuide[0].p, bytes}, {planes_out[1], c->dGuide[1].p, bytes}, {planes_out[2], c->dGuide[2].p, bytes}});
}

// Measurement access (not part of pt_api.h; tools/guides_rate.py): the pass of pt_render_guides enqueued `reps` times between two events on the
// context's stream, after one untimed run -- milliseconds per run in *ms_out.  Synchronous.
__attribute__((visibility("default"))) int pt_debug_guides_time(pt_context* c, uint32_t planes, float miss_depth, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!ms_out || reps < 1)
    return c->fail(PT_ERR_INVALID, "pt_debug_guides_time: null or reps < 1");
  GuideArgs a;
  STAGE_TRY(prepare_guides(c, "pt_debug_guides_time", planes, miss_depth, a));
  return stage_time(c, "pt_debug_guides_time", reps, ms_out, [&] { launch_guides(c, a); });
}

}  // extern "C"
