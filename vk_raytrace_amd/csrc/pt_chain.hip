// pt_render_guides_chain / pt_read_guide_chain (include/pt_api.h): the guide planes of the first surface behind mirrors and clear glass (DESIGN.md
// section 5.8).  The per-pixel body is pt_chain.h; this unit holds its kernel, the launch and the entry points.  No existing kernel is involved and none
// is compiled from other text than before: the pass walks the structures the frames walk and writes only the context's guide planes and its link plane.
#include "pt_stage.h"
#include "pt_chain.h"

// Waves per SIMD the kernel is compiled for, flat / two-level, chosen by timing the candidates of k_guides at 1080p with every surface followed at
// maxLinks 1 (nothing followed in brackets): flat 4 / 5 / 6 waves 2.17 / 2.08 / 2.94 ms (0.85 / 0.84 / 1.20), two-level 3 / 4 / 5 waves
// 3.34 / 3.40 / 4.55 ms (1.38 / 1.38 / 1.87) -- profiles/chain_rate.txt; DESIGN.md section 5.8 has the registers of each.  The loop around the walk keeps
// more alive than k_guides does: at 4 waves the two-level kernel spills 192 B of registers, at 3 16 B.  -DPT_CHAIN_WAVES=n / -DPT_CHAIN_WAVES_TWO=n
// build another.
#ifndef PT_CHAIN_WAVES
#define PT_CHAIN_WAVES 5
#endif
#ifndef PT_CHAIN_WAVES_TWO
#define PT_CHAIN_WAVES_TWO 3
#endif
#define CHAIN_TILE 8  // k_guides' geometry: a block of TRACE_BLOCK lanes covers 8 x 8 pixels
static_assert(CHAIN_TILE * CHAIN_TILE == TRACE_BLOCK, "one pixel per lane");

struct ChainArgs {
  float4*    plane[PT_DENOISE_GUIDES];  // row-major w x h; read only for the planes in `planes`
  uint32_t*  links;                     // row-major w x h: links | end << 8, always written
  int        w, h;
  uint32_t   planes;  // PT_GUIDES_*
  float      missDepth;
  ChainConst k;
};

// lane l of block (bx, by) is pixel (8 bx + (l & 7), 8 by + (l >> 3)).  A lane's chain is a loop of at most maxLinks + 1 walks; a lane whose chain has
// ended idles until its wavefront is done.  A pixel writes 16 bytes per selected plane and its link word.
template <bool TWO>
__global__ void __launch_bounds__(TRACE_BLOCK, TWO ? PT_CHAIN_WAVES_TWO : PT_CHAIN_WAVES) k_guides_chain(DeviceScene S, ChainArgs a, Counters* counters)
{
  __shared__ uint32_t stack[STACK_LDS * TRACE_BLOCK];
  const int           x = int(blockIdx.x) * CHAIN_TILE + int(threadIdx.x & 7u), y = int(blockIdx.y) * CHAIN_TILE + int(threadIdx.x >> 3);
  if(x >= a.w || y >= a.h)
    return;
  GuidePixel     px;
  const uint32_t word = chain_pixel<TWO>(S, a.k, a.w, a.h, x, y, a.planes, a.missDepth, stack + threadIdx.x, counters, px);
  const size_t   at   = size_t(y) * size_t(a.w) + size_t(x);
  a.links[at]         = word;
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    if(a.planes & (1u << j))
      a.plane[j][at] = px.plane[j];
}

static void launch_chain(pt_context* c, const ChainArgs& a)
{
  const dim3 grid = stage_grid(a.w, a.h, CHAIN_TILE, CHAIN_TILE);
  if(c->scene.twoLevel)
    k_guides_chain<true><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, a, (Counters*)c->dCounters.p);
  else
    k_guides_chain<false><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, a, (Counters*)c->dCounters.p);
  c->renderedSinceCheck = true;  // the walks count into the same counter as the frames' (check_traversal)
}

// Everything pt_render_guides_chain checks -- pt_render_guides' list and the chain parameters -- then the planes allocated; nothing is launched
static int prepare_chain(pt_context* c, const char* who, const pt_GuideChain* chain, uint32_t planes, float missDepth, ChainArgs& a)
{
  const char* why = "";
  const int   rc  = chain_constants(chain, &a.k, &why);
  if(rc != PT_OK)
    return c->fail(rc, "%s: %s", who, why);
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
  STAGE_TRY(dev_alloc(c, c->dChainPlane, sizeof(uint32_t) * stage_pixels(c)));
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
  {
    if(planes & (1u << j))
      STAGE_TRY(dev_alloc(c, c->dGuide[j], sizeof(float4) * stage_pixels(c)));
    a.plane[j] = (float4*)c->dGuide[j].p;
  }
  a.links     = (uint32_t*)c->dChainPlane.p;
  a.w         = c->width;
  a.h         = c->height;
  a.planes    = planes;
  a.missDepth = missDepth;
  return PT_OK;
}

extern "C" {

int pt_render_guides_chain(pt_context* c, const pt_GuideChain* chain, uint32_t planes, float miss_depth)
{
  CTX_CHECK(c);
  ChainArgs a;
  STAGE_TRY(prepare_chain(c, "pt_render_guides_chain", chain, planes, miss_depth, a));
  launch_chain(c, a);  // (like pt_render_guides: frames pending or in flight share only the scene and the overflow counter with the pass)
  HIP_TRY(c, hipGetLastError());
  return PT_OK;
}

int pt_read_guide_chain(pt_context* c, uint32_t* links_out)
{
  CTX_CHECK(c);
  if(!links_out)
    return c->fail(PT_ERR_INVALID, "pt_read_guide_chain: null");
  STAGE_TRY(stage_need_image(c, "pt_read_guide_chain"));
  const char* why = "";
  const int   rc  = chain_need_plane(c->dChainPlane.p != nullptr, &why);
  if(rc != PT_OK)
    return c->fail(rc, "pt_read_guide_chain: %s", why);
  HIP_TRY(c, hipSetDevice(c->device));
  return stage_read(c, {{links_out, c->dChainPlane.p, sizeof(uint32_t) * stage_pixels(c)}});
}

// Measurement access (not part of pt_api.h; tools/chain_rate.py): the pass of pt_render_guides_chain enqueued `reps` times between two events on the
// context's stream, after one untimed run -- milliseconds per run in *ms_out.  Synchronous.
__attribute__((visibility("default"))) int pt_debug_guides_chain_time(pt_context* c, const pt_GuideChain* chain, uint32_t planes, float miss_depth, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!ms_out || reps < 1)
    return c->fail(PT_ERR_INVALID, "pt_debug_guides_chain_time: null or reps < 1");
  ChainArgs a;
  STAGE_TRY(prepare_chain(c, "pt_debug_guides_chain_time", chain, planes, miss_depth, a));
  return stage_time(c, "pt_debug_guides_chain_time", reps, ms_out, [&] { launch_chain(c, a); });
}

}  // extern "C"
