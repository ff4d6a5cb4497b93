// pt_render_instance_plane / pt_set_instance_plane / pt_read_instance_plane and the kernels of pt_temporal_accumulate_moving (include/pt_api.h): motion
// of moving instances for the temporal stage.  The per-pixel bodies are pt_guides.h (instance_pixel) and pt_motion.h
// (temporal_pixel_moving); this unit holds their kernels, the launches and the instance plane's entry points.  The entry point of the moving temporal
// step, the history and the motion table's upload are pt_temporal.hip's.  No existing kernel is involved and none is compiled from other text than before.
#include "pt_stage.h"
#include "pt_guides.h"
#include "pt_motion.h"
#include "pt_svgf.h"  // svgf_moments: pt_temporal_track_moments applies to the moving form

// ---- the instance pass ------------------------------------------------------------------------------------------------------------------------------------
// k_guides (pt_guides.hip) with one word more per pixel: the same 8 x 8 pixel tile per block of 64 lanes, the same LDS traversal stack, and the waves
// per SIMD that kernel was timed for -- kept until this one is measured (-DPT_INSTANCES_WAVES=n / -DPT_INSTANCES_WAVES_TWO=n build another).
#ifndef PT_INSTANCES_WAVES
#define PT_INSTANCES_WAVES 5
#endif
#ifndef PT_INSTANCES_WAVES_TWO
#define PT_INSTANCES_WAVES_TWO 4
#endif
#define INSTANCES_TILE 8
static_assert(INSTANCES_TILE * INSTANCES_TILE == TRACE_BLOCK, "one pixel per lane");

struct InstanceArgs {
  uint32_t* ids;                       // row-major w x h
  float4*   plane[PT_DENOISE_GUIDES];  // read only for the planes in `planes`
  int       w, h;
  uint32_t  planes;  // PT_GUIDES_*, may be 0
  float     missDepth;
};

// lane l of block (bx, by) is pixel (8 bx + (l & 7), 8 by + (l >> 3)): the eight lanes of a tile row store 32 contiguous bytes of the instance plane
template <bool TWO>
__global__ void __launch_bounds__(TRACE_BLOCK, TWO ? PT_INSTANCES_WAVES_TWO : PT_INSTANCES_WAVES) k_instances(DeviceScene S, InstanceArgs a, Counters* counters)
{
  __shared__ uint32_t stack[STACK_LDS * TRACE_BLOCK];
  const int           x = int(blockIdx.x) * INSTANCES_TILE + int(threadIdx.x & 7u), y = int(blockIdx.y) * INSTANCES_TILE + int(threadIdx.x >> 3);
  if(x >= a.w || y >= a.h)
    return;
  GuidePixel     px;
  const uint32_t id = instance_pixel<TWO>(S, a.w, a.h, x, y, a.planes, a.missDepth, stack + threadIdx.x, counters, px);
  const size_t   at = size_t(y) * size_t(a.w) + size_t(x);
  a.ids[at]         = id;
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
    if(a.planes & (1u << j))
      a.plane[j][at] = px.plane[j];
}

static void launch_instances(pt_context* c, const InstanceArgs& a)
{
  const dim3 grid = stage_grid(a.w, a.h, INSTANCES_TILE, INSTANCES_TILE);
  if(c->scene.twoLevel)
    k_instances<true><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, a, (Counters*)c->dCounters.p);
  else
    k_instances<false><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, a, (Counters*)c->dCounters.p);
  c->renderedSinceCheck = true;  // the walks count into the same counter as the frames' (check_traversal)
}

// Everything pt_render_instance_plane checks -- pt_render_guides' list, but for the empty mask -- then the planes allocated; nothing is launched
static int prepare_instances(pt_context* c, const char* who, uint32_t planes, float missDepth, InstanceArgs& a)
{
  if(planes & ~(PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH))
    return c->fail(PT_ERR_INVALID, "%s: guide_planes = 0x%x (a mask of PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH, or 0)", who, planes);
  if(!(fabsf(missDepth) <= 3.402823466e38f))  // NaN, +-Inf
    return c->fail(PT_ERR_INVALID, "%s: miss_depth is not finite", who);
  if(!c->haveScene || !c->haveAccel)
    return c->fail(PT_ERR_STATE, "%s %s", who, c->no_accel());
  if(!c->haveCamera)
    return c->fail(PT_ERR_STATE, "%s before pt_set_camera", who);
  STAGE_TRY(stage_need_image(c, who));
  HIP_TRY(c, hipSetDevice(c->device));
  STAGE_TRY(dev_alloc(c, c->dInstPlane, sizeof(uint32_t) * stage_pixels(c)));
  for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
  {
    if(planes & (1u << j))
      STAGE_TRY(dev_alloc(c, c->dGuide[j], sizeof(float4) * stage_pixels(c)));
    a.plane[j] = (float4*)c->dGuide[j].p;
  }
  a.ids       = (uint32_t*)c->dInstPlane.p;
  a.w         = c->width;
  a.h         = c->height;
  a.planes    = planes;
  a.missDepth = missDepth;
  return PT_OK;
}

int debug_instances_time(pt_context* c, uint32_t planes, float missDepth, int reps, float* ms_out)
{
  InstanceArgs a;
  STAGE_TRY(prepare_instances(c, "pt_debug_motion_time", planes, missDepth, a));
  return stage_time(c, "pt_debug_motion_time", reps, ms_out, [&] { launch_instances(c, a); });
}

// ---- the moving temporal step -------------------------------------------------------------------------------------------------------------------------------
// k_temporal's 32 x 8 tile (pt_temporal.hip), one pixel per lane: a wave covers two rows of 32 pixels and reads the 4-byte instance plane in 128-byte runs,
// like the length plane.  The table is read behind the bound test and, past its `moved` word, only on the branch that applies it: neighbouring lanes name
// the same record, and the branch diverges only along the outlines of moved objects.
#define MV_TX 32
#define MV_TY 8

struct MvArgs {
  TemporalMArgs    m;  // m.hm / m.hmOut are read by the kernel with the moments image only
  TemporalConst    k;
  const uint32_t*  ids;
  const MotionRec* table;
  uint32_t         numInstances;
};
struct MvGlobal {
  const MvArgs& a;
  __device__ size_t   at(int x, int y) const { return size_t(y) * size_t(a.m.w) + size_t(x); }
  __device__ DnPx     colour(int x, int y) const { return stage_px(a.m.c[at(x, y)]); }
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

template <bool MOMENTS>
__global__ void __launch_bounds__(MV_TX * MV_TY) k_temporal_moving(MvArgs a)
{
  const int x = int(blockIdx.x) * MV_TX + int(threadIdx.x), y = int(blockIdx.y) * MV_TY + int(threadIdx.y);
  if(x >= a.m.w || y >= a.m.h)
    return;
  const MvGlobal src{a};
  const size_t   at = size_t(y) * size_t(a.m.w) + size_t(x);
  TemporalOut    o;
  if constexpr(MOMENTS)
  {
    TemporalProbe pr;
    o             = temporal_pixel_moving(src, a.k, a.table, a.numInstances, x, y, a.m.w, a.m.h, &pr);
    const SvM m   = svgf_moments(src, pr, o, src.colour(x, y));
    a.m.hmOut[at] = make_float2(m.x, m.y);
  }
  else
    o = temporal_pixel_moving(src, a.k, a.table, a.numInstances, x, y, a.m.w, a.m.h, nullptr);
  a.m.hcOut[at] = make_float4(o.colour.x, o.colour.y, o.colour.z, o.colour.w);
  a.m.hgOut[at] = make_float4(o.guide.x, o.guide.y, o.guide.z, o.guide.w);
  a.m.hnOut[at] = o.length;
}

void launch_temporal_moving(hipStream_t stream, const TemporalMArgs& a, const TemporalConst& k, const uint32_t* ids, const MotionRec* table, uint32_t numInstances)
{
  const dim3   grid = stage_grid(a.w, a.h, MV_TX, MV_TY), block(MV_TX, MV_TY);
  const MvArgs v{a, k, ids, table, numInstances};
  if(a.hm)
    k_temporal_moving<true><<<grid, block, 0, stream>>>(v);
  else
    k_temporal_moving<false><<<grid, block, 0, stream>>>(v);
}

extern "C" {

int pt_render_instance_plane(pt_context* c, uint32_t guide_planes, float miss_depth)
{
  CTX_CHECK(c);
  InstanceArgs a;
  STAGE_TRY(prepare_instances(c, "pt_render_instance_plane", guide_planes, miss_depth, a));
  launch_instances(c, a);  // (like pt_render_guides: frames pending or in flight share only the scene and the overflow counter with the pass)
  HIP_TRY(c, hipGetLastError());
  return PT_OK;
}

int pt_set_instance_plane(pt_context* c, const uint32_t* ids)
{
  CTX_CHECK(c);
  STAGE_TRY(stage_need_image(c, "pt_set_instance_plane"));
  HIP_TRY(c, hipSetDevice(c->device));
  if(!ids)
  {
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // a pass that writes the plane may be in flight
    dev_free(c->dInstPlane);
    return PT_OK;
  }
  const size_t bytes = sizeof(uint32_t) * stage_pixels(c);
  STAGE_TRY(dev_alloc(c, c->dInstPlane, bytes));
  HIP_TRY(c, hipMemcpyAsync(c->dInstPlane.p, ids, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

int pt_read_instance_plane(pt_context* c, uint32_t* ids_out)
{
  CTX_CHECK(c);
  if(!ids_out)
    return c->fail(PT_ERR_INVALID, "pt_read_instance_plane: null");
  STAGE_TRY(stage_need_image(c, "pt_read_instance_plane"));
  if(!c->dInstPlane.p)
    return c->fail(PT_ERR_STATE, "pt_read_instance_plane: no instance plane is installed");
  HIP_TRY(c, hipSetDevice(c->device));
  return stage_read(c, {{ids_out, c->dInstPlane.p, sizeof(uint32_t) * stage_pixels(c)}});
}

}  // extern "C"
