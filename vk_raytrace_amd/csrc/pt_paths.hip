// pt_trace_paths (include/pt_api.h): the radiance along caller rays, one ray per lane.  The per-ray body is pt_paths.h; this
// unit holds its kernel, the launch and the entry point with its checks and staging.  No existing kernel is involved: the paths walk the structures
// the frames walk and are shaded by the functions the frames' kernels are made of, on a path state that lives in the lane.
#include "pt_stage.h"  // stage_time
#include "pt_machine.h"  // supply_next
#include "pt_paths.h"

// wavefronts of a launch unless pt_debug_paths_waves says otherwise: k_tail's (pt_render.hip), 2 per SIMD on 256 CUs
#define PT_PATHS_WAVES 2048u

PT_DEV void store_result(pt_PathResult* __restrict__ results, uint32_t i, const pt_PathResult& r)
{
  float4* op = reinterpret_cast<float4*>(results + i);
  op[0]      = make_float4(r.radiance[0], r.radiance[1], r.radiance[2], r.firstT);
  op[1]      = make_float4(__uint_as_float(r.seed), __uint_as_float(r.status), __uint_as_float(r.closestRays), __uint_as_float(r._pad));
}

// Path lengths differ widely (Russian roulette from depth 0, misses, maxSamples paths per ray), so the rays are not dealt out up front.  k_tail's
// shape (pt_render.hip): persistent wavefronts, one ray per lane carried bounce by bounce (path_step) through every sample -- the seed chains -- and
// a lane whose ray is finished stores its record and takes the next ray index from the supply (supply_next: a wave reserves 64 consecutive rays
// with one atomic on chunkCounter, zero at launch) while its neighbours go on.  Nothing waits for the longest path of a wavefront's rays, only for
// the longest remaining one at the end.  A ray's record does not depend on which lane ran it.  rays / results are 16-byte aligned (pt_trace_paths
// checks the caller's device pointers; the staging buffers are allocations).
template <bool TWO>
__global__ void __launch_bounds__(TRACE_BLOCK, 2)
    k_paths(DeviceScene S, FrameParams fp, uint32_t n, const pt_Ray* __restrict__ rays, pt_PathResult* __restrict__ results, uint32_t* chunkCounter, Counters* counters)
{
  __shared__ uint32_t stack[STACK_LDS * TRACE_BLOCK];
  uint32_t* lds = stack + threadIdx.x;
  RaySupply rs;
  rs.chunk       = 64;
  PathLane L;
  uint32_t i     = 0;
  bool     alive = false;
#pragma unroll 1
  for(;;)
  {
    const uint32_t qi = supply_next(rs, chunkCounter, n, !alive);
    if(qi != 0xffffffffu)  // (qi < n: supply_next hands out indices below `count` only)
    {
      i                = qi;
      const float4* rp = reinterpret_cast<const float4*>(rays + i);
      const float4  a = rp[0], b = rp[1];
      pt_Ray        ray;
      ray.origin[0] = a.x; ray.origin[1] = a.y; ray.origin[2] = a.z; ray.tmax = a.w;
      ray.direction[0] = b.x; ray.direction[1] = b.y; ray.direction[2] = b.z; ray.seed = __float_as_uint(b.w);
      pt_PathResult invalid;
      alive = path_begin(fp, ray, L, invalid);
      if(!alive)
        store_result(results, i, invalid);  // (the lane asks again in the next round)
    }
    // nobody has a ray: either the supply has run dry, or every ray just handed out was invalid -- then the next round asks again
    if(!__ballot(alive) && !rs.more)
      break;
    if(alive && path_step<TWO>(S, fp, fp.variant, L, lds, counters))
    {
      store_result(results, i, path_end(fp, L));
      alive = false;
    }
  }
}

// n rays (at most 2^30 per launch: the caller cuts longer arrays) on the context's stream: the chunk counter cleared, then one launch of at most
// `waves` wavefronts
static hipError_t launch_paths(pt_context* c, const FrameParams& fp, uint32_t n, const pt_Ray* dRays, pt_PathResult* dResults)
{
  const hipError_t e = hipMemsetAsync(c->dPathsChunk.p, 0, sizeof(uint32_t), c->stream);
  if(e != hipSuccess)
    return e;
  const uint32_t cap = c->pathsWaves > 0 ? uint32_t(c->pathsWaves) : PT_PATHS_WAVES, need = (n + TRACE_BLOCK - 1) / TRACE_BLOCK, grid = need < cap ? need : cap;
  if(c->scene.twoLevel)
    k_paths<true><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, fp, n, dRays, dResults, (uint32_t*)c->dPathsChunk.p, (Counters*)c->dCounters.p);
  else
    k_paths<false><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, fp, n, dRays, dResults, (uint32_t*)c->dPathsChunk.p, (Counters*)c->dCounters.p);
  c->renderedSinceCheck = true;  // the paths' walks count into the same counter as the frames' (check_traversal)
  return hipGetLastError();
}

// Everything a query through the path loop checks (pt_context.h: pt_gather calls this too), each refusal with its own text; then the kernel's
// parameters filled.  Nothing is allocated or launched.
int path_query_checks(pt_context* c, const char* who, const pt_RtxState* st, uint32_t flags, uint64_t n, const void* rays, const void* results, FrameParams& fp)
{
  if(!st)
    return c->fail(PT_ERR_INVALID, "%s: null state", who);
  if(flags & ~PT_RAYS_DEVICE)
    return c->fail(PT_ERR_INVALID, "%s: unknown flag bits 0x%x", who, flags & ~PT_RAYS_DEVICE);
  if(n > 0 && (!rays || !results))
    return c->fail(PT_ERR_INVALID, "%s: null", who);
  if(n > 0 && (flags & PT_RAYS_DEVICE) && ((uintptr_t(rays) | uintptr_t(results)) & 15u))
    return c->fail(PT_ERR_INVALID, "%s: device pointers must be 16-byte aligned", who);
  if(n > (uint64_t(1) << 40))
    return c->fail(PT_ERR_INVALID, "%s: n = %llu", who, (unsigned long long)n);
  if(st->maxDepth < 0 || st->maxDepth > PT_MAX_DEPTH)
    return c->fail(PT_ERR_INVALID, "%s: RtxState.maxDepth = %d (0 .. %d)", who, st->maxDepth, PT_MAX_DEPTH);
  if(st->maxSamples < 1 || st->maxSamples > PT_PATHS_MAX_SAMPLES)
    return c->fail(PT_ERR_INVALID, "%s: RtxState.maxSamples = %d (1 .. %d)", who, st->maxSamples, PT_PATHS_MAX_SAMPLES);
  if(st->pbrMode != 0 && st->pbrMode != 1)
    return c->fail(PT_ERR_INVALID, "%s: RtxState.pbrMode = %d (0: Disney, 1: glTF)", who, st->pbrMode);
  if(st->debugging_mode == PT_DEBUG_HEATMAP)
    return c->fail(PT_ERR_INVALID, "%s: RtxState.debugging_mode = PT_DEBUG_HEATMAP (the heat map is a frame's: it colours the time its kernels spent on a pixel)", who);
  if(!c->haveScene || !c->haveAccel)
    return c->fail(PT_ERR_STATE, "%s %s", who, c->no_accel());
  if(!c->haveEnv && c->scene.sunsky.in_use != 1)
    return c->fail(PT_ERR_STATE, "%s without an environment (pt_set_env) or sun & sky", who);
  if(!c->haveCamera)
    return c->fail(PT_ERR_STATE, "%s before pt_set_camera (its nbLights says how many lights the paths sample)", who);
  if(c->scene.camera.nbLights < 0 || uint32_t(c->scene.camera.nbLights) > c->numLights)  // pt_render_frame's rule
    return c->fail(PT_ERR_INVALID, "%s: camera.nbLights = %d but the scene holds %u lights", who, c->scene.camera.nbLights, c->numLights);
  std::memset(&fp, 0, sizeof(fp));
  fp.st      = *st;
  fp.batch   = 1;
  fp.variant = c->variant;
  return PT_OK;
}

// path_query_checks, then the chunk counter allocated.  Nothing is launched.
static int prepare_paths(pt_context* c, const char* who, const pt_RtxState* st, uint32_t flags, uint64_t n, const void* rays, const void* results, FrameParams& fp)
{
  STAGE_TRY(path_query_checks(c, who, st, flags, n, rays, results, fp));
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return dev_alloc(c, c->dPathsChunk, sizeof(uint32_t));
}

extern "C" {

int pt_trace_paths(pt_context* c, const pt_RtxState* state, uint32_t flags, uint64_t n, const pt_Ray* rays, pt_PathResult* results)
{
  CTX_CHECK(c);
  FrameParams fp;
  STAGE_TRY(prepare_paths(c, "pt_trace_paths", state, flags, n, rays, results, fp));
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, sync_all(c));  // the frames in flight first, like pt_trace_rays
  const bool device = (flags & PT_RAYS_DEVICE) != 0;
  // a piece: what one launch traces.  Host arrays: one staging buffer of rays and one of records (pt_trace_rays' buffers: the record sizes match);
  // device arrays: up to 2^30 rays in place
  const uint64_t piece = device ? uint64_t(1) << 30 : uint64_t(PT_QUERY_CHUNK);
  if(!device)
  {
    STAGE_TRY(dev_alloc(c, c->dQueryRays, sizeof(pt_Ray) * size_t(PT_QUERY_CHUNK)));
    STAGE_TRY(dev_alloc(c, c->dQueryHits, sizeof(pt_PathResult) * size_t(PT_QUERY_CHUNK)));
  }
  for(uint64_t at = 0; at < n; at += piece)
  {
    const uint32_t m        = uint32_t(n - at < piece ? n - at : piece);
    const pt_Ray*  dRays    = device ? rays + at : (const pt_Ray*)c->dQueryRays.p;
    pt_PathResult* dResults = device ? results + at : (pt_PathResult*)c->dQueryHits.p;
    if(!device)
      HIP_TRY(c, hipMemcpyAsync(c->dQueryRays.p, rays + at, sizeof(pt_Ray) * size_t(m), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_paths(c, fp, m, dRays, dResults));
    if(!device)
      HIP_TRY(c, hipMemcpyAsync(results + at, c->dQueryHits.p, sizeof(pt_PathResult) * size_t(m), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return check_traversal(c);
}

// Test access (not part of pt_api.h): caps the wavefronts of pt_trace_paths' launches, so that a small n makes every wavefront come back for more
// rays; 0 or negative restores the default.  Results do not depend on it.
__attribute__((visibility("default"))) int pt_debug_paths_waves(pt_context* c, int waves)
{
  CTX_CHECK(c);
  c->pathsWaves = waves > 0 ? waves : 0;
  return PT_OK;
}

// Measurement access (not part of pt_api.h; tools/paths_rate.py): pt_trace_paths' launch on device arrays (n <= 2^30) enqueued `reps` times between two
// events on the context's stream, after one untimed run -- milliseconds per run in *ms_out.  Synchronous.
__attribute__((visibility("default"))) int pt_debug_paths_time(pt_context* c, const pt_RtxState* state, uint64_t n, const pt_Ray* dRays, pt_PathResult* dResults, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!ms_out || reps < 1 || n < 1 || n > (uint64_t(1) << 30))
    return c->fail(PT_ERR_INVALID, "pt_debug_paths_time: null, reps < 1 or n outside 1 .. 2^30");
  FrameParams fp;
  STAGE_TRY(prepare_paths(c, "pt_debug_paths_time", state, PT_RAYS_DEVICE, n, dRays, dResults, fp));
  hipError_t first = hipSuccess;  // (launch_paths has taken the launch's error off the runtime: kept here for after the timing)
  const int  rc    = stage_time(c, "pt_debug_paths_time", reps, ms_out, [&] {
    const hipError_t e = launch_paths(c, fp, uint32_t(n), dRays, dResults);
    first              = first == hipSuccess ? e : first;
  });
  HIP_TRY(c, first);
  return rc;
}

}  // extern "C"
