// pt_gather (include/pt_api.h): irradiance at caller points and spherical-harmonic probes, one point per lane.  The
// per-point body is pt_gather.h; this unit holds its kernel, the launch and the entry point with its staging.  No existing kernel is involved, and
// the checks are pt_trace_paths' (path_query_checks, pt_paths.hip).
#include "pt_stage.h"    // stage_time
#include "pt_machine.h"  // supply_next
#include "pt_gather.h"

// wavefronts of a launch unless pt_debug_gather_waves says otherwise: k_paths' (pt_paths.hip), 2 per SIMD on 256 CUs
#define PT_GATHER_WAVES 2048u

// k_paths' shape (pt_paths.hip): persistent wavefronts, one point per lane carried bounce by bounce (gather_step) through all its samples -- the
// seed chains through draws and paths -- and a lane whose point is finished takes the next index from the supply while its neighbours go on.  A
// point's record does not depend on which lane ran it: the lane's own state and, for PT_GATHER_SPHERE, the point's own record (the 27 sums live
// there between samples; written and read by this lane alone, so program order is all the ordering they need) are everything it reads.
// points / results are 16-byte aligned (pt_gather checks the caller's device pointers; the staging buffers are allocations); a record is
// ROWS float4: 2 (pt_GatherResult) or 8 (pt_ProbeResult).  (Not to be confused with pt_accel.hip's k_gather, the builder's non-template kernel that
// puts triangle records in leaf order (another signature, another symbol), or with the context's dGather, the image gather's buffer: this query's members are dPointsChunk / pointsWaves.)
template <bool TWO, uint32_t KIND>
__global__ void __launch_bounds__(TRACE_BLOCK, 2)
    k_gather(DeviceScene S, FrameParams fp, uint32_t n, const pt_GatherPoint* __restrict__ points, float4* results, uint32_t* chunkCounter, Counters* counters)
{
  constexpr uint32_t ROWS = KIND == PT_GATHER_HEMISPHERE ? 2u : 8u;
  __shared__ uint32_t stack[STACK_LDS * TRACE_BLOCK];
  uint32_t* lds = stack + threadIdx.x;
  RaySupply rs;
  rs.chunk       = 64;
  GatherLane G;
  float4*  rec   = results;
  bool     alive = false;
#pragma unroll 1
  for(;;)
  {
    const uint32_t qi = supply_next(rs, chunkCounter, n, !alive);
    if(qi != 0xffffffffu)  // (qi < n: supply_next hands out indices below `count` only)
    {
      rec              = results + size_t(qi) * ROWS;
      const float4* pp = reinterpret_cast<const float4*>(points + qi);
      const float4  a = pp[0], b = pp[1];
      pt_GatherPoint pt;
      pt.position[0] = a.x; pt.position[1] = a.y; pt.position[2] = a.z; pt.seed = __float_as_uint(a.w);
      pt.normal[0] = b.x; pt.normal[1] = b.y; pt.normal[2] = b.z; pt._pad = 0u;
      alive = gather_begin<KIND>(fp, pt, G, rec);  // (an invalid point's record is written there; the lane asks again in the next round)
    }
    // nobody has a point: either the supply has run dry, or every point just handed out was invalid -- then the next round asks again
    if(!__ballot(alive) && !rs.more)
      break;
    if(alive && gather_step<TWO, KIND>(S, fp, fp.variant, G, rec, lds, counters))
    {
      gather_end<KIND>(fp, G, rec);
      alive = false;
    }
  }
}

// n points (at most 2^30 / 2^28 per launch: the record index times ROWS stays below 2^32 either way, and is widened before use) on the context's
// stream: the chunk counter cleared, then one launch of at most `waves` wavefronts
static hipError_t launch_gather(pt_context* c, const FrameParams& fp, uint32_t kind, uint32_t n, const pt_GatherPoint* dPoints, void* dResults)
{
  const hipError_t e = hipMemsetAsync(c->dPointsChunk.p, 0, sizeof(uint32_t), c->stream);
  if(e != hipSuccess)
    return e;
  const uint32_t cap = c->pointsWaves > 0 ? uint32_t(c->pointsWaves) : PT_GATHER_WAVES, need = (n + TRACE_BLOCK - 1) / TRACE_BLOCK, grid = need < cap ? need : cap;
  uint32_t* chunk    = (uint32_t*)c->dPointsChunk.p;
  Counters* counters = (Counters*)c->dCounters.p;
  float4*   out      = (float4*)dResults;
  const bool two     = c->scene.twoLevel;
  if(kind == PT_GATHER_HEMISPHERE)
  {
    if(two)
      k_gather<true, PT_GATHER_HEMISPHERE><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, fp, n, dPoints, out, chunk, counters);
    else
      k_gather<false, PT_GATHER_HEMISPHERE><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, fp, n, dPoints, out, chunk, counters);
  }
  else
  {
    if(two)
      k_gather<true, PT_GATHER_SPHERE><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, fp, n, dPoints, out, chunk, counters);
    else
      k_gather<false, PT_GATHER_SPHERE><<<grid, TRACE_BLOCK, 0, c->stream>>>(c->scene, fp, n, dPoints, out, chunk, counters);
  }
  c->renderedSinceCheck = true;  // the walks count into the same counter as the frames' (check_traversal)
  return hipGetLastError();
}

// pt_trace_paths' checks and the kind's; then the chunk counter allocated and the kernel's parameters filled.  Nothing is launched.
static int prepare_gather(pt_context* c, const char* who, const pt_RtxState* st, uint32_t kind, uint32_t flags, uint64_t n, const void* points, const void* results, FrameParams& fp)
{
  if(kind != PT_GATHER_HEMISPHERE && kind != PT_GATHER_SPHERE)
    return c->fail(PT_ERR_INVALID, "%s: unknown kind %u (PT_GATHER_HEMISPHERE, PT_GATHER_SPHERE)", who, kind);
  STAGE_TRY(path_query_checks(c, who, st, flags, n, points, results, fp));
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return dev_alloc(c, c->dPointsChunk, sizeof(uint32_t));
}

static size_t gather_record_bytes(uint32_t kind) { return kind == PT_GATHER_HEMISPHERE ? sizeof(pt_GatherResult) : sizeof(pt_ProbeResult); }

extern "C" {

int pt_gather(pt_context* c, const pt_RtxState* state, uint32_t kind, uint32_t flags, uint64_t n, const pt_GatherPoint* points, void* results)
{
  CTX_CHECK(c);
  FrameParams fp;
  STAGE_TRY(prepare_gather(c, "pt_gather", state, kind, flags, n, points, results, fp));
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, sync_all(c));  // the frames in flight first, like pt_trace_paths
  const bool   device = (flags & PT_RAYS_DEVICE) != 0;
  const size_t recb   = gather_record_bytes(kind);
  // a piece: what one launch gathers.  Host arrays: what fits pt_trace_rays' staging buffer of results (32 MB: PT_QUERY_CHUNK 32-byte records, a
  // quarter as many 128-byte ones); device arrays: up to 2^28 points in place
  const uint64_t piece = device ? uint64_t(1) << 28 : uint64_t(PT_QUERY_CHUNK) * sizeof(pt_RayHit) / recb;
  if(!device)
  {
    STAGE_TRY(dev_alloc(c, c->dQueryRays, sizeof(pt_Ray) * size_t(PT_QUERY_CHUNK)));
    STAGE_TRY(dev_alloc(c, c->dQueryHits, sizeof(pt_RayHit) * size_t(PT_QUERY_CHUNK)));
  }
  for(uint64_t at = 0; at < n; at += piece)
  {
    const uint32_t        m        = uint32_t(n - at < piece ? n - at : piece);
    const pt_GatherPoint* dPoints  = device ? points + at : (const pt_GatherPoint*)c->dQueryRays.p;
    void*                 hResults = (char*)results + at * recb;
    void*                 dResults = device ? hResults : c->dQueryHits.p;
    if(!device)
      HIP_TRY(c, hipMemcpyAsync(c->dQueryRays.p, points + at, sizeof(pt_GatherPoint) * size_t(m), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_gather(c, fp, kind, m, dPoints, dResults));
    if(!device)
      HIP_TRY(c, hipMemcpyAsync(hResults, c->dQueryHits.p, recb * size_t(m), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return check_traversal(c);
}

// Test access (not part of pt_api.h): caps the wavefronts of pt_gather's launches, so that a small n makes every wavefront come back for more
// points; 0 or negative restores the default.  Results do not depend on it.
__attribute__((visibility("default"))) int pt_debug_gather_waves(pt_context* c, int waves)
{
  CTX_CHECK(c);
  c->pointsWaves = waves > 0 ? waves : 0;
  return PT_OK;
}

// Measurement access (not part of pt_api.h; tools/gather_rate.py): pt_gather's launch on device arrays (n <= 2^28) enqueued `reps` times between two
// events on the context's stream, after one untimed run -- milliseconds per run in *ms_out.  Synchronous.
__attribute__((visibility("default"))) int pt_debug_gather_time(pt_context* c, const pt_RtxState* state, uint32_t kind, uint64_t n, const pt_GatherPoint* dPoints, void* dResults, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!ms_out || reps < 1 || n < 1 || n > (uint64_t(1) << 28))
    return c->fail(PT_ERR_INVALID, "pt_debug_gather_time: null, reps < 1 or n outside 1 .. 2^28");
  FrameParams fp;
  STAGE_TRY(prepare_gather(c, "pt_debug_gather_time", state, kind, PT_RAYS_DEVICE, n, dPoints, dResults, fp));
  hipError_t first = hipSuccess;  // (launch_gather has taken the launch's error off the runtime: kept here for after the timing)
  const int  rc    = stage_time(c, "pt_debug_gather_time", reps, ms_out, [&] {
    const hipError_t e = launch_gather(c, fp, kind, uint32_t(n), dPoints, dResults);
    first              = first == hipSuccess ? e : first;
  });
  HIP_TRY(c, first);
  return rc;
}

}  // extern "C"
