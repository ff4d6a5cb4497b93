// pt_trace_rays (include/pt_api.h): caller rays through the trace contract, one ray per lane.  The per-ray body is pt_query.h; this unit holds
// its kernel, the launch and the entry point with its staging.  No existing kernel is involved: the query kernels walk the structures the frames
// walk, with the functions the frames' kernels are made of.
#include "pt_context.h"
#include "pt_query.h"

// as k_closest_x (pt_render.hip): 5 waves per SIMD on the flat structure, 4 on the two-level one (object-space ray constants + instance context)
#define PT_QUERY_WAVES 5
#define PT_QUERY_WAVES_TWO 4

// rays / hits are 16-byte aligned (pt_trace_rays checks the caller's device pointers; the staging buffers are allocations)
template <bool TWO>
__global__ void __launch_bounds__(TRACE_BLOCK, TWO ? PT_QUERY_WAVES_TWO : PT_QUERY_WAVES)
    k_query(DeviceScene S, int kind, int variant, uint32_t n, const pt_Ray* __restrict__ rays, pt_RayHit* __restrict__ hits, uint32_t hitsPerRay, Counters* counters)
{
  __shared__ uint32_t stack[STACK_LDS * TRACE_BLOCK];
  const uint32_t      i = blockIdx.x * TRACE_BLOCK + threadIdx.x;
  if(i >= n)
    return;
  const float4* rp = reinterpret_cast<const float4*>(rays + i);
  const float4  a = rp[0], b = rp[1];
  pt_Ray        ray;
  ray.origin[0] = a.x; ray.origin[1] = a.y; ray.origin[2] = a.z; ray.tmax = a.w;
  ray.direction[0] = b.x; ray.direction[1] = b.y; ray.direction[2] = b.z; ray.seed = __float_as_uint(b.w);
  query_ray<TWO>(S, kind, variant, ray, hitsPerRay, stack + threadIdx.x, counters, hits + size_t(i) * hitsPerRay);
}

// n rays (at most 2^30 per launch: the caller cuts longer arrays), grid = ceil(n / 64)
static void pt_launch_query(hipStream_t stream, const DeviceScene& scene, int kind, int variant, uint32_t n, const pt_Ray* dRays, pt_RayHit* dHits, uint32_t hitsPerRay, Counters* counters)
{
  const uint32_t grid = (n + TRACE_BLOCK - 1) / TRACE_BLOCK;
  if(scene.twoLevel)
    k_query<true><<<grid, TRACE_BLOCK, 0, stream>>>(scene, kind, variant, n, dRays, dHits, hitsPerRay, counters);
  else
    k_query<false><<<grid, TRACE_BLOCK, 0, stream>>>(scene, kind, variant, n, dRays, dHits, hitsPerRay, counters);
}

extern "C" int pt_trace_rays(pt_context* c, int kind, uint32_t flags, uint64_t n, const pt_Ray* rays, pt_RayHit* hits, uint32_t hits_per_ray)
{
  CTX_CHECK(c);
  if(kind < PT_RAYS_CLOSEST || kind > PT_RAYS_CANDIDATES)
    return c->fail(PT_ERR_INVALID, "pt_trace_rays: unknown kind %d", kind);
  if(flags & ~PT_RAYS_DEVICE)
    return c->fail(PT_ERR_INVALID, "pt_trace_rays: unknown flag bits 0x%x", flags & ~PT_RAYS_DEVICE);
  if(hits_per_ray < 1 || hits_per_ray > (kind == PT_RAYS_CANDIDATES ? PT_RAYS_MAX_HITS : 1u))
    return c->fail(PT_ERR_INVALID, "pt_trace_rays: hits_per_ray = %u (1 .. %u for PT_RAYS_CANDIDATES, 1 for every other kind)", hits_per_ray, PT_RAYS_MAX_HITS);
  if(n > 0 && (!rays || !hits))
    return c->fail(PT_ERR_INVALID, "pt_trace_rays: null");
  const bool device = (flags & PT_RAYS_DEVICE) != 0;
  if(n > 0 && device && ((uintptr_t(rays) | uintptr_t(hits)) & 15u))
    return c->fail(PT_ERR_INVALID, "pt_trace_rays: device pointers must be 16-byte aligned");
  if(n > (uint64_t(1) << 40))
    return c->fail(PT_ERR_INVALID, "pt_trace_rays: n = %llu", (unsigned long long)n);
  if(!c->haveScene || !c->haveAccel)
    return c->fail(PT_ERR_STATE, "pt_trace_rays %s", c->no_accel());
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));  // the frames in flight first, like pt_pick
  // a piece: what one launch traces.  Host arrays: as many rays as fill one staging buffer with results; device arrays: up to 2^30 rays in place
  const uint64_t piece = device ? (uint64_t(1) << 30) / hits_per_ray : PT_QUERY_CHUNK / hits_per_ray;
  if(!device)
  {
    int rc;
    if((rc = dev_alloc(c, c->dQueryRays, sizeof(pt_Ray) * size_t(PT_QUERY_CHUNK))) != PT_OK || (rc = dev_alloc(c, c->dQueryHits, sizeof(pt_RayHit) * size_t(PT_QUERY_CHUNK))) != PT_OK)
      return rc;
  }
  for(uint64_t at = 0; at < n; at += piece)
  {
    const uint32_t   m     = uint32_t(n - at < piece ? n - at : piece);
    const pt_Ray*    dRays = device ? rays + at : (const pt_Ray*)c->dQueryRays.p;
    pt_RayHit*       dHits = device ? hits + at * hits_per_ray : (pt_RayHit*)c->dQueryHits.p;
    if(!device)
      HIP_TRY(c, hipMemcpyAsync(c->dQueryRays.p, rays + at, sizeof(pt_Ray) * size_t(m), hipMemcpyHostToDevice, c->stream));
    pt_launch_query(c->stream, c->scene, kind, c->variant, m, dRays, dHits, hits_per_ray, (Counters*)c->dCounters.p);
    c->renderedSinceCheck = true;  // the rays' own walks count into the same counter (check_traversal)
    HIP_TRY(c, hipGetLastError());
    if(!device)
      HIP_TRY(c, hipMemcpyAsync(hits + at * hits_per_ray, c->dQueryHits.p, sizeof(pt_RayHit) * size_t(m) * hits_per_ray, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return check_traversal(c);
}
