// The product's ray-query body on the host (unit of the host harness, tests/host_harness.py; the reference of tests/test_query_host.py and, for the
// device runs, of tests/test_query_gpu.py).  vk_raytrace_amd/csrc/pt_query.h -- query_ray<TWO>, what pt_trace_rays' kernel runs per lane -- on the
// structures th_scene.h assembles.
#include "th_walk.h"
#include "pt_query.h"

// n rays of `kind` on the flat (two = 0) or the two-level structure; hits: n x hitsPerRay records.  Returns the traversal-stack overflows counted.
extern "C" uint32_t qh_query(void* p, int two, int kind, int variant, uint64_t n, const pt_Ray* rays, pt_RayHit* hits, uint32_t hitsPerRay)
{
  Scene*             s = static_cast<Scene*>(p);
  const DeviceScene& S = two ? s->dsTwo : s->dsFlat;
  return for_each_ray((long long)n, 64, nullptr, [&](WalkCtx& c, long long r) {
    if(two)
      query_ray<true>(S, kind, variant, rays[r], hitsPerRay, c.stack.data(), &c.cnt, hits + size_t(r) * hitsPerRay);
    else
      query_ray<false>(S, kind, variant, rays[r], hitsPerRay, c.stack.data(), &c.cnt, hits + size_t(r) * hitsPerRay);
  });
}
