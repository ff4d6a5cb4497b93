// CPU harness around the product's ray-query body (test infrastructure; built and used by tests/test_query_host.py and, as the reference of the
// device runs, by tests/test_query_gpu.py).  vk_raytrace_amd/csrc/pt_query.h -- query_ray<TWO>, what pt_trace_rays' kernel runs per lane -- is
// compiled for the host next to the harness of the traversal source (trace_host.cpp: its Scene, th_create*, th_candidates, th_settle), on the
// structures that harness assembles.
#include "trace_host.cpp"
#include "pt_query.h"

// n rays of `kind` on the flat (two = 0) or the two-level structure; hits: n x hitsPerRay records.  Returns the traversal-stack overflows counted.
extern "C" uint32_t qh_query(void* p, int two, int kind, int variant, uint64_t n, const pt_Ray* rays, pt_RayHit* hits, uint32_t hitsPerRay)
{
  Scene*             s = static_cast<Scene*>(p);
  const DeviceScene& S = two ? s->dsTwo : s->dsFlat;
  uint32_t           overflow = 0;
#pragma omp parallel
  {
    std::vector<uint32_t> stack(size_t(STACK_LDS) * TRACE_BLOCK);
    Counters              cnt;
    std::memset(&cnt, 0, sizeof(cnt));
#pragma omp for schedule(dynamic, 64)
    for(long long r = 0; r < (long long)n; ++r)
    {
      if(two)
        query_ray<true>(S, kind, variant, rays[r], hitsPerRay, stack.data(), &cnt, hits + size_t(r) * hitsPerRay);
      else
        query_ray<false>(S, kind, variant, rays[r], hitsPerRay, stack.data(), &cnt, hits + size_t(r) * hitsPerRay);
    }
#pragma omp critical
    overflow += cnt.stackOverflow;
  }
  return overflow;
}
