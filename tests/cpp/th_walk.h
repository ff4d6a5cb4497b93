// What every entry point of the host harness that walks rays needs: a per-thread walk context, the parallel loop over rays, and the one machine
// leg of the harness -- the run loop and the service round of the persistent kernels for one lane.
#pragma once
#include "th_scene.h"

// per thread: the traversal stack in the kernels' layout (LDS part strided by TRACE_BLOCK + private spill array), the counters the walks add to,
// and the render buffers of the call with `counters` pointing at this thread's
struct WalkCtx {
  std::vector<uint32_t> stack, spill;
  Counters              cnt;
  RenderBuffers         rb;
  explicit WalkCtx(const RenderBuffers* proto) : stack(size_t(STACK_LDS) * TRACE_BLOCK), spill(STACK_SPILL)
  {
    std::memset(&cnt, 0, sizeof(cnt));
    if(proto)
      rb = *proto;
    else
      std::memset(&rb, 0, sizeof(rb));
    rb.counters = &cnt;
  }
};

// body(ctx, r) for every r in [0, n) in parallel (rays are independent: the schedule does not matter); returns the traversal-stack overflows summed
template <class Body>
uint32_t for_each_ray(long long n, int chunk, const RenderBuffers* proto, Body body)
{
  uint32_t overflow = 0;
#pragma omp parallel
  {
    WalkCtx ctx(proto);
#pragma omp for schedule(dynamic, chunk)
    for(long long r = 0; r < n; ++r)
      body(ctx, r);
    TH_AFTER_RAYS();
#pragma omp critical
    overflow += ctx.cnt.stackOverflow;
  }
  return overflow;
}

// The verdict of drive_lane: settled -- the lane's best hit (L.bslot, L.bw, L.bt, L.bu, L.bv) stands, nDraw draws were consumed and s2 is the RNG
// state after them -- or the ray needs the exact key-ordered loop, with its seed untouched.
struct LaneVerdict {
  bool               settled;
  uint32_t           nDraw, s2;
  unsigned long long innerSteps, leafSteps;  // node / triangle steps of the walk
  int                maxSp;                  // deepest traversal-stack level it used
};

// The run loop and the service round of k_closest_p / k_shadow_p / k_trace_p for one lane that has been begun (lane_fetch_*; `seed`: what the fetch
// returned).  What the service round decides -- pass A -> pass B transition, the draws, hand-over to the exact loop -- is the settle rule of
// pt_trace.h, needs_count_pass and settle_draws: the very functions the kernels call.  What is done with the verdict is the caller's.
template <bool TWO>
LaneVerdict drive_lane(const DeviceScene& S, TraceLane& L, uint32_t seed, WalkCtx& c)
{
  LaneVerdict v{false, 0u, seed, 0ull, 0ull, 0};
  for(;;)
  {
    while(!L.done)
    {
      if(!(L.cur & BVH_LEAF))
      {
        ++v.innerSteps;
        lane_inner<false, TWO>(S, L, c.stack.data(), c.spill.data(), &c.cnt);
        v.maxSp = L.sp > v.maxSp ? L.sp : v.maxSp;
      }
      if(!L.done && (L.cur & BVH_LEAF))
      {
        ++v.leafSteps;
        lane_leaf<false, TWO>(S, L, c.stack.data(), c.spill.data());
      }
    }
    if(needs_count_pass(L.flags, L.pass, L.bslot, L.bt, L.zeroMaxT, L.zeroMaxT2, L.zeroMaxT3, L.cnt))
    {
      lane_begin_count<TWO>(L);
      continue;
    }
    v.settled = !(L.flags & TF_SAW_FRAC) && settle_draws(L.bslot, L.bw, L.cnt, seed, v.nDraw, v.s2);
    return v;
  }
}
