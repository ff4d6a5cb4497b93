// The hand-over of a packet's pass A to the trace machine (csrc/pt_settle.h store_handover, csrc/pt_machine.h lane_fetch_handover) on the CPU:
// one entry point of the host harness (tests/host_harness.py), on the scenes th_create_scene makes, with the machine leg of th_walk.h.
//
// For every ray two routes are run on the same scene and the same seed:
//   (a) the lane starts at the root (lane_fetch_closest) and is driven through the service round of k_closest_p to its end (drive_lane);
//   (b) pass A comes from traverse<TM_CLOSEST> (what the packet kernel holds per lane when its traversal ends), k_closest_k's decision is taken
//       on it, and a ray that needs the count pass is stored with store_handover, begun with lane_fetch_handover and driven by the same drive_lane.
// A ray either route cannot settle goes through settle_closest_exact, like k_closest_x.  tests/test_handover_host.py requires both routes to
// leave the same hit record, the same RNG state, the same number of draws and to have taken the same way (settled / exact loop).
#include "th_walk.h"

namespace {
struct RouteOut {
  uint32_t hit[4], seed, draws, exact;
};
// the lane's verdict as k_closest_p acts on it (pt_render.hip closest_machine): the hit record and the seed go to the path state
template <bool TWO>
void drive_and_store(const DeviceScene& S, TraceLane& L, uint32_t seed, WalkCtx& c, RouteOut& out)
{
  const LaneVerdict v = drive_lane<TWO>(S, L, seed, c);
  if(v.settled)
  {
    store_hit(c.rb, 0u, L.bslot, L.bw, TWO, L.bt, L.bu, L.bv);
    if(v.nDraw)
      c.rb.ps.rayD[0].w = __uint_as_float(v.s2);
    out.draws = v.nDraw;
  }
  out.exact = v.settled ? 0u : 1u;
}
template <bool TWO>
void finish(const DeviceScene& S, const RenderBuffers& rb, uint32_t r, f3 o, f3 d, uint32_t seed0, uint32_t* stack, RouteOut& out)
{
  if(out.exact)
  {  // k_closest_x: the ray and the untouched seed from the path state
    uint32_t nAlpha = 0;
    settle_closest_exact<TWO>(S, rb, r, o, d, seed0, stack, nAlpha);
    out.draws = nAlpha;
  }
  const float4 h = rb.ps.hit[r];
  out.hit[0] = __float_as_uint(h.x); out.hit[1] = __float_as_uint(h.y); out.hit[2] = __float_as_uint(h.z); out.hit[3] = __float_as_uint(h.w);
  out.seed   = __float_as_uint(rb.ps.rayD[r].w);
}


template <bool TWO>
uint32_t handover_rays(Scene* s, uint32_t nrays, const float* org, const float* dir, const uint32_t* seeds, uint32_t* outA, uint32_t* outB, uint32_t* info)
{
  const DeviceScene&    S = TWO ? s->dsTwo : s->dsFlat;
  std::vector<float4>   rayO(1), rayD(1), hit(1);  // one path slot, used by every ray in turn
  RenderBuffers         proto;
  std::memset(&proto, 0, sizeof(proto));
  proto.ps.rayO.p = rayO.data(); proto.ps.rayD.p = rayD.data(); proto.ps.hit.p = hit.data();
  WalkCtx              ctx(&proto);
  const RenderBuffers& rb    = ctx.rb;
  uint32_t* const      stack = ctx.stack.data();
  for(uint32_t r = 0; r < nrays; ++r)
  {
    const f3 o = f3{org[3 * r], org[3 * r + 1], org[3 * r + 2]}, d = f3{dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    auto     reset = [&]() {
      rayO[0] = make_float4(o.x, o.y, o.z, 0.f);
      rayD[0] = make_float4(d.x, d.y, d.z, __uint_as_float(seeds[r]));
      hit[0]  = make_float4(-1.f, -1.f, -1.f, -1.f);
    };
    // ---- (a) from the root
    RouteOut a{};
    {
      reset();
      TraceLane L;
      uint32_t  seed = 0;
      lane_fetch_closest(S, rb, 0u, L, seed);
      drive_and_store<TWO>(S, L, seed, ctx, a);
      finish<TWO>(S, rb, 0u, o, d, seeds[r], stack, a);
    }
    // ---- (b) pass A as the packet kernel holds it, k_closest_k's decision, the hand-over
    RouteOut b{};
    RayHit   h;
    bool     dummy, handed = false;
    {
      reset();
      traverse<TM_CLOSEST, TWO>(S, o, d, PT_INFINITY, 0.0f, 0xffffffffu, 0u, stack, h, dummy, &ctx.cnt);
      uint32_t   count     = h.count;
      const bool frac      = (h.flags & TF_SAW_FRAC) != 0;
      const bool countPass = needs_count_pass(h.flags, 0, h.slot, h.t, h.zeroMaxT, h.zeroMaxT2, h.zeroMaxT3, count);
      if(!frac && !countPass)
      {
        uint32_t nDraw, s2;
        if(settle_draws(h.slot, h.w, count, seeds[r], nDraw, s2))
        {
          store_hit(rb, 0u, h.slot, h.w, TWO, h.t, h.u, h.v);
          if(nDraw)
            rayD[0].w = __uint_as_float(s2);
          b.draws = nDraw;
        }
        else
          b.exact = 1u;
      }
      else if(countPass)
      {
        handed = true;
        store_handover(rb, 0u, h, TWO);
        TraceLane L;
        uint32_t  seed = 0;
        lane_fetch_handover<TWO>(S, rb, 0u, L, seed);
        drive_and_store<TWO>(S, L, seed, ctx, b);
      }
      else
        b.exact = 1u;
      finish<TWO>(S, rb, 0u, o, d, seeds[r], stack, b);
    }
    // ---- what the fixture holds: pass A's view of the ray, and the count pass in front of its hit run for every ray
    RayHit c;
    traverse<TM_COUNT, TWO>(S, o, d, h.slot == BVH_NONE ? PT_INFINITY : h.t, 0.0f, 0xffffffffu, h.slot == BVH_NONE ? 0u : (h.w & TRI_INDEX_MASK), stack, c, dummy, &ctx.cnt);
    std::memcpy(outA + 7 * size_t(r), &a, sizeof(a));
    std::memcpy(outB + 7 * size_t(r), &b, sizeof(b));
    uint32_t* I = info + 9 * size_t(r);
    I[0] = h.flags; I[1] = h.count; I[2] = __float_as_uint(h.zeroMaxT); I[3] = __float_as_uint(h.zeroMaxT2); I[4] = __float_as_uint(h.zeroMaxT3);
    I[5] = __float_as_uint(h.t); I[6] = h.slot == BVH_NONE ? 0xffffffffu : (h.w >> 29); I[7] = c.flags; I[8] = handed ? 1u : 0u;
  }
  return ctx.cnt.stackOverflow;
}
}  // namespace

static_assert(sizeof(RouteOut) == 7 * sizeof(uint32_t), "seven words per route");

// outA / outB: 7 words per ray (hit record x 4, RNG state afterwards, draws, 1 = the exact loop settled it); info: 9 words per ray -- pass A's flags, count,
// zeroMaxT .. zeroMaxT3, t, the hit triangle's flag bits (0xffffffff: miss), the flags of the count pass in front of the hit, 1 = route (b) handed the ray over.
// Returns the number of traversal-stack overflows.
extern "C" uint32_t th_handover(void* p, int two, uint32_t nrays, const float* org, const float* dir, const uint32_t* seeds, uint32_t* outA, uint32_t* outB, uint32_t* info)
{
  Scene* s = static_cast<Scene*>(p);
  return two ? handover_rays<true>(s, nrays, org, dir, seeds, outA, outB, info) : handover_rays<false>(s, nrays, org, dir, seeds, outA, outB, info);
}
