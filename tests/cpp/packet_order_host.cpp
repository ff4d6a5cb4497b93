// The packet stage's child order on the CPU (tests/test_packet_order.py): the encoding of csrc/pt_order.h as the collapse kernel runs it, and a plain
// model of the 64-ray packet walk of csrc/pt_packet.h (traverse_packet<false>: one traversal for all lanes, a wave-level stack, the per-lane slab
// tests, triangle test and candidate rules of the product's own headers) with the ORDER POLICY as a parameter, on the scenes th_create_scene makes.
// A library of its own next to trace_host.cpp (which owns the scenes); th_scene.h and th_walk.h are included as they are.
//
// For every ray of a packet two routes are run on the same scene and seed:
//   (a) the lane starts at the root (lane_fetch_closest) and is driven through the service round of k_closest_p to its end (drive_lane);
//   (b) pass A comes from the packet model under the given policy, k_closest_k's decision is taken on it: settled on the spot, handed over to the
//       count pass (store_handover, lane_fetch_handover, drive_lane) or sent to the exact loop.
// A ray either route cannot settle goes through settle_closest_exact, like k_closest_x.  The test requires both routes to leave the same hit record
// and the same RNG state under every policy.
#include "th_walk.h"
#include "pt_order.h"

namespace {
enum Policy { PO_SORTED = 0, PO_TABLE = 1, PO_SLOTS = 2, PO_REVERSED = 3 };
constexpr int LANES = 64;

struct WalkStats {
  unsigned long long inner = 0, leaf = 0, packets = 0, incoherent = 0;
};

// false: the lanes disagree on a direction sign (nothing was traversed).  wide: the flat structure's nodes with the order tables written.
bool packet_walk(const DeviceScene& S, const WideNode* wide, int n, const f3* o, const f3* d, int policy, RayHit* best, WalkStats& st)
{
  RayBox rb[LANES];
  int    neg[3] = {0, 0, 0};
  for(int l = 0; l < n; ++l)
  {
    rb[l] = make_raybox(o[l], d[l]);
    neg[0] += rb[l].idir.x < 0.0f; neg[1] += rb[l].idir.y < 0.0f; neg[2] += rb[l].idir.z < 0.0f;
  }
  for(int a = 0; a < 3; ++a)
    if(neg[a] != 0 && neg[a] != n)
      return false;
  for(int l = 0; l < n; ++l)
  {
    RayHit& b = best[l];
    b.slot = BVH_NONE; b.t = PT_INFINITY; b.w = 0xffffffffu; b.flags = 0; b.count = 0;
    b.zeroMaxT = b.zeroMaxT2 = b.zeroMaxT3 = -1.0f;
    b.u = b.v = 0.0f;
  }
  if(S.numTris == 0 || n == 0)
    return true;
  const uint32_t off[3] = {neg[0] ? 12u : 0u, neg[1] ? 12u : 0u, neg[2] ? 12u : 0u};  // in floats: near planes at +off, far planes at +12 - off
  const uint32_t oct    = (neg[0] ? 1u : 0u) | (neg[1] ? 2u : 0u) | (neg[2] ? 4u : 0u);
  std::vector<uint32_t> stack;
  uint32_t              cur = 0;
  for(;;)
  {
    if(!(cur & BVH_LEAF))
    {
      ++st.inner;
      const WideNode& w    = wide[cur & BVH_SLOT_MASK];
      const float*    base = reinterpret_cast<const float*>(&w);
      const uint32_t  cc[4] = {w.child[0].x, w.child[0].y, w.child[0].z, w.child[0].w};
      bool            hit[4];
      float           first[4];  // entry distance of the first lane that hits the child (the sorted visit's key)
      for(int k = 0; k < 4; ++k)
      {
        const float px = base[off[0] + k], qx = base[12 - off[0] + k], py = base[4 + off[1] + k], qy = base[16 - off[1] + k], pz = base[8 + off[2] + k], qz = base[20 - off[2] + k];
        hit[k]   = false;
        first[k] = 0.f;
        for(int l = 0; l < n && cc[k] != BVH_NONE; ++l)
        {
          const float nr = fmaxf(fmaxf(__builtin_fmaf(px, rb[l].idir.x, rb[l].nlo.x), __builtin_fmaf(py, rb[l].idir.y, rb[l].nlo.y)), fmaxf(__builtin_fmaf(pz, rb[l].idir.z, rb[l].nlo.z), 0.0f)) * 0.9999996f;
          const float fr = fminf(fminf(__builtin_fmaf(qx, rb[l].idir.x, rb[l].nhi.x), __builtin_fmaf(qy, rb[l].idir.y, rb[l].nhi.y)), fminf(__builtin_fmaf(qz, rb[l].idir.z, rb[l].nhi.z), best[l].t)) * 1.0000004f;
          if(nr <= fr)
          {
            if(!hit[k])
              first[k] = nr;
            hit[k] = true;
          }
        }
      }
      uint32_t cid[4];
      int      nh = 0;
      if(policy == PO_SORTED)
      {
        float key[4];
        for(int k = 0; k < 4; ++k)
          if(hit[k])
          {
            key[nh] = first[k]; cid[nh] = cc[k]; ++nh;
          }
        for(int i = 1; i < nh; ++i)
          for(int j = i; j > 0 && key[j] < key[j - 1]; --j)
          {
            std::swap(key[j], key[j - 1]);
            std::swap(cid[j], cid[j - 1]);
          }
      }
      else
      {
        const uint32_t byte = policy == PO_SLOTS ? pt_order_byte(0u, 0u, oct) : pt_order_byte(w.pad[0].x, w.pad[0].y, oct);
        for(int i = 0; i < 4; ++i)
        {
          const uint32_t s = (byte >> (2 * (policy == PO_REVERSED ? 3 - i : i))) & 3u;
          if(hit[s])
            cid[nh++] = cc[s];
        }
      }
      if(nh)
      {
        for(int i = nh - 1; i >= 1; --i)
          stack.push_back(cid[i]);
        cur = cid[0];
        continue;
      }
    }
    else
    {
      ++st.leaf;
      const uint32_t slot = cur & BVH_SLOT_MASK;
      const TriRec   tr   = S.tris[slot];
      const uint32_t wbits = __float_as_uint(tr.p0w.w);
      const uint32_t flags = wbits >> 29;
      const bool     opq   = (flags & TRI_OPAQUE) != 0;
      for(int l = 0; l < n; ++l)
      {
        RayHit& b = best[l];
        float   t, u, v;
        if(tri_test(tr, flags, o[l], d[l], t, u, v) && t > 0.0f && t < PT_INFINITY)
        {
          const uint32_t wi = wbits & TRI_INDEX_MASK;
          if(b.slot == BVH_NONE || key_less(t, wi, b.t, b.w & TRI_INDEX_MASK))
          {
            bool certain = opq;
            if(!opq)
            {
              const float op = opacity_class(S, S.alphaRecs[slot], u, v);
              certain        = op >= 1.0f;
              if(!certain)
              {
                b.flags |= (op <= 0.0f) ? TF_SAW_ZERO : TF_SAW_FRAC;
                if(op <= 0.0f)
                {
                  b.count++;
                  note_zero_candidate(t, b.zeroMaxT, b.zeroMaxT2, b.zeroMaxT3);
                }
              }
            }
            if(certain)
            {
              b.t = t; b.u = u; b.v = v; b.slot = slot; b.w = wbits;
            }
          }
        }
      }
    }
    if(stack.empty())
      break;
    cur = stack.back();
    stack.pop_back();
  }
  return true;
}

struct RouteOut {
  uint32_t hit[4], seed, draws, exact;
};
void drive_and_store(const DeviceScene& S, TraceLane& L, uint32_t seed, WalkCtx& c, RouteOut& out)
{
  const LaneVerdict v = drive_lane<false>(S, L, seed, c);
  if(v.settled)
  {
    store_hit(c.rb, 0u, L.bslot, L.bw, false, L.bt, L.bu, L.bv);
    if(v.nDraw)
      c.rb.ps.rayD[0].w = __uint_as_float(v.s2);
    out.draws = v.nDraw;
  }
  out.exact = v.settled ? 0u : 1u;
}
void finish(const DeviceScene& S, const RenderBuffers& rb, f3 o, f3 d, uint32_t seed0, uint32_t* stack, RouteOut& out)
{
  if(out.exact)
  {
    uint32_t nAlpha = 0;
    settle_closest_exact<false>(S, rb, 0u, o, d, seed0, stack, nAlpha);
    out.draws = nAlpha;
  }
  const float4 h = rb.ps.hit[0];
  out.hit[0] = __float_as_uint(h.x); out.hit[1] = __float_as_uint(h.y); out.hit[2] = __float_as_uint(h.z); out.hit[3] = __float_as_uint(h.w);
  out.seed   = __float_as_uint(rb.ps.rayD[0].w);
}
static_assert(sizeof(RouteOut) == 7 * sizeof(uint32_t), "seven words per route");
}  // namespace

// pt_order_encode for n nodes: lo / hi 12 floats per node ([axis][slot]), cc 4 words per node -> out 2 words per node
extern "C" void po_encode(uint32_t n, const float* lo, const float* hi, const uint32_t* cc, uint32_t* out)
{
  for(uint32_t i = 0; i < n; ++i)
  {
    float l[3][4], h[3][4];
    std::memcpy(l, lo + 12 * size_t(i), sizeof(l));
    std::memcpy(h, hi + 12 * size_t(i), sizeof(h));
    pt_order_encode(l, h, cc + 4 * size_t(i), out + 2 * size_t(i));
  }
}
extern "C" uint32_t po_byte(uint32_t w0, uint32_t w1, uint32_t octant) { return pt_order_byte(w0, w1, octant); }

// the same through a WideNode, pad and all: what k_collapse does to a finished node.  node: 32 words in, 32 words out
extern "C" void po_write_node(uint32_t* node)
{
  WideNode w;
  std::memcpy(&w, node, sizeof(w));
  pt_order_write(w);
  std::memcpy(node, &w, sizeof(w));
}

// npackets packets of 64 rays each on the flat structure of the scene.  outA / outB: 7 words per ray (hit record x 4, RNG state afterwards, draws,
// 1 = the exact loop settled it) of the route from the root / the route through the packet model; route: per ray 0 settled by the packet, 1 handed
// over, 2 exact loop, 3 its packet was sign-incoherent (route (a) stands for it).  stats: inner visits, leaf visits, packets traversed, packets
// that were sign-incoherent.  Returns the traversal-stack overflows of the machine legs.
extern "C" uint32_t po_packet_routes(void* p, int policy, uint32_t npackets, const float* org, const float* dir, const uint32_t* seeds, uint32_t* outA, uint32_t* outB, uint32_t* route,
                                     unsigned long long* stats)
{
  Scene*                s = static_cast<Scene*>(p);
  const DeviceScene&    S = s->dsFlat;
  std::vector<WideNode> wide(S.wide, S.wide + s->flat.wide.size());
  for(WideNode& w : wide)
    pt_order_write(w);
  std::vector<float4> rayO(1), rayD(1), hit(1);  // one path slot, used by every ray in turn
  RenderBuffers       proto;
  std::memset(&proto, 0, sizeof(proto));
  proto.ps.rayO.p = rayO.data(); proto.ps.rayD.p = rayD.data(); proto.ps.hit.p = hit.data();
  WalkCtx              ctx(&proto);
  const RenderBuffers& rb    = ctx.rb;
  uint32_t* const      stack = ctx.stack.data();
  WalkStats            st;
  for(uint32_t pk = 0; pk < npackets; ++pk)
  {
    f3     o[LANES], d[LANES];
    RayHit best[LANES];
    for(int l = 0; l < LANES; ++l)
    {
      const size_t r = size_t(pk) * LANES + l;
      o[l] = f3{org[3 * r], org[3 * r + 1], org[3 * r + 2]};
      d[l] = f3{dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    }
    const bool traversed = packet_walk(S, wide.data(), LANES, o, d, policy, best, st);
    ++(traversed ? st.packets : st.incoherent);
    for(int l = 0; l < LANES; ++l)
    {
      const size_t   r     = size_t(pk) * LANES + l;
      const uint32_t seed0 = seeds[r];
      auto           reset = [&]() {
        rayO[0] = make_float4(o[l].x, o[l].y, o[l].z, 0.f);
        rayD[0] = make_float4(d[l].x, d[l].y, d[l].z, __uint_as_float(seed0));
        hit[0]  = make_float4(-1.f, -1.f, -1.f, -1.f);
      };
      RouteOut a{};
      {
        reset();
        TraceLane L;
        uint32_t  seed = 0;
        lane_fetch_closest(S, rb, 0u, L, seed);
        drive_and_store(S, L, seed, ctx, a);
        finish(S, rb, o[l], d[l], seed0, stack, a);
      }
      RouteOut b{};
      uint32_t way = 3u;
      if(!traversed)
        b = a;
      else
      {
        reset();
        RayHit&    h         = best[l];
        uint32_t   count     = h.count;
        const bool frac      = (h.flags & TF_SAW_FRAC) != 0;
        const bool countPass = needs_count_pass(h.flags, 0, h.slot, h.t, h.zeroMaxT, h.zeroMaxT2, h.zeroMaxT3, count);
        way                  = 2u;
        if(!frac && !countPass)
        {
          uint32_t nDraw, s2;
          if(settle_draws(h.slot, h.w, count, seed0, nDraw, s2))
          {
            store_hit(rb, 0u, h.slot, h.w, false, h.t, h.u, h.v);
            if(nDraw)
              rayD[0].w = __uint_as_float(s2);
            b.draws = nDraw;
            way     = 0u;
          }
          else
            b.exact = 1u;
        }
        else if(countPass)
        {
          way = 1u;
          store_handover(rb, 0u, h, false);
          TraceLane L;
          uint32_t  seed = 0;
          lane_fetch_handover<false>(S, rb, 0u, L, seed);
          drive_and_store(S, L, seed, ctx, b);
        }
        else
          b.exact = 1u;
        finish(S, rb, o[l], d[l], seed0, stack, b);
      }
      std::memcpy(outA + 7 * r, &a, sizeof(a));
      std::memcpy(outB + 7 * r, &b, sizeof(b));
      route[r] = way;
    }
  }
  stats[0] = st.inner; stats[1] = st.leaf; stats[2] = st.packets; stats[3] = st.incoherent;
  return ctx.cnt.stackOverflow;
}
