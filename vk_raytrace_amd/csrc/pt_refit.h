// Refit of a built acceleration structure after the vertices moved (pt_update_vertices / pt_refit_accel): the per-slot and
// per-node bodies, plain inline functions compiled by hipcc for the device (pt_refit.hip) and by g++ for the host (tests/cpp/refit_host.cpp), so that
// the device is held bit for bit to the host build.  Nothing here chooses a topology: every child word, every slot's (instance, primitive) and every
// node count stays; the records, the leaf boxes, the inner boxes and the order tables are made again from the vertices, in the operation order of the
// builders (pt_accel.hip: T1 of k_world_tris, tri_box, the min / max union of k_refit, pt_order_write).
//
// A structure is given as node ranges (base, count) -- the flat hierarchy, or the merged hierarchy and every BLAS of the two-level mode -- and slot
// ranges (RfSlots) that say which form the leaf records of a range have and, for the vertex form, which mesh they come from.
#pragma once
#include <cfloat>
#include <cmath>
#include "pt_device.h"
#include "pt_order.h"

#if defined(__HIPCC__)
#define RF_FN __host__ __device__ inline
#else
#define RF_FN inline
#endif

#if PT_BVH_WIDTH == 4

#define RF_NONE 0xffffffffu
#define RF_WORLD 0u   // TriRec in world-space edge form (flat and merged structure): instance in e1n.w, primitive in e2p.w
#define RF_VERTEX 1u  // TriRec in object-space vertex form (a BLAS): primitive in p0w.w

// the leaf slots [slotBase, slotBase + count) and where their triangles come from
struct RfSlots {
  uint32_t slotBase, count, form;
  uint32_t vertexOffset, firstIndex;  // RF_VERTEX: the mesh (RF_WORLD: the record's instance says)
};
// where the box of a node or of a leaf slot lives: slot k of node `node`; a root has node == RF_NONE and k = the index of its node range
struct RfParent {
  uint32_t node, k;
};

RF_FN f3 rf_load_pos(const float4* vertices, uint32_t v)
{
  const float4 a = vertices[size_t(v) * 2];
  return f3{a.x, a.y, a.z};
}
RF_FN float rf_min(float a, float b) { return fminf(a, b); }
RF_FN float rf_max(float a, float b) { return fmaxf(a, b); }

// the padded box of an edge-form record, as pt_accel.hip tri_box computes it
RF_FN void rf_tri_box(f3 p0, f3 e1, f3 e2, f3& lo, f3& hi)
{
  const f3 p1 = p0 + e1;
  const f3 p2 = p0 + e2;
  lo = f3{rf_min(p0.x, rf_min(p1.x, p2.x)), rf_min(p0.y, rf_min(p1.y, p2.y)), rf_min(p0.z, rf_min(p1.z, p2.z))};
  hi = f3{rf_max(p0.x, rf_max(p1.x, p2.x)), rf_max(p0.y, rf_max(p1.y, p2.y)), rf_max(p0.z, rf_max(p1.z, p2.z))};
  const f3 m   = f3{rf_max(fabsf(lo.x), fabsf(hi.x)), rf_max(fabsf(lo.y), fabsf(hi.y)), rf_max(fabsf(lo.z), fabsf(hi.z))};
  const f3 pad = m * 4e-6f + 1e-30f;
  lo = lo - pad;
  hi = hi + pad;
}

// the range that holds slot s (ranges sorted by slotBase, s inside one of them)
RF_FN uint32_t rf_find_slots(const RfSlots* ranges, uint32_t numRanges, uint32_t s)
{
  uint32_t lo = 0, hi = numRanges - 1;
  while(lo < hi)
  {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if(ranges[mid].slotBase <= s)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

RF_FN void rf_write_uv(AlphaRec& ar, const float4* vertices, uint32_t v0, uint32_t v1, uint32_t v2)
{
  const float4 b0 = vertices[size_t(v0) * 2 + 1], b1 = vertices[size_t(v1) * 2 + 1], b2 = vertices[size_t(v2) * 2 + 1];
  ar.uv0[0] = b0.x; ar.uv0[1] = b0.y; ar.uv1[0] = b1.x; ar.uv1[1] = b1.y; ar.uv2[0] = b2.x; ar.uv2[1] = b2.y;
}

// One leaf slot: the record and the any-hit texcoords made again from the vertices (the three .w words, the material and the padding word stay), the
// box of the new record returned.
//   RF_WORLD   T1 in k_world_tris's order: xform_point of the three vertices, then e1 = p1 - p0 and e2 = p2 - p0
//   RF_VERTEX  the three object-space positions as k_blas_vertex_form writes them; the box is that of the edge form under the identity transform,
//              which is what the BLAS build computed it from
RF_FN void rf_leaf(const RfSlots& R, uint32_t s, const InstanceRec* inst, const float4* vertices, const uint32_t* indices, TriRec* tris, AlphaRec* alpha, f3& lo, f3& hi)
{
  TriRec r = tris[s];
  if(R.form == RF_WORLD)
  {
    const InstanceRec& I = inst[__float_as_uint(r.e1n.w)];
    const uint32_t*    t = indices + I.firstIndex + 3 * size_t(__float_as_uint(r.e2p.w));
    const uint32_t     v0 = I.vertexOffset + t[0], v1 = I.vertexOffset + t[1], v2 = I.vertexOffset + t[2];
    const Affine       M  = I.objectToWorld;
    const f3           p0 = xform_point(M, rf_load_pos(vertices, v0));
    const f3           p1 = xform_point(M, rf_load_pos(vertices, v1));
    const f3           p2 = xform_point(M, rf_load_pos(vertices, v2));
    const f3           e1 = p1 - p0, e2 = p2 - p0;
    r.p0w = make_float4(p0.x, p0.y, p0.z, r.p0w.w);
    r.e1n = make_float4(e1.x, e1.y, e1.z, r.e1n.w);
    r.e2p = make_float4(e2.x, e2.y, e2.z, r.e2p.w);
    rf_write_uv(alpha[s], vertices, v0, v1, v2);
    rf_tri_box(p0, e1, e2, lo, hi);
  }
  else
  {
    const uint32_t* t = indices + R.firstIndex + 3 * size_t(__float_as_uint(r.p0w.w));
    const uint32_t  v0 = R.vertexOffset + t[0], v1 = R.vertexOffset + t[1], v2 = R.vertexOffset + t[2];
    const f3        a = rf_load_pos(vertices, v0), b = rf_load_pos(vertices, v1), c = rf_load_pos(vertices, v2);
    r.p0w = make_float4(a.x, a.y, a.z, r.p0w.w);
    r.e1n = make_float4(b.x, b.y, b.z, r.e1n.w);
    r.e2p = make_float4(c.x, c.y, c.z, r.e2p.w);
    rf_write_uv(alpha[s], vertices, v0, v1, v2);
    Affine id;
    id.r0 = make_float4(1.f, 0.f, 0.f, 0.f);
    id.r1 = make_float4(0.f, 1.f, 0.f, 0.f);
    id.r2 = make_float4(0.f, 0.f, 1.f, 0.f);
    const f3 p0 = xform_point(id, a), p1 = xform_point(id, b), p2 = xform_point(id, c);
    rf_tri_box(p0, p1 - p0, p2 - p0, lo, hi);
  }
  tris[s] = r;
}

// planes of a node as six rows of four floats: min x, y, z then max x, y, z; row a, column k = child slot k
RF_FN float* rf_planes(WideNode& w) { return &w.minx[0].x; }
RF_FN const float* rf_planes(const WideNode& w) { return &w.minx[0].x; }
RF_FN const uint32_t* rf_children(const WideNode& w) { return &w.child[0].x; }

RF_FN void rf_store_box(WideNode* wide, RfParent p, f3 lo, f3 hi)
{
  float* f = rf_planes(wide[p.node]) + p.k;  // six different words of the node; the other slots' words belong to other threads
  f[0] = lo.x; f[4] = lo.y; f[8] = lo.z; f[12] = hi.x; f[16] = hi.y; f[20] = hi.z;
}

RF_FN uint32_t rf_used(const WideNode& w)
{
  const uint32_t* c = rf_children(w);
  return (c[0] != BVH_NONE) + (c[1] != BVH_NONE) + (c[2] != BVH_NONE) + (c[3] != BVH_NONE);
}

// the min / max union of the used slots (k_refit's fminf / fmaxf, slot by slot) and the node's tree-cost term: the sum over its used child boxes of
// dx dy + dy dz + dz dx, differences and products in double from the fp32 planes
RF_FN double rf_union_and_cost(const WideNode& w, f3& lo, f3& hi)
{
  const float*    f = rf_planes(w);
  const uint32_t* c = rf_children(w);
  lo = f3{FLT_MAX, FLT_MAX, FLT_MAX};
  hi = f3{-FLT_MAX, -FLT_MAX, -FLT_MAX};
  double cost = 0.0;
  for(int k = 0; k < 4; ++k)
    if(c[k] != BVH_NONE)
    {
      lo = f3{rf_min(lo.x, f[k]), rf_min(lo.y, f[4 + k]), rf_min(lo.z, f[8 + k])};
      hi = f3{rf_max(hi.x, f[12 + k]), rf_max(hi.y, f[16 + k]), rf_max(hi.z, f[20 + k])};
      const double dx = double(f[12 + k]) - double(f[k]), dy = double(f[16 + k]) - double(f[4 + k]), dz = double(f[20 + k]) - double(f[8 + k]);
      cost += dx * dy + dy * dz + dz * dx;
    }
  return cost;
}

// the parent table: node i says where the box of each of its children lives
// (a reference that leaves its array is skipped: the slot or node it names then has no parent and the refit leaves it alone)
RF_FN void rf_parents_of(const WideNode* wide, uint32_t i, RfParent* parentOfNode, uint32_t numNodes, RfParent* parentOfSlot, uint32_t numSlots)
{
  const uint32_t* c = rf_children(wide[i]);
  for(uint32_t k = 0; k < 4; ++k)
    if(c[k] != BVH_NONE && (c[k] & BVH_SLOT_MASK) < ((c[k] & BVH_LEAF) ? numSlots : numNodes))
      ((c[k] & BVH_LEAF) ? parentOfSlot : parentOfNode)[c[k] & BVH_SLOT_MASK] = RfParent{i, k};
}

#define RF_COST_BINS 64  // the cost terms are added into this many accumulators (by node number), summed on the host

// The bottom-up pass from one leaf slot, k_refit's protocol (pt_accel.hip): a box goes into its parent's slot, then the writer arrives at the parent
// -- Sync::arrive is an agent-scope release with the stores drained, then an agent-scope relaxed fetch_add on the node's counter.  The arrival that
// finds used - 1 earlier ones is the last: it takes an agent-scope acquire (Sync::own), owns the node, writes its order table, and carries the union
// of its slots one level up.  Every other arrival returns; nobody waits.  rootBox: six floats per node range, written by the owner of the range's root.
template <class Sync>
RF_FN void rf_climb(WideNode* wide, const RfParent* parentOfNode, RfParent p, f3 lo, f3 hi, unsigned int* arrive, float* rootBox, double* costBins)
{
  while(p.node != RF_NONE)  // (a slot nothing refers to has no parent)
  {
    rf_store_box(wide, p, lo, hi);
    const uint32_t     cur  = p.node;
    const unsigned int prev = Sync::arrive(&arrive[cur]);
    if(prev + 1u != rf_used(wide[cur]))  // (the child words are not written by a refit: reading them needs no hand-off)
      return;
    Sync::own();
    WideNode w = wide[cur];
    pt_order_write(w);
    wide[cur].pad[0].x = w.pad[0].x;
    wide[cur].pad[0].y = w.pad[0].y;
    Sync::add(&costBins[cur % RF_COST_BINS], rf_union_and_cost(w, lo, hi));
    p = parentOfNode[cur];
    if(p.node == RF_NONE)
    {
      if(p.k == RF_NONE)  // a node nothing refers to that is no range's root
        return;
      float* b = rootBox + 6 * size_t(p.k);
      b[0] = lo.x; b[1] = lo.y; b[2] = lo.z; b[3] = hi.x; b[4] = hi.y; b[5] = hi.z;
      return;
    }
  }
}

#endif  // PT_BVH_WIDTH == 4
