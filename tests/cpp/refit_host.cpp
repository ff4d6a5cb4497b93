// The refit of csrc/pt_refit.h on the CPU (tests/test_refit_host.py, tests/test_refit_gpu.py): ONE pure function over arrays in the dump format of
// csrc/pt_accel_dump.h -- the same per-slot and per-node bodies the kernels of pt_refit.hip run, the arrivals taken one after the other -- plus the
// forms the product makes again after a refit with code of its own: the compact nodes (pt_cnode.h cn_encode, the very function) and the shading lines
// (restated from pt_accel.hip k_shade_tris).  It serves a harness dump on the CPU and a device dump on the GPU.  Every index the arrays hold is
// checked before it is used: a malformed input is refused (negative return), never read past.
#include "th_shims.h"
#include "pt_refit.h"
#include "pt_cnode.h"

namespace {
struct HostSync {  // one thread: an arrival is a plain increment
  static unsigned int arrive(unsigned int* counter) { return (*counter)++; }
  static void         own() {}
  static void         add(double* p, double v) { *p += v; }
};

double sum_bins(const double* bins)
{
  double s = 0.0;
  for(int b = 0; b < RF_COST_BINS; ++b)
    s += bins[b];
  return s;
}
}  // namespace

// wide: numNodes x 32 words, tris: numSlots x 12, alpha: numSlots x 8 (all refitted in place); ranges: (base, count) per hierarchy; slotRanges: RfSlots
// records (5 words); inst: InstanceRec records (128 bytes); vertices: numVertices x 8 floats; cnodes (may be null): numNodes x 20 words, the nodes of
// the ranges are encoded again; shade (may be null): numShade x 32 words, the shading lines of slots 0 .. numShade (world form); rootBox: 6 floats per
// range; costs: [0] the tree cost of the arrays as given, [1] after the refit.  Returns 0, or the negative number of the check that refused the input.
extern "C" int rfh_refit(uint32_t numNodes, uint32_t* wideWords, uint32_t numSlots, uint32_t* triWords, uint32_t* alphaWords, uint32_t numRanges, const uint32_t* ranges,
                         uint32_t numSlotRanges, const uint32_t* slotRanges, uint32_t numInst, const void* instRecs, uint32_t numVertices, const float* vertexWords, uint32_t numIndices,
                         const uint32_t* indices, uint32_t* cnodeWords, uint32_t numShade, uint32_t* shadeWords, float* rootBox, double* costs)
{
#if PT_BVH_WIDTH == 4
  static_assert(sizeof(WideNode) == 128 && sizeof(TriRec) == 48 && sizeof(AlphaRec) == 32 && sizeof(InstanceRec) == 128 && sizeof(RfSlots) == 20 && sizeof(CompactNode) == 80, "dump format");
  WideNode*          wide  = reinterpret_cast<WideNode*>(wideWords);
  TriRec*            tris  = reinterpret_cast<TriRec*>(triWords);
  AlphaRec*          alpha = reinterpret_cast<AlphaRec*>(alphaWords);
  const InstanceRec* inst  = static_cast<const InstanceRec*>(instRecs);
  const float4*      vertices = reinterpret_cast<const float4*>(vertexWords);
  const RfSlots*     slots = reinterpret_cast<const RfSlots*>(slotRanges);
  if(numRanges == 0 || numSlotRanges == 0)
    return -1;
  for(uint32_t r = 0; r < numRanges; ++r)
    if(ranges[2 * r + 1] == 0 || uint64_t(ranges[2 * r]) + ranges[2 * r + 1] > numNodes)
      return -2;
  for(uint32_t r = 0; r < numSlotRanges; ++r)
    if(uint64_t(slots[r].slotBase) + slots[r].count > numSlots || (r && slots[r].slotBase < slots[r - 1].slotBase + slots[r - 1].count) || slots[r].form > RF_VERTEX)
      return -3;
  // what a leaf slot names must exist: the instance, the primitive's three indices, their vertices
  auto mesh_ok = [&](uint32_t vertexOffset, uint32_t firstIndex, uint32_t prim) {
    const uint64_t i0 = uint64_t(firstIndex) + 3 * uint64_t(prim);
    if(i0 + 3 > numIndices)
      return false;
    for(int j = 0; j < 3; ++j)
      if(uint64_t(vertexOffset) + indices[i0 + j] >= numVertices)
        return false;
    return true;
  };
  for(uint32_t r = 0; r < numSlotRanges; ++r)
    for(uint32_t s = slots[r].slotBase; s < slots[r].slotBase + slots[r].count; ++s)
    {
      if(slots[r].form == RF_WORLD)
      {
        const uint32_t ii = __float_as_uint(tris[s].e1n.w);
        if(ii >= numInst || !mesh_ok(inst[ii].vertexOffset, inst[ii].firstIndex, __float_as_uint(tris[s].e2p.w)))
          return -4;
      }
      else if(!mesh_ok(slots[r].vertexOffset, slots[r].firstIndex, __float_as_uint(tris[s].p0w.w)))
        return -4;
    }
  std::vector<RfParent>     parentOfNode(numNodes, RfParent{RF_NONE, RF_NONE}), parentOfSlot(numSlots, RfParent{RF_NONE, RF_NONE});
  std::vector<unsigned int> arrive(numNodes, 0u);
  double                    bins[RF_COST_BINS] = {};
  for(uint32_t r = 0; r < numRanges; ++r)
  {
    for(uint32_t i = 0; i < ranges[2 * r + 1]; ++i)
    {
      f3 lo, hi;
      rf_parents_of(wide, ranges[2 * r] + i, parentOfNode.data(), numNodes, parentOfSlot.data(), numSlots);
      bins[(ranges[2 * r] + i) % RF_COST_BINS] += rf_union_and_cost(wide[ranges[2 * r] + i], lo, hi);
    }
    parentOfNode[ranges[2 * r]] = RfParent{RF_NONE, r};
  }
  costs[0] = sum_bins(bins);
  for(double& b : bins)
    b = 0.0;
  for(uint32_t k = 0; k < 6 * numRanges; ++k)
    rootBox[k] = 0.0f;
  for(uint32_t s = 0; s < numSlots; ++s)
  {
    const RfSlots R = slots[rf_find_slots(slots, numSlotRanges, s)];
    if(s - R.slotBase >= R.count)
      continue;
    f3 lo, hi;
    rf_leaf(R, s, inst, vertices, indices, tris, alpha, lo, hi);
    rf_climb<HostSync>(wide, parentOfNode.data(), parentOfSlot[s], lo, hi, arrive.data(), rootBox, bins);
  }
  costs[1] = sum_bins(bins);
  if(cnodeWords)
  {
    CompactNode* cn = reinterpret_cast<CompactNode*>(cnodeWords);
    for(uint32_t r = 0; r < numRanges; ++r)
      for(uint32_t i = 0; i < ranges[2 * r + 1]; ++i)
        if(!cn_encode(wide[ranges[2 * r] + i], cn[ranges[2 * r] + i]))
          return -5;
  }
  if(shadeWords)
  {  // k_shade_tris: the three vertices' attribute pairs, then (instance, primitive, material, 0) and a zero quad
    if(numShade > numSlots)
      return -6;
    float4* out = reinterpret_cast<float4*>(shadeWords);
    for(uint32_t s = 0; s < numShade; ++s)
    {
      const uint32_t ii = __float_as_uint(tris[s].e1n.w), prim = __float_as_uint(tris[s].e2p.w);
      if(ii >= numInst || !mesh_ok(inst[ii].vertexOffset, inst[ii].firstIndex, prim))
        return -6;
      const InstanceRec& I = inst[ii];
      const uint32_t*    t = indices + I.firstIndex + 3 * size_t(prim);
      float4*            o = out + size_t(s) * PT_SHADE_REC_QUADS;
      for(int k = 0; k < 3; ++k)
      {
        o[2 * k]     = vertices[size_t(I.vertexOffset + t[k]) * 2];
        o[2 * k + 1] = vertices[size_t(I.vertexOffset + t[k]) * 2 + 1];
      }
      o[6] = make_float4(__uint_as_float(ii), __uint_as_float(prim), __uint_as_float(uint32_t(I.materialIndex)), 0.f);
      o[7] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  return 0;
#else
  return -100;
#endif
}
