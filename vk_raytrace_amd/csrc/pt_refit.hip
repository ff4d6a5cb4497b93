// Refit of the kept 4-wide hierarchies after pt_update_vertices: the kernels around the per-slot and per-node bodies of
// pt_refit.h, and the host side that owns the parent table.  No reference counterpart: the reference builds its acceleration structures once, on load.
//   k_rf_parents   once per build: for every child reference of the used node ranges, where its box lives (parent node, slot)
//   k_rf_cost      the tree cost of the structure as it stands (costBefore: measured before the first refit changes a box)
//   k_rf_leaves    one thread per leaf slot: record, texcoords and leaf box made again, then the bottom-up pass of rf_climb
// Everything runs on the caller's stream; the compact nodes and the shading lines are made again by the caller (pt_capi_accel.hip).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "pt_internal.h"

#if PT_BVH_WIDTH == 4
namespace {

// k_refit's hand-off (pt_accel.hip): the arrivals at a node run on different CUs, and a CU's L1 is never refreshed by other CUs' stores
struct DeviceSync {
  static __device__ __forceinline__ unsigned int arrive(unsigned int* counter)
  {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void own() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
  static __device__ __forceinline__ void add(double* p, double v) { atomicAdd(p, v); }
};

// blockIdx.y: the node range; the blocks of a row stride over its nodes
__global__ void __launch_bounds__(256) k_rf_parents(const uint2* __restrict__ ranges, uint32_t firstRange, const WideNode* __restrict__ wide, RfParent* __restrict__ parentOfNode,
                                                    uint32_t numNodes, RfParent* __restrict__ parentOfSlot, uint32_t numSlots)
{
  const uint32_t r     = firstRange + blockIdx.y;
  const uint2    range = ranges[r];
  for(uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < range.y; i += gridDim.x * blockDim.x)
  {
    rf_parents_of(wide, range.x + i, parentOfNode, numNodes, parentOfSlot, numSlots);
    if(i == 0)
      parentOfNode[range.x] = RfParent{RF_NONE, r};  // the range's first node is its root: nothing refers to it
  }
}

__global__ void __launch_bounds__(256) k_rf_cost(const uint2* __restrict__ ranges, uint32_t firstRange, const WideNode* __restrict__ wide, double* costBins)
{
  const uint2 range = ranges[firstRange + blockIdx.y];
  for(uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < range.y; i += gridDim.x * blockDim.x)
  {
    f3 lo, hi;
    atomicAdd(&costBins[(range.x + i) % RF_COST_BINS], rf_union_and_cost(wide[range.x + i], lo, hi));
  }
}

__global__ void __launch_bounds__(256) k_rf_leaves(uint32_t numSlots, const RfSlots* __restrict__ slots, uint32_t numSlotRanges, const InstanceRec* __restrict__ inst,
                                                   const float4* __restrict__ vertices, const uint32_t* __restrict__ indices, TriRec* tris, AlphaRec* alpha, WideNode* wide,
                                                   const RfParent* __restrict__ parentOfNode, const RfParent* __restrict__ parentOfSlot, unsigned int* arrive, float* rootBox,
                                                   double* costBins)
{
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s >= numSlots)
    return;
  const RfSlots R = slots[rf_find_slots(slots, numSlotRanges, s)];
  if(s - R.slotBase >= R.count)
    return;  // a slot no range owns (cannot happen for a built structure)
  f3 lo, hi;
  rf_leaf(R, s, inst, vertices, indices, tris, alpha, lo, hi);
  rf_climb<DeviceSync>(wide, parentOfNode, parentOfSlot[s], lo, hi, arrive, rootBox, costBins);
}

constexpr uint32_t kRowBlocks = 256;    // blocks of a node range's row at most
constexpr uint32_t kRowsMax   = 65535;  // rows per launch (gridDim.y)

size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

int fail(hipStream_t stream, char* err, size_t errLen, const char* why)
{
  snprintf(err, errLen, "refit: %s", why);
  (void)hipStreamSynchronize(stream);
  (void)hipGetLastError();
  return -1;
}

// the node ranges [from, to) in launches of at most kRowsMax rows
template <class Launch>
void each_row_chunk(uint32_t from, uint32_t to, uint32_t maxCount, Launch&& launch)
{
  const uint32_t gx = std::max(1u, std::min(kRowBlocks, (maxCount + 255) / 256));
  for(uint32_t first = from; first < to; first += kRowsMax)
    launch(dim3(gx, std::min(kRowsMax, to - first)), first);
}

int read_cost(hipStream_t stream, const PtRefitTable& T, double* out)
{
  double bins[RF_COST_BINS];
  if(hipMemcpyAsync(bins, T.costBins, sizeof(bins), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess)
    return -1;
  double sum = 0.0;
  for(double b : bins)
    sum += b;
  *out = sum;
  return 0;
}

}  // namespace

size_t pt_refit_table_bytes(uint32_t numNodes, uint32_t numSlots, uint32_t numRanges, uint32_t numSlotRanges)
{
  return align256(sizeof(RfParent) * size_t(numNodes)) + align256(sizeof(RfParent) * size_t(numSlots)) + align256(4 * size_t(numNodes)) + align256(sizeof(uint2) * size_t(numRanges)) +
         align256(sizeof(RfSlots) * size_t(numSlotRanges)) + align256(24 * size_t(numRanges)) + align256(sizeof(double) * RF_COST_BINS);
}

int pt_refit_prepare(hipStream_t stream, void* dMem, const uint32_t* hBaseCount, uint32_t numRanges, const RfSlots* hSlots, uint32_t numSlotRanges, uint32_t numNodes, uint32_t numSlots,
                     const WideNode* dWide, PtRefitTable& T, uint32_t numFirstClass, double* costBuilt2, char* err, size_t errLen)
{
  char* p = (char*)dMem;
  auto  carve = [&](size_t bytes) {
    void* q = p;
    p += align256(bytes);
    return q;
  };
  T.parentOfNode = (RfParent*)carve(sizeof(RfParent) * size_t(numNodes));
  T.parentOfSlot = (RfParent*)carve(sizeof(RfParent) * size_t(numSlots));
  T.arrive       = (unsigned int*)carve(4 * size_t(numNodes));
  T.ranges       = (uint2*)carve(sizeof(uint2) * size_t(numRanges));
  T.slots        = (RfSlots*)carve(sizeof(RfSlots) * size_t(numSlotRanges));
  T.rootBox      = (float*)carve(24 * size_t(numRanges));
  T.costBins     = (double*)carve(sizeof(double) * RF_COST_BINS);
  T.numRanges = numRanges; T.numSlotRanges = numSlotRanges; T.numNodes = numNodes; T.numSlots = numSlots;
  T.maxCount = 0;
  for(uint32_t r = 0; r < numRanges; ++r)
  {
    if(hBaseCount[2 * r + 1] == 0 || uint64_t(hBaseCount[2 * r]) + hBaseCount[2 * r + 1] > numNodes)
      return fail(stream, err, errLen, "a node range leaves the node array");
    T.maxCount = std::max(T.maxCount, hBaseCount[2 * r + 1]);
  }
  for(uint32_t r = 0; r < numSlotRanges; ++r)
    if(uint64_t(hSlots[r].slotBase) + hSlots[r].count > numSlots || (r && hSlots[r].slotBase < hSlots[r - 1].slotBase + hSlots[r - 1].count))
      return fail(stream, err, errLen, "the slot ranges are not ascending inside the slot array");
  if(numRanges == 0 || numSlotRanges == 0)
    return fail(stream, err, errLen, "no hierarchy");
  // 0xff bytes: RfParent{RF_NONE, RF_NONE} for whatever no used node refers to
  if(hipMemsetAsync(T.parentOfNode, 0xff, sizeof(RfParent) * size_t(numNodes), stream) != hipSuccess || hipMemsetAsync(T.parentOfSlot, 0xff, sizeof(RfParent) * size_t(numSlots), stream) != hipSuccess ||
     hipMemsetAsync(T.costBins, 0, sizeof(double) * RF_COST_BINS, stream) != hipSuccess ||
     hipMemcpyAsync(T.ranges, hBaseCount, sizeof(uint2) * size_t(numRanges), hipMemcpyHostToDevice, stream) != hipSuccess ||
     hipMemcpyAsync(T.slots, hSlots, sizeof(RfSlots) * size_t(numSlotRanges), hipMemcpyHostToDevice, stream) != hipSuccess)
    return fail(stream, err, errLen, "upload failed");
  each_row_chunk(0, numRanges, T.maxCount, [&](dim3 grid, uint32_t first) {
    k_rf_parents<<<grid, 256, 0, stream>>>(T.ranges, first, dWide, T.parentOfNode, numNodes, T.parentOfSlot, numSlots);
  });
  // the cost of the structure as it stands, class by class: the first numFirstClass ranges, then the rest
  numFirstClass = std::min(numFirstClass, numRanges);
  const uint32_t bounds[3] = {0u, numFirstClass, numRanges};
  for(int cls = 0; cls < 2; ++cls)
  {
    costBuilt2[cls] = 0.0;
    if(bounds[cls] == bounds[cls + 1])
      continue;
    if(hipMemsetAsync(T.costBins, 0, sizeof(double) * RF_COST_BINS, stream) != hipSuccess)
      return fail(stream, err, errLen, "clearing the cost sums failed");
    each_row_chunk(bounds[cls], bounds[cls + 1], T.maxCount, [&](dim3 grid, uint32_t first) { k_rf_cost<<<grid, 256, 0, stream>>>(T.ranges, first, dWide, T.costBins); });
    if(read_cost(stream, T, &costBuilt2[cls]) != 0)
      return fail(stream, err, errLen, "the parent-table kernels failed");
  }
  if(hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess)  // (the host arrays of the two copies above are the caller's)
    return fail(stream, err, errLen, "the parent-table kernels failed");
  return 0;
}

int pt_refit_run(hipStream_t stream, const PtRefitTable& T, const InstanceRec* dInst, const float4* dVertices, const uint32_t* dIndices, TriRec* dTris, AlphaRec* dAlpha, WideNode* dWide,
                 float* hRootBox, double* costAfter, char* err, size_t errLen)
{
  // every polled word is cleared per refit
  if(hipMemsetAsync(T.arrive, 0, 4 * size_t(T.numNodes), stream) != hipSuccess || hipMemsetAsync(T.costBins, 0, sizeof(double) * RF_COST_BINS, stream) != hipSuccess ||
     hipMemsetAsync(T.rootBox, 0, 24 * size_t(T.numRanges), stream) != hipSuccess)
    return fail(stream, err, errLen, "clearing the counters failed");
  if(T.numSlots)  // (no slot at all: nothing to launch, every sum stays 0)
    k_rf_leaves<<<(T.numSlots + 255) / 256, 256, 0, stream>>>(T.numSlots, T.slots, T.numSlotRanges, dInst, dVertices, dIndices, dTris, dAlpha, dWide, T.parentOfNode, T.parentOfSlot, T.arrive,
                                                              T.rootBox, T.costBins);
  if(hipMemcpyAsync(hRootBox, T.rootBox, 24 * size_t(T.numRanges), hipMemcpyDeviceToHost, stream) != hipSuccess || read_cost(stream, T, costAfter) != 0)
    return fail(stream, err, errLen, "the refit kernel failed");
  return 0;
}
#endif  // PT_BVH_WIDTH == 4
