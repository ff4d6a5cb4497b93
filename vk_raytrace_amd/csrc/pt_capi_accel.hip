// The acceleration-structure side of the C ABI: pt_build_accel (flat structure, or BLAS per prim-mesh + merged world-space structure + TLAS),
// the refit of pt_update_instances, the two calls that force a rebuild (pt_use_any_hit, pt_set_accel_mode) and the deforming meshes
// (pt_update_vertices, pt_refit_accel; kernels: pt_refit.hip).  Host sequencing only: the builders themselves are pt_accel.hip / pt_sah.hip.  Mirrors AccelStructure (src/accelstruct.cpp) of the reference.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include "pt_context.h"
#include "pt_scene_records.h"

namespace {
// world bounds (origin cells of the ray-sort keys) from the binary root of a hierarchy
void bounds_from_root(pt_context* c, const BvhNode& root, bool two)
{
  const float lmin[3] = {root.a.x, root.a.y, root.a.z}, lmax[3] = {root.a.w, root.b.x, root.b.y};
  const float rmin[3] = {root.b.z, root.b.w, root.c.x}, rmax[3] = {root.c.y, root.c.z, root.c.w};
  for(int k = 0; k < 3; ++k)
  {
    const float mn = two ? std::min(lmin[k], rmin[k]) : lmin[k], mx = two ? std::max(lmax[k], rmax[k]) : lmax[k];
    c->scene.boundsMin[k]    = std::isfinite(mn) ? mn : 0.f;
    c->scene.boundsInvExt[k] = (std::isfinite(mx - mn) && mx > mn) ? 1.0f / (mx - mn) : 0.f;
  }
}

// a structure that is rebuilt or whose topology changes takes the parent table of the refit with it.  keepBlasCost: only the merged structure is built
// again -- the cost of the BLASes as built, if it was measured, still belongs to them
void drop_refit_table(pt_context* c, bool keepBlasCost = false)
{
  c->haveRefitTable = false;
  c->haveCostBlas   = c->haveCostBlas && keepBlasCost;
  dev_free(c->dRefit);
}

// hPrimBound of the prim-meshes pt_update_vertices touched, by build_scene_records' rule: the maximum |coordinate| over the mesh's finite coordinates
void refresh_prim_bounds(pt_context* c)
{
  for(size_t p = 0; p < c->primTouched.size(); ++p)
  {
    if(!c->primTouched[p])
      continue;
    c->primTouched[p] = 0;
    float        b = 0.f;
    const float* q = c->hPositions.data() + 3 * size_t(c->hPrimMeshVerts[2 * p]);
    for(size_t k = 0; k < 3 * size_t(c->hPrimMeshVerts[2 * p + 1]); ++k)
      if(std::isfinite(q[k]))
        b = std::max(b, std::fabs(q[k]));
    c->hPrimBound[p] = b;
  }
}

// compact nodes of a real two-level structure: every bottom-level structure at its node base, and the TLAS
void build_cnodes_two_level(pt_context* c)
{
  c->haveCNodes = false;
  if(!c->tune.cnodes || c->nodeCapacity == 0 || c->numTlasNodes == 0)
  {
    dev_free(c->dCNodes);
    dev_free(c->dCTlas);
    return;
  }
  if(dev_alloc(c, c->dCNodes, sizeof(CompactNode) * size_t(c->nodeCapacity)) != PT_OK || dev_alloc(c, c->dCTlas, sizeof(CompactNode) * size_t(c->numTlasNodes)) != PT_OK)
  {
    (void)hipGetLastError();
    return;
  }
  std::vector<uint32_t> ranges = c->hBlasRanges;
  if(c->mergedWide)
  {
    ranges.push_back(0u);
    ranges.push_back(c->mergedWide);
  }
  c->haveCNodes = pt_compact_node_ranges(c->stream, ranges.data(), uint32_t(ranges.size() / 2), (const WideNode*)c->dWide.p, (CompactNode*)c->dCNodes.p) == 0 &&
                  pt_compact_nodes(c->stream, c->numTlasNodes, (const WideNode*)c->dTlas.p, (CompactNode*)c->dCTlas.p) == 0;
}

// DeviceScene::cnodes over the first n wide nodes of a flat-format structure (best effort: without it the kernels walk the WideNodes)
void build_cnodes(pt_context* c, uint32_t n)
{
  c->haveCNodes = false;
  if(!c->tune.cnodes || n == 0)
  {
    dev_free(c->dCNodes);
    return;
  }
  if(dev_alloc(c, c->dCNodes, sizeof(CompactNode) * size_t(n)) != PT_OK)
  {
    (void)hipGetLastError();
    return;
  }
  c->haveCNodes = pt_compact_nodes(c->stream, n, (const WideNode*)c->dWide.p, (CompactNode*)c->dCNodes.p) == 0;
}
// DeviceScene::shadeTris over the first n leaf records of a flat-format structure (best effort: without the memory k_shade takes the indexed route)
void build_shade_tris(pt_context* c, uint32_t n)
{
  c->haveShadeTris = false;
  if(!c->tune.shadeTris || n == 0)
  {
    dev_free(c->dShadeTris);
    return;
  }
  if(dev_alloc(c, c->dShadeTris, sizeof(float4) * PT_SHADE_REC_QUADS * size_t(n)) != PT_OK)
  {
    (void)hipGetLastError();
    return;
  }
  pt_launch_shade_tris(c->stream, n, (const TriRec*)c->dTris.p, (const InstanceRec*)c->dInstances.p, (const float4*)c->dVertices.p, (const uint32_t*)c->dIndices.p,
                       (float4*)c->dShadeTris.p);
  c->haveShadeTris = hipStreamSynchronize(c->stream) == hipSuccess && hipGetLastError() == hipSuccess;
}

// TLAS of the two-level structure over the current instance transforms (also the refit after pt_update_instances: the BLASes stay)
int build_tlas(pt_context* c)
{
  const std::vector<InstanceRec> inst = effective_instances(c);
  std::vector<uint32_t>          active, triBase(inst.empty() ? 1 : inst.size(), 0u);
  std::vector<float>             pad(inst.empty() ? 2 : 2 * inst.size(), 0.f);
  std::vector<char> isMerged(inst.size(), 0);
  for(uint32_t i : c->hMerged)
    isMerged[i] = 1;
  for(uint32_t i = 0; i < inst.size(); ++i)
  {
    triBase[i] = inst[i].triBase;
    if(inst[i].triCount == 0 || isMerged[i])
      continue;
    active.push_back(i);
    two_level_pad(inst[i], c->hPrimBound[inst[i].primMesh], pad[2 * i], pad[2 * i + 1]);
  }
  c->numActive = uint32_t(active.size());
  int rc;
  const uint32_t none = 0;
  if((rc = upload(c, c->dActive, active.empty() ? &none : active.data(), 4 * std::max<size_t>(1, active.size()))) != PT_OK) return rc;
  if((rc = upload(c, c->dInstTriBase, triBase.data(), 4 * triBase.size())) != PT_OK) return rc;
  {  // block table of instance_of_world_tri (pt_trace.h): entry e = the last instance whose triBase <= e << PT_INST_BLOCK_SHIFT
    const size_t          entries = (size_t(c->numTris) >> PT_INST_BLOCK_SHIFT) + 2;
    std::vector<uint32_t> block(entries, 0u);
    uint32_t              at = 0;
    for(size_t e = 0; e < entries; ++e)
    {
      const uint64_t first = uint64_t(e) << PT_INST_BLOCK_SHIFT;
      while(at + 1 < triBase.size() && uint64_t(triBase[at + 1]) <= first)
        ++at;
      block[e] = at;
    }
    if((rc = upload(c, c->dInstBlock, block.data(), 4 * block.size())) != PT_OK) return rc;
  }
  if((rc = upload(c, c->dInstPad, pad.data(), 4 * pad.size())) != PT_OK) return rc;
  if((rc = upload(c, c->dInstNodeBase, c->hInstNodeBase.empty() ? &none : c->hInstNodeBase.data(), 4 * std::max<size_t>(1, c->hInstNodeBase.size()))) != PT_OK) return rc;
  bool mergedOpaque = true;  // the reference to the merged structure's leaf is tagged BVH_ALPHA only when one of its triangles can draw
  for(uint32_t i : c->hMerged)
    mergedOpaque = mergedOpaque && (inst[i].flags & TRI_OPAQUE) != 0;
  const uint32_t numPrims = c->numActive + (c->mergedTris ? 1u : 0u);
  if((rc = dev_alloc(c, c->dTlas, sizeof(WideNode) * size_t(std::max(1u, numPrims)))) != PT_OK) return rc;
  if((rc = dev_alloc(c, c->dTlasLeaves, sizeof(TlasLeaf) * size_t(std::max(1u, numPrims)))) != PT_OK) return rc;
  auto    t0 = std::chrono::steady_clock::now();
  char    msg[256];
  BvhNode root{};
  if(pt_tlas_build(c->stream, c->tune, (const InstanceRec*)c->dInstances.p, (const uint32_t*)c->dActive.p, c->numActive, (const uint32_t*)c->dInstNodeBase.p, (const float*)c->dInstPad.p,
                   (const float4*)c->dVertices.p, (const uint32_t*)c->dIndices.p, (WideNode*)c->dTlas.p, (TlasLeaf*)c->dTlasLeaves.p, &root, &c->numTlasNodes, msg, sizeof(msg),
                   c->mergedTris ? c->mergedBox : nullptr, 0u, mergedOpaque) != 0)
    return c->fail(PT_ERR_HIP, "TLAS build: %s", msg);
  c->msBuildTlas = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for(int k = 0; k < 3; ++k)
    c->scene.boundsMin[k] = c->scene.boundsInvExt[k] = 0.f;
  if(numPrims > 0)
    bounds_from_root(c, root, numPrims > 1 && root.d.y != BVH_NONE);
  c->mergedOnly = c->mergedTris > 0 && c->numActive == 0;
  if(c->mergedOnly)
    build_cnodes(c, c->mergedWide);  // the flat kernels run on the merged structure
  else
    build_cnodes_two_level(c);
  build_shade_tris(c, c->mergedOnly ? c->mergedTris : 0u);
  return PT_OK;
}

// (re)builds the merged world-space structure over c->hMerged with the current transforms, in place at slot 0 / node 0 of the BLAS arrays
int build_merged(pt_context* c)
{
  const uint32_t before = c->mergedWide;
  struct KeepStat {  // the wide-node statistic follows the merged structure's size on every (re)build, refits included
    pt_context* c; uint32_t before;
    ~KeepStat() { c->numWideNodes = c->numWideNodes - std::min(c->numWideNodes, before) + c->mergedWide; }
  } keep{c, before};
  c->mergedWide = 0;
  drop_refit_table(c, true);  // the merged structure gets a new topology
  if(c->hMerged.empty())
    return PT_OK;
  const std::vector<InstanceRec> inst = effective_instances(c);
  std::vector<InstanceRec>       sub;
  std::vector<uint32_t>          worldBase;
  uint32_t                       n = 0;
  for(uint32_t i : c->hMerged)
  {
    InstanceRec I = inst[i];
    worldBase.push_back(I.triBase);
    I.triBase = n;
    n += I.triCount;
    sub.push_back(I);
  }
  char msg[256];
  if(pt_merged_build(c->stream, c->tune, sub.data(), c->hMerged.data(), worldBase.data(), uint32_t(sub.size()), n, (const float4*)c->dVertices.p, (const uint32_t*)c->dIndices.p, (TriRec*)c->dTris.p,
                     (AlphaRec*)c->dAlphaRecs.p, (WideNode*)c->dWide.p, 0u, 0u, &c->mergedWide, c->mergedBox, msg, sizeof(msg)) != 0)
    return c->fail(PT_ERR_HIP, "pt_build_accel (two-level, merged structure): %s", msg);
  return PT_OK;
}

// AccelStructure::create as the reference does it [src/accelstruct.cpp:110-162]: one BLAS per prim-mesh that some node instantiates, one TLAS
// instance per node
int build_two_level(pt_context* c)
{
  const std::vector<InstanceRec> inst = effective_instances(c);
  std::map<int32_t, uint32_t>    blasOf;
  std::vector<PtBlasDesc>        blas;
  uint64_t                       slots = 0, nodes = 0;
  c->hInstNodeBase.assign(inst.size(), 0u);
  // prim-meshes instantiated once: their instances share one world-space structure, first in the arrays
  c->hMerged.clear();
  c->mergedTris = 0;
  c->mergedOnly = false;
  std::vector<char> isMerged(inst.size(), 0);
  if(c->tune.mergeSingles)
  {
    std::map<int32_t, uint32_t> uses;
    for(const InstanceRec& I : inst)
      if(I.triCount)
        uses[I.primMesh]++;
    for(uint32_t i = 0; i < inst.size(); ++i)
      if(inst[i].triCount && uses[inst[i].primMesh] == 1)
      {
        c->hMerged.push_back(i);
        isMerged[i] = 1;
        c->mergedTris += inst[i].triCount;
      }
    slots = c->mergedTris;
    nodes = c->mergedTris ? std::max(1u, c->mergedTris - 1) : 0;
  }
  for(uint32_t i = 0; i < inst.size(); ++i)
  {
    const InstanceRec& I = inst[i];
    if(I.triCount == 0 || isMerged[i])
      continue;
    auto it = blasOf.find(I.primMesh);
    if(it == blasOf.end())
    {
      PtBlasDesc d{};
      d.primMesh = uint32_t(I.primMesh); d.vertexOffset = I.vertexOffset; d.firstIndex = I.firstIndex; d.triCount = I.triCount;
      d.flags = I.flags & ~TRI_FLIP; d.materialIndex = I.materialIndex;
      d.slotBase = uint32_t(slots); d.nodeBase = uint32_t(nodes);
      slots += I.triCount;
      nodes += std::max(1u, I.triCount - 1);
      it = blasOf.emplace(I.primMesh, uint32_t(blas.size())).first;
      blas.push_back(d);
    }
    c->hInstNodeBase[i] = blas[it->second].nodeBase;
  }
  if(slots > BVH_SLOT_MASK || nodes > BVH_SLOT_MASK)
    return c->fail(PT_ERR_INVALID, "two-level structure: %llu distinct triangles exceed the reference range", (unsigned long long)slots);
  int rc;
  if((rc = dev_alloc(c, c->dTris, sizeof(TriRec) * size_t(std::max<uint64_t>(1, slots)))) != PT_OK) return rc;
  if((rc = dev_alloc(c, c->dAlphaRecs, sizeof(AlphaRec) * size_t(std::max<uint64_t>(1, slots)))) != PT_OK) return rc;
  if((rc = dev_alloc(c, c->dWide, sizeof(WideNode) * size_t(std::max<uint64_t>(1, nodes)))) != PT_OK) return rc;
  dev_free(c->dBvh);  // the binary nodes are a build temporary here
  auto t0 = std::chrono::steady_clock::now();
  char msg[256];
  if(pt_blas_build(c->stream, c->tune, blas.data(), uint32_t(blas.size()), (const float4*)c->dVertices.p, (const uint32_t*)c->dIndices.p, (TriRec*)c->dTris.p, (AlphaRec*)c->dAlphaRecs.p,
                   (WideNode*)c->dWide.p, msg, sizeof(msg)) != 0)
    return c->fail(PT_ERR_HIP, "pt_build_accel (two-level): %s", msg);
  if((rc = build_merged(c)) != PT_OK)
    return rc;
  c->hBlas = blas;
  c->hBlasRanges.clear();
  for(const PtBlasDesc& d : blas)
  {
    c->hBlasRanges.push_back(d.nodeBase);
    c->hBlasRanges.push_back(d.numWide);
  }
  c->nodeCapacity = uint32_t(std::max<uint64_t>(1, nodes));
  c->numBlas      = uint32_t(blas.size()) + (c->mergedTris ? 1u : 0u);
  c->numBvhNodes  = uint32_t(nodes);
  c->numWideNodes = c->mergedWide;  // (build_merged above already counted it into the old total: start over)
  for(const PtBlasDesc& d : blas)
    c->numWideNodes += d.numWide;
  if((rc = build_tlas(c)) != PT_OK)
    return rc;
  HIP_TRY(c, sync_all(c));
  c->msBuild   = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  c->haveAccel = true;
  c->warmPending = true;
  refresh_scene_ptrs(c);
  return PT_OK;
}
}  // namespace

extern "C" {

int pt_build_accel(pt_context* c)
{
  CTX_CHECK(c);
  if(!c->haveScene)
    return c->fail(PT_ERR_STATE, "pt_build_accel before pt_set_scene");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  c->haveAccel  = false;
  c->accelStale = false;
  drop_refit_table(c);
  refresh_prim_bounds(c);  // (pt_update_vertices without a structure, or with one that is rebuilt instead of refitted)
  // overflows of the previous structure say nothing about the new one (check_traversal)
  HIP_TRY(c, hipMemset((char*)c->dCounters.p + offsetof(Counters, stackOverflow), 0, sizeof(unsigned int)));
  clear_overflow(c);
  if(c->accelMode == PT_ACCEL_TWO_LEVEL)
    return build_two_level(c);
  int rc;
  c->numBlas = c->numTlasNodes = c->numActive = 0;
  c->hMerged.clear();
  c->mergedTris = c->mergedWide = 0;
  c->mergedOnly = false;
  c->hBlasRanges.clear();
  c->hBlas.clear();
  c->nodeCapacity = 0;
  dev_free(c->dCTlas);
  c->numBvhNodes = c->numTris > 1 ? c->numTris - 1 : 1;
  if((rc = dev_alloc(c, c->dTris, sizeof(TriRec) * size_t(c->numTris ? c->numTris : 1))) != PT_OK) return rc;
  if((rc = dev_alloc(c, c->dAlphaRecs, sizeof(AlphaRec) * size_t(c->numTris ? c->numTris : 1))) != PT_OK) return rc;
  if((rc = dev_alloc(c, c->dBvh, sizeof(BvhNode) * size_t(c->numBvhNodes))) != PT_OK) return rc;
  if((rc = dev_alloc(c, c->dWide, sizeof(WideNode) * size_t(c->numBvhNodes))) != PT_OK) return rc;
  auto t0 = std::chrono::steady_clock::now();
  char msg[256];
  int brc;
  {  // the arena goes back before the compact nodes and shading lines are allocated, and inside the timed window
    PtScratch scratch;
    scratch.reserve(pt_scratch_bytes(c->tune, c->numTris, false));
    brc = pt_accel_build(c->stream, c->tune, (const InstanceRec*)c->dInstances.p, c->numInstances, (const float4*)c->dVertices.p, (const uint32_t*)c->dIndices.p, c->numTris,
                         (TriRec*)c->dTris.p, (AlphaRec*)c->dAlphaRecs.p, (BvhNode*)c->dBvh.p, (WideNode*)c->dWide.p, &c->numWideNodes, msg, sizeof(msg), scratch);
  }
  if(brc != 0)
    return c->fail(PT_ERR_HIP, "pt_build_accel: %s", msg);
  build_cnodes(c, c->numWideNodes);
  build_shade_tris(c, c->numTris);
  HIP_TRY(c, sync_all(c));
  c->msBuild   = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // world bounds of the triangles = union of the root's two child boxes (origin cells of the ray-sort keys)
  for(int k = 0; k < 3; ++k)
  {
    c->scene.boundsMin[k]    = 0.f;
    c->scene.boundsInvExt[k] = 0.f;
  }
  if(c->numTris > 0)
  {
    BvhNode root;
    HIP_TRY(c, hipMemcpy(&root, c->dBvh.p, sizeof(root), hipMemcpyDeviceToHost));
    bounds_from_root(c, root, c->numTris > 1 && root.d.y != BVH_NONE);
  }
  c->haveAccel = true;
  c->warmPending = true;
  refresh_scene_ptrs(c);
  return PT_OK;
}

int pt_use_any_hit(pt_context* c, int enable)
{
  CTX_CHECK(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));  // frames already handed over keep the mode they were given
  const bool on = enable != 0;
  if(on == c->anyHit)
    return PT_OK;
  c->anyHit = on;
  if(!c->haveScene)
    return PT_OK;
  int rc = upload_instances(c);
  if(rc != PT_OK)
    return rc;
  refresh_scene_ptrs(c);
  if(c->haveAccel || c->accelStale)
  {  // the opaque / non-opaque classification is baked into the triangle records: rebuild, like useAnyHit re-creates the pipeline
    c->haveAccel = false;
    return pt_build_accel(c);
  }
  return PT_OK;
}


int pt_set_accel_mode(pt_context* c, int mode)
{
  CTX_CHECK(c);
  if(mode != PT_ACCEL_FLAT && mode != PT_ACCEL_TWO_LEVEL)
    return c->fail(PT_ERR_INVALID, "pt_set_accel_mode: %d", mode);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));  // frames already handed over keep the structure they were given
  if(mode == c->accelMode)
    return PT_OK;
  c->accelMode = mode;
  if(c->haveAccel || c->accelStale)
  {
    c->haveAccel = false;
    return pt_build_accel(c);
  }
  refresh_scene_ptrs(c);
  return PT_OK;
}

int pt_update_instances(pt_context* c, const pt_Node* nodes, uint32_t numNodes)
{
  CTX_CHECK(c);
  if(!c->haveScene)
    return c->fail(PT_ERR_STATE, "pt_update_instances before pt_set_scene");
  if(!nodes || numNodes != c->hInstances.size())
    return c->fail(PT_ERR_INVALID, "pt_update_instances: %u nodes, the scene has %zu", numNodes, c->hInstances.size());
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));  // frames already handed over keep the transforms they were given
  std::vector<InstanceRec> inst = c->hInstances;
  for(uint32_t n = 0; n < numNodes; ++n)
  {
    if(nodes[n].primMesh != inst[n].primMesh)
      return c->fail(PT_ERR_INVALID, "pt_update_instances: node %u changes its primMesh (%d -> %d); only the world matrices may change", n, inst[n].primMesh, nodes[n].primMesh);
    if(!set_instance_transform(inst[n], nodes[n].worldMatrix, inst[n].flags))
      return c->fail(PT_ERR_INVALID, "node %u: singular world matrix", n);
  }
  const std::vector<InstanceRec> before = c->hInstances;
  c->hInstances = inst;
  int rc = upload_instances(c);
  if(rc != PT_OK)
    return rc;
  refresh_scene_ptrs(c);
  if(c->accelStale)  // pt_update_vertices since the build: the bottom-level structures are stale too
    return pt_build_accel(c);
  if(!c->haveAccel)
    return PT_OK;
  if(c->accelMode == PT_ACCEL_TWO_LEVEL)
  {  // refit: the object-space BLASes are untouched, only the instance boxes and the hierarchy over them are redone; the merged world-space
     // structure is rebuilt when one of its instances moved
    auto t0 = std::chrono::steady_clock::now();
    bool mergedMoved = false;
    for(uint32_t i : c->hMerged)
      mergedMoved = mergedMoved || std::memcmp(&before[i].objectToWorld, &c->hInstances[i].objectToWorld, sizeof(Affine)) != 0;
    if(mergedMoved && (rc = build_merged(c)) != PT_OK)
    {
      c->haveAccel = false;
      return rc;
    }
    if((rc = build_tlas(c)) != PT_OK)
    {
      c->haveAccel = false;
      return rc;
    }
    c->msBuild = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    refresh_scene_ptrs(c);
    return PT_OK;
  }
  c->haveAccel = false;  // flat structure: the world-space triangles are baked in
  return pt_build_accel(c);
}

int pt_update_vertices(pt_context* c, uint32_t first, uint32_t num, const pt_VertexAttributes* vertices)
{
  CTX_CHECK(c);
  if(!c->haveScene)
    return c->fail(PT_ERR_STATE, "pt_update_vertices before pt_set_scene");
  if(num == 0)
    return PT_OK;
  if(!vertices)
    return c->fail(PT_ERR_INVALID, "pt_update_vertices: null vertices");
  if(first > c->numVertices || num > c->numVertices - first || sizeof(pt_VertexAttributes) * (size_t(first) + num) > c->dVertices.bytes)  // (the buffer's own size too)
    return c->fail(PT_ERR_INVALID, "pt_update_vertices: vertices %u .. %llu, the scene has %u", first, (unsigned long long)first + num, c->numVertices);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));  // frames already handed over keep the geometry they were given
  HIP_TRY(c, hipMemcpy((char*)c->dVertices.p + sizeof(pt_VertexAttributes) * size_t(first), vertices, sizeof(pt_VertexAttributes) * size_t(num), hipMemcpyHostToDevice));
  for(uint32_t v = 0; v < num; ++v)
    std::memcpy(&c->hPositions[3 * (size_t(first) + v)], vertices[v].position, 12);
  for(size_t p = 0; p < c->primTouched.size(); ++p)
  {
    const uint64_t lo = c->hPrimMeshVerts[2 * p], hi = lo + c->hPrimMeshVerts[2 * p + 1];
    if(lo < uint64_t(first) + num && hi > first)
      c->primTouched[p] = 1;
  }
  if(c->haveAccel)
  {  // the structure no longer describes the vertices: nothing walks it until pt_refit_accel or pt_build_accel
    c->haveAccel  = false;
    c->accelStale = true;
  }
  return PT_OK;
}

int pt_refit_accel(pt_context* c, pt_RefitInfo* out)
{
  CTX_CHECK(c);
  if(out)
    *out = pt_RefitInfo{};
  if(!c->haveScene || !(c->haveAccel || c->accelStale))
    return c->fail(PT_ERR_STATE, "pt_refit_accel: no structure to refit (pt_build_accel first)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  const auto t0 = std::chrono::steady_clock::now();
  pt_RefitInfo info{};
#if PT_BVH_WIDTH != 4
  {  // the refit works on the 4-wide nodes: other widths rebuild
    const int rc = pt_build_accel(c);
    info.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if(out)
      *out = info;
    return rc;
  }
#else
  const bool two = c->accelMode == PT_ACCEL_TWO_LEVEL;
  // the hierarchies that are kept: their node ranges and where their leaf slots' triangles come from
  std::vector<uint32_t> ranges;
  std::vector<RfSlots>  slots;
  uint32_t              numNodes = c->numWideNodes, numSlots = c->numTris;
  if(!two)
  {
    if(c->numTris)
    {
      ranges = {0u, c->numWideNodes};
      slots.push_back(RfSlots{0u, c->numTris, RF_WORLD, 0u, 0u});
    }
  }
  else
  {
    numNodes = c->nodeCapacity;
    numSlots = c->mergedTris;
    if(c->mergedTris)
    {
      ranges = {0u, c->mergedWide};
      slots.push_back(RfSlots{0u, c->mergedTris, RF_WORLD, 0u, 0u});
    }
    for(const PtBlasDesc& d : c->hBlas)
    {
      ranges.push_back(d.nodeBase);
      ranges.push_back(d.numWide);
      slots.push_back(RfSlots{d.slotBase, d.triCount, RF_VERTEX, d.vertexOffset, d.firstIndex});
      numSlots = std::max(numSlots, d.slotBase + d.triCount);
    }
  }
  // from here on a failure leaves no structure: the boxes may be half written
  c->haveAccel  = false;
  c->accelStale = false;
  int rc;
  if(!slots.empty())
  {
    char                msg[256] = "";
    const uint32_t      numRanges = uint32_t(ranges.size() / 2);
    std::vector<float>  rootBox(6 * size_t(numRanges), 0.f);
    if(!c->haveRefitTable)
    {  // once per build: the parent table, and the cost of the tree as built
      if((rc = dev_alloc(c, c->dRefit, pt_refit_table_bytes(numNodes, numSlots, numRanges, uint32_t(slots.size())))) != PT_OK)
        return rc;
      double measured[2] = {0, 0};
      if(pt_refit_prepare(c->stream, c->dRefit.p, ranges.data(), numRanges, slots.data(), uint32_t(slots.size()), numNodes, numSlots, (const WideNode*)c->dWide.p, c->refit,
                          two ? (c->mergedTris ? 1u : 0u) : numRanges, measured, msg, sizeof(msg)) != 0)
        return c->fail(PT_ERR_HIP, "pt_refit_accel: %s", msg);
      c->costBuilt[0] = measured[0];
      if(!c->haveCostBlas)  // (kept across a rebuild of the merged structure alone: earlier refits may have changed the BLASes' boxes)
        c->costBuilt[1] = measured[1];
      c->haveCostBlas = true;
      c->haveRefitTable = true;
    }
    if(pt_refit_run(c->stream, c->refit, (const InstanceRec*)c->dInstances.p, (const float4*)c->dVertices.p, (const uint32_t*)c->dIndices.p, (TriRec*)c->dTris.p, (AlphaRec*)c->dAlphaRecs.p,
                    (WideNode*)c->dWide.p, rootBox.data(), &info.costAfter, msg, sizeof(msg)) != 0)
      return c->fail(PT_ERR_HIP, "pt_refit_accel: %s", msg);
    info.costBefore = c->costBuilt[0] + c->costBuilt[1];
    for(size_t r = 0; r < numRanges; ++r)
      info.nodesWritten += ranges[2 * r + 1];
    for(const RfSlots& s : slots)
      info.slotsWritten += s.count;
    if(!two)
    {  // world bounds = the union of the root's slots (what bounds_from_root takes from the binary root), then the forms made from the nodes and records
      for(int k = 0; k < 3; ++k)
      {
        const float mn = rootBox[k], mx = rootBox[3 + k];
        c->scene.boundsMin[k]    = std::isfinite(mn) ? mn : 0.f;
        c->scene.boundsInvExt[k] = (std::isfinite(mx - mn) && mx > mn) ? 1.0f / (mx - mn) : 0.f;
      }
      build_cnodes(c, c->numWideNodes);
      build_shade_tris(c, c->numTris);
      dev_free(c->dBvh);  // the binary nodes describe the old vertices
    }
    else if(c->mergedTris)
      std::memcpy(c->mergedBox, rootBox.data(), sizeof(c->mergedBox));
  }
  if(two)
  {  // the per-mesh bounds of the ray transform's padding, then the instance boxes and the hierarchy over them as after pt_update_instances
     // (build_tlas makes the compact nodes of the bottom-level ranges again as well)
    refresh_prim_bounds(c);
    if((rc = build_tlas(c)) != PT_OK)
      return rc;
  }
  HIP_TRY(c, sync_all(c));
  c->haveAccel   = true;
  c->warmPending = true;
  refresh_scene_ptrs(c);
  info.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if(out)
    *out = info;
  return PT_OK;
#endif
}

}  // extern "C"
