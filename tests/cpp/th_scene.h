// The scene of the host harness (test infrastructure; tests/host_harness.py builds it): the PRODUCT's headers compiled for the host, and the
// acceleration structures they walk, assembled on the host in the product's formats (TriRec, WideNode, TlasLeaf, CompactNode).
//
// Topology comes from the product's device builder run through its host emulation (pt_debug_sahdev_topology in libptmi.so); boxes, the 4-wide
// collapse, the vertex form of BLAS leaves and the TLAS proxies restate pt_accel.hip (k_gather's tri_box, k_collapse, k_blas_vertex_form,
// k_instance_proxies).  The restated stages are held, node by node, to the same auditor as the device's own arrays (tests/accel_audit.py through
// th_accel_read; tests/test_accel_audit.py), so a walk test that passes here passes on a structure with the invariants DESIGN.md "What the build
// guarantees" lists.  build_structures at the end of this file spells out the stages.
#pragma once
#include "th_shims.h"
#include "pt_shade.h"    // pt_settle.h (pt_trace.h + the per-ray settle functions k_tail runs) + the shading steps of a path (generate_ray, shade_path, ...)
#include "pt_machine.h"  // the resumable per-lane traversal of the persistent kernels (k_closest_p / k_shadow_p)
#include "pt_cnode.h"    // WideNode -> CompactNode (what pt_accel.hip k_compact_nodes runs per node)
#include "../../include/pt_types.h"

extern "C" int pt_debug_sahdev_topology(uint32_t n, const float* tri9, uint32_t* vals, uint32_t* childL, uint32_t* childR, uint32_t* parI, uint32_t* parL);

// build options of th_create / th_create_scene (tests/host_harness.py MERGE_SINGLES / COMPACT_NODES)
enum : uint32_t {
  TH_MERGE_SINGLES = 1u,  // PT_TUNE mergeSingles (pt_internal.h), the product's default: prim-meshes instantiated once share one world-space structure
  TH_COMPACT_NODES = 2u,  // PT_TUNE cnodes: the machine walks read the 80-byte form of the nodes
};

struct Box {
  float lo[3], hi[3];
  bool  alpha;
};
struct Bvh {
  std::vector<TriRec>   tris;   // leaf order
  std::vector<WideNode> wide;   // node 0 = root
  float                 lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  // the binary tree the wide nodes were collapsed from (experiments/step_model.cpp re-collapses it at other widths)
  std::vector<uint32_t> cl, cr;
  std::vector<Box>      leafBox, innerBox;
};

// pt_accel.hip tri_box: padded box of a record (p0, p0 + e1, p0 + e2)
inline void tri_box_h(const TriRec& r, float lo[3], float hi[3])
{
  const float p0[3] = {r.p0w.x, r.p0w.y, r.p0w.z};
  const float p1[3] = {r.p0w.x + r.e1n.x, r.p0w.y + r.e1n.y, r.p0w.z + r.e1n.z};
  const float p2[3] = {r.p0w.x + r.e2p.x, r.p0w.y + r.e2p.y, r.p0w.z + r.e2p.z};
  for(int a = 0; a < 3; ++a)
  {
    lo[a] = std::fmin(p0[a], std::fmin(p1[a], p2[a]));
    hi[a] = std::fmax(p0[a], std::fmax(p1[a], p2[a]));
    const float m = std::fmax(std::fabs(lo[a]), std::fabs(hi[a])), pad = m * 4e-6f + 1e-30f;
    lo[a] -= pad;
    hi[a] += pad;
  }
}

inline float half_area_h(const Box& b)
{
  const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
  return dx * dy + dy * dz + dz * dx;
}

// the collapse rule (k_collapse): the children of binary node `node`, then the inner child of largest area opened until there are `width`
inline int open_children(const std::vector<uint32_t>& cl, const std::vector<uint32_t>& cr, const std::vector<Box>& inner, uint32_t node, int width, uint32_t* id)
{
  int cnt   = 0;
  id[cnt++] = cl[node];
  id[cnt++] = cr[node];
  while(cnt < width)
  {
    int   best = -1;
    float bestA = -1.f;
    for(int k = 0; k < cnt; ++k)
      if(!(id[k] & BVH_LEAF) && half_area_h(inner[id[k]]) > bestA)
      {
        bestA = half_area_h(inner[id[k]]);
        best  = k;
      }
    if(best < 0)
      break;
    const uint32_t open = id[best];
    id[best]            = id[cnt - 1];
    --cnt;
    id[cnt++] = cl[open];
    id[cnt++] = cr[open];
  }
  return cnt;
}

// records (edge form, flags in p0w.w >> 29) -> leaf order + 4-wide nodes (k_gather, k_refit, k_emit, k_collapse)
inline Bvh build_bvh(const std::vector<TriRec>& in)
{
  Bvh            out;
  const uint32_t n = uint32_t(in.size());
  if(n == 0)
    return out;
  std::vector<uint32_t> vals(n), cl(n), cr(n), pi(n), pl(n);
  if(n >= 2)
  {
    std::vector<float> tri9(size_t(n) * 9);
    for(uint32_t i = 0; i < n; ++i)
    {
      const float v[9] = {in[i].p0w.x, in[i].p0w.y, in[i].p0w.z, in[i].e1n.x, in[i].e1n.y, in[i].e1n.z, in[i].e2p.x, in[i].e2p.y, in[i].e2p.z};
      std::memcpy(&tri9[size_t(i) * 9], v, sizeof(v));
    }
    if(pt_debug_sahdev_topology(n, tri9.data(), vals.data(), cl.data(), cr.data(), pi.data(), pl.data()) != 0)
      return out;
  }
  else
    vals[0] = 0;
  out.tris.resize(n);
  std::vector<Box> leaf(n), inner(n > 1 ? n - 1 : 1);
  for(uint32_t i = 0; i < n; ++i)
  {
    out.tris[i] = in[vals[i]];
    tri_box_h(out.tris[i], leaf[i].lo, leaf[i].hi);
    leaf[i].alpha = !((__float_as_uint(out.tris[i].p0w.w) >> 29) & TRI_OPAQUE);
  }
  auto ref_box = [&](uint32_t r) -> const Box& { return (r & BVH_LEAF) ? leaf[r & ~BVH_LEAF] : inner[r]; };
  if(n >= 2)
  {  // boxes bottom-up: a subtree over k leaves owns k-1 consecutive ids starting at its root, so children have larger ids than parents
    for(uint32_t k = n - 1; k-- > 0;)
    {
      const Box &a = ref_box(cl[k]), &b = ref_box(cr[k]);
      for(int x = 0; x < 3; ++x)
      {
        inner[k].lo[x] = std::fmin(a.lo[x], b.lo[x]);
        inner[k].hi[x] = std::fmax(a.hi[x], b.hi[x]);
      }
      inner[k].alpha = a.alpha || b.alpha;
    }
  }
  auto child_ref = [&](uint32_t r) -> uint32_t {
    if(r & BVH_LEAF)
      return BVH_LEAF | (r & ~BVH_LEAF) | (leaf[r & ~BVH_LEAF].alpha ? BVH_ALPHA : 0u);
    return r;
  };
  // collapse: per wide node, open_children until 4 children
  struct Item { uint32_t b2, wide; };
  std::vector<Item> queue{{0u, 0u}};
  out.wide.resize(1);
  for(size_t qi = 0; qi < queue.size(); ++qi)
  {
    const Item it = queue[qi];
    uint32_t   id[4];
    int        cnt = 0;
    if(n == 1)
      id[cnt++] = BVH_LEAF | 0u;
    else
      cnt = open_children(cl, cr, inner, it.b2, 4, id);
    WideNode w;
    std::memset(&w, 0, sizeof(w));
    float*    mnx = &w.minx[0].x; float* mny = &w.miny[0].x; float* mnz = &w.minz[0].x;
    float*    mxx = &w.maxx[0].x; float* mxy = &w.maxy[0].x; float* mxz = &w.maxz[0].x;
    uint32_t* ch  = &w.child[0].x;
    for(int k = 0; k < 4; ++k)
    {
      if(k < cnt)
      {
        const Box& b = ref_box(id[k]);
        mnx[k] = b.lo[0]; mny[k] = b.lo[1]; mnz[k] = b.lo[2]; mxx[k] = b.hi[0]; mxy[k] = b.hi[1]; mxz[k] = b.hi[2];
        if(id[k] & BVH_LEAF)
          ch[k] = child_ref(id[k]);
        else
        {
          const uint32_t wid = uint32_t(out.wide.size());
          out.wide.emplace_back();
          queue.push_back({id[k], wid});
          ch[k] = wid | (inner[id[k]].alpha ? BVH_ALPHA : 0u);
        }
      }
      else
      {
        mnx[k] = mny[k] = mnz[k] = FLT_MAX;
        mxx[k] = mxy[k] = mxz[k] = -FLT_MAX;
        ch[k]                    = BVH_NONE;
      }
    }
    out.wide[it.wide] = w;
  }
  const Box& root = n >= 2 ? inner[0] : leaf[0];
  for(int a = 0; a < 3; ++a)
  {
    out.lo[a] = root.lo[a];
    out.hi[a] = root.hi[a];
  }
  out.cl = cl; out.cr = cr; out.leafBox = leaf; out.innerBox = inner;
  return out;
}

struct InstIn {
  uint32_t vertexOffset, firstIndex, triCount, flags;  // flags: TRI_OPAQUE / TRI_NOCULL (TRI_FLIP is derived from the matrix)
  int32_t  primMesh;
  float    worldMatrix[16];  // column-major
};

struct Scene {
  std::vector<float4>      vertices;  // 2 x float4 per vertex
  std::vector<uint32_t>    indices;
  std::vector<InstanceRec> inst;
  std::vector<float>       pad;       // per instance padC0, padC1: the box padding of its TLAS leaf (pt_scene_records.cpp two_level_pad)
  uint32_t                 numPrimMeshes = 0, options = TH_MERGE_SINGLES;
  std::vector<uint32_t>    instTriBase;
  std::vector<TriRec>      world;     // world index order (brute force)
  Bvh                      flat;
  std::vector<AlphaRec>    flatAlpha;
  // two-level
  std::vector<TriRec>      blasTris;
  std::vector<AlphaRec>    blasAlpha;
  std::vector<WideNode>    blasWide;
  Bvh                      tlas;
  std::vector<TlasLeaf>    tlasLeaves;
  std::vector<uint32_t>    instBlock;  // DeviceScene::instBlock (pt_capi_accel.hip build_tlas)
  std::vector<CompactNode> flatCNodes, blasCNodes, tlasCNodes;  // TH_COMPACT_NODES: the nodes in the compact form (read by lane_inner only)
  bool                     compactOk = false;  // ... and every node of the three structures could be encoded
  // what th_accel_info / th_accel_read report of the two-level build (pt_accel_dump.h)
  std::vector<uint32_t>    instNodeBase, blasRanges, mergedList;
  uint32_t                 mergedTris = 0, mergedWide = 0, numActive = 0;
  float                    mergedBox[6] = {0, 0, 0, 0, 0, 0};
  std::vector<AlphaMat>    alphaMats;   // th_create_scene: the product's own records (pt_debug_scene_records)
  std::vector<uint32_t>    alphaMaps, texels;
  std::vector<TexRec>      texRecs;
  std::vector<uint4>       matLines;  // per material its 128-byte line (pt_device.h mat_line_pack)
  std::vector<pt_GltfShadeMaterial> materials;
  std::vector<pt_Light>    lights;
  std::vector<float4>      env;
  std::vector<pt_EnvAccel> envAccel;
  DeviceScene              dsFlat, dsTwo;
};

inline f3 vpos(const Scene& s, uint32_t v) { const float4 a = s.vertices[size_t(v) * 2]; return f3{a.x, a.y, a.z}; }

// k_world_tris (trace contract T1)
inline TriRec world_record(const Scene& s, const InstanceRec& I, uint32_t inst, uint32_t k, uint32_t w)
{
  const uint32_t* t  = &s.indices[I.firstIndex + 3 * size_t(k)];
  const f3        p0 = xform_point(I.objectToWorld, vpos(s, I.vertexOffset + t[0])), p1 = xform_point(I.objectToWorld, vpos(s, I.vertexOffset + t[1])),
           p2 = xform_point(I.objectToWorld, vpos(s, I.vertexOffset + t[2]));
  const f3 e1 = p1 - p0, e2 = p2 - p0;
  TriRec   r;
  r.p0w = make_float4(p0.x, p0.y, p0.z, __uint_as_float(w | (I.flags << 29)));
  r.e1n = make_float4(e1.x, e1.y, e1.z, __uint_as_float(inst));
  r.e2p = make_float4(e2.x, e2.y, e2.z, __uint_as_float(k));
  return r;
}


// any-hit inputs of triangle k of instance I (k_world_tris): raw texcoords of the three vertices + material
inline AlphaRec alpha_record(const Scene& s, const InstanceRec& I, uint32_t k)
{
  const uint32_t* t = &s.indices[I.firstIndex + 3 * size_t(k)];
  const float4    b0 = s.vertices[size_t(I.vertexOffset + t[0]) * 2 + 1], b1 = s.vertices[size_t(I.vertexOffset + t[1]) * 2 + 1], b2 = s.vertices[size_t(I.vertexOffset + t[2]) * 2 + 1];
  AlphaRec        ar;
  ar.uv0[0] = b0.x; ar.uv0[1] = b0.y; ar.uv1[0] = b1.x; ar.uv1[1] = b1.y; ar.uv2[0] = b2.x; ar.uv2[1] = b2.y;
  ar.material = uint32_t(I.materialIndex < 0 ? 0 : I.materialIndex);
  ar._pad     = 0;
  return ar;
}

// ---- the stages of build_structures, in the order it runs them ----------------------------------------------------------------------------------
// what the two-level stages hand to each other
struct TwoLevelPlan {
  std::vector<char>    isMerged;    // per instance: its triangles live in the merged world-space structure
  bool                 haveMerged = false;
  float                mlo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mhi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};  // root box of the merged structure
  std::vector<int64_t> nodeBaseOf;  // per prim-mesh: first node of its BLAS, -1 without one
};

// flat: world records of every instance, one hierarchy
inline void build_flat(Scene* s)
{
  const uint32_t numInst  = uint32_t(s->inst.size());
  uint32_t       triTotal = 0;
  s->instTriBase.assign(numInst ? numInst : 1, 0u);
  for(uint32_t i = 0; i < numInst; ++i)
  {
    s->instTriBase[i] = s->inst[i].triBase;
    triTotal += s->inst[i].triCount;
  }
  s->world.reserve(triTotal);
  for(uint32_t i = 0; i < numInst; ++i)
    for(uint32_t k = 0; k < s->inst[i].triCount; ++k)
      s->world.push_back(world_record(*s, s->inst[i], i, k, s->inst[i].triBase + k));
  s->flat = build_bvh(s->world);
  s->flatAlpha.assign(std::max<size_t>(1, s->flat.tris.size()), AlphaRec{});
  for(size_t i = 0; i < s->flat.tris.size(); ++i)
    s->flatAlpha[i] = alpha_record(*s, s->inst[__float_as_uint(s->flat.tris[i].e1n.w)], __float_as_uint(s->flat.tris[i].e2p.w));
}

// two-level: the prim-meshes instantiated once share one world-space structure at slot 0 / node 0 (pt_capi_accel.hip build_merged / pt_accel.hip
// pt_merged_build)
inline void build_merged_singles(Scene* s, TwoLevelPlan& plan)
{
  const uint32_t        numInst = uint32_t(s->inst.size());
  std::vector<uint32_t> uses(s->numPrimMeshes, 0);
  for(uint32_t i = 0; i < numInst; ++i)
    if(s->inst[i].triCount)
      uses[s->inst[i].primMesh]++;
  std::vector<TriRec> mw;
  for(uint32_t i = 0; i < numInst; ++i)
    if(s->inst[i].triCount && uses[s->inst[i].primMesh] == 1)
    {
      plan.isMerged[i] = 1;
      for(uint32_t k = 0; k < s->inst[i].triCount; ++k)
        mw.push_back(world_record(*s, s->inst[i], i, k, s->inst[i].triBase + k));
    }
  if(mw.empty())
    return;
  plan.haveMerged = true;
  Bvh b           = build_bvh(mw);
  for(const TriRec& r : b.tris)
  {
    s->blasTris.push_back(r);
    s->blasAlpha.push_back(alpha_record(*s, s->inst[__float_as_uint(r.e1n.w)], __float_as_uint(r.e2p.w)));
    float lo[3], hi[3];
    tri_box_h(r, lo, hi);  // the root box of the structure is the union of its padded leaf boxes
    for(int a = 0; a < 3; ++a)
    {
      plan.mlo[a] = std::fmin(plan.mlo[a], lo[a]);
      plan.mhi[a] = std::fmax(plan.mhi[a], hi[a]);
    }
  }
  for(const WideNode& w : b.wide)
    s->blasWide.push_back(w);  // slot base and node base are 0: the references are already global
}

// ... and one object-space BLAS per other prim-mesh that is instantiated (pt_capi_accel.hip build_two_level / pt_accel.hip pt_blas_build)
inline void build_blases(Scene* s, TwoLevelPlan& plan)
{
  for(uint32_t i = 0; i < uint32_t(s->inst.size()); ++i)
  {
    const InstanceRec& I = s->inst[i];
    if(I.triCount == 0 || plan.isMerged[i] || plan.nodeBaseOf[I.primMesh] >= 0)
      continue;
    InstanceRec P = I;  // the pseudo-instance: identity transform, no TRI_FLIP
    P.objectToWorld.r0 = make_float4(1, 0, 0, 0); P.objectToWorld.r1 = make_float4(0, 1, 0, 0); P.objectToWorld.r2 = make_float4(0, 0, 1, 0);
    P.flags &= ~TRI_FLIP;
    std::vector<TriRec> obj(I.triCount);
    for(uint32_t k = 0; k < I.triCount; ++k)
      obj[k] = world_record(*s, P, 0, k, k);
    Bvh            b        = build_bvh(obj);
    const uint32_t nodeBase = uint32_t(s->blasWide.size()), slotBase = uint32_t(s->blasTris.size());
    for(TriRec r : b.tris)
    {  // vertex form (k_blas_vertex_form)
      const uint32_t  k = __float_as_uint(r.e2p.w);
      const uint32_t* t = &s->indices[I.firstIndex + 3 * size_t(k)];
      const f3        v0 = vpos(*s, I.vertexOffset + t[0]), v1 = vpos(*s, I.vertexOffset + t[1]), v2 = vpos(*s, I.vertexOffset + t[2]);
      r.p0w = make_float4(v0.x, v0.y, v0.z, __uint_as_float(k));
      r.e1n = make_float4(v1.x, v1.y, v1.z, 0.f);
      r.e2p = make_float4(v2.x, v2.y, v2.z, 0.f);
      s->blasTris.push_back(r);
      s->blasAlpha.push_back(alpha_record(*s, I, k));
    }
    for(WideNode w : b.wide)
    {  // global references (k_blas_rebase)
      uint32_t* ch = &w.child[0].x;
      for(int k = 0; k < 4; ++k)
        if(ch[k] != BVH_NONE)
          ch[k] = (ch[k] & ~BVH_SLOT_MASK) | ((ch[k] & BVH_SLOT_MASK) + ((ch[k] & BVH_LEAF) ? slotBase : nodeBase));
      s->blasWide.push_back(w);
    }
    plan.nodeBaseOf[I.primMesh] = nodeBase;
  }
  if(s->blasAlpha.empty())
    s->blasAlpha.emplace_back();
}

// TLAS over the exact world boxes of the instances (k_instance_proxies), as "diagonal" records, and its leaves
inline void build_tlas(Scene* s, const TwoLevelPlan& plan)
{
  std::vector<TriRec> prox;
  for(uint32_t i = 0; i < uint32_t(s->inst.size()); ++i)
  {
    const InstanceRec& I = s->inst[i];
    if(I.triCount == 0 || plan.isMerged[i])
      continue;
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for(uint32_t j = 0; j < 3 * I.triCount; ++j)
    {
      const f3    p    = xform_point(I.objectToWorld, vpos(*s, I.vertexOffset + s->indices[I.firstIndex + j]));
      const float q[3] = {p.x, p.y, p.z};
      for(int a = 0; a < 3; ++a)
      {
        lo[a] = std::fmin(lo[a], q[a]);
        hi[a] = std::fmax(hi[a], q[a]);
      }
    }
    TriRec r;
    r.p0w = make_float4(lo[0], lo[1], lo[2], __uint_as_float(i | (I.flags << 29)));
    r.e1n = make_float4(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2], 0.f);
    r.e2p = make_float4(0.f, 0.f, 0.f, 0.f);
    prox.push_back(r);
  }
  if(plan.haveMerged)
  {  // the merged structure's proxy (pt_tlas_build): its root box, opaque when every merged triangle is
    bool opaque = true;
    for(uint32_t i = 0; i < uint32_t(s->inst.size()); ++i)
      opaque = opaque && (!plan.isMerged[i] || (s->inst[i].flags & TRI_OPAQUE));
    TriRec r;
    r.p0w = make_float4(plan.mlo[0], plan.mlo[1], plan.mlo[2], __uint_as_float(TRI_INDEX_MASK | (opaque ? TRI_OPAQUE << 29 : 0u)));
    r.e1n = make_float4(plan.mhi[0] - plan.mlo[0], plan.mhi[1] - plan.mlo[1], plan.mhi[2] - plan.mlo[2], 0.f);
    r.e2p = make_float4(0.f, 0.f, 0.f, 0.f);
    prox.push_back(r);
  }
  s->tlas = build_bvh(prox);
  for(const TriRec& r : s->tlas.tris)
  {
    const uint32_t id = __float_as_uint(r.p0w.w) & TRI_INDEX_MASK;
    TlasLeaf       l;
    std::memset(&l, 0, sizeof(l));
    if(id == TRI_INDEX_MASK)
    {
      l.inst = PT_INST_MERGED;
      s->tlasLeaves.push_back(l);
      continue;
    }
    l.inst     = id;
    l.nodeBase = uint32_t(plan.nodeBaseOf[s->inst[id].primMesh]);
    l.wflags   = s->inst[id].triBase | (s->inst[id].flags << 29);
    l.padC0    = s->pad[2 * id];
    l.padC1    = s->pad[2 * id + 1];
    s->tlasLeaves.push_back(l);
  }
  if(s->tlasLeaves.empty())
    s->tlasLeaves.emplace_back();
}

// the scene records the walk reads, once per structure
inline void bind_device_scenes(Scene* s)
{
  if(s->alphaMats.empty())
  {
    AlphaMat m;
    std::memset(&m, 0, sizeof(m));
    m.factorA = 1.0f; m.tex = -1; m.mapOffset = ALPHA_NO_MAP;
    s->alphaMats.push_back(m);
  }
  if(s->alphaMaps.empty())
    s->alphaMaps.push_back(0u);
  if(s->texels.empty())
    s->texels.push_back(0xffffffffu);
  const uint32_t triTotal = uint32_t(s->world.size());
  DeviceScene    d;
  std::memset(&d, 0, sizeof(d));
  d.vertices = s->vertices.data(); d.indices = s->indices.data(); d.instances = s->inst.data();
  d.alphaMats = s->alphaMats.data(); d.alphaMaps = s->alphaMaps.data(); d.texels = s->texels.data();
  d.materials = s->materials.empty() ? nullptr : s->materials.data(); d.lights = s->lights.empty() ? nullptr : s->lights.data();
  d.texRecs = s->texRecs.empty() ? nullptr : s->texRecs.data();
  d.matLines = s->matLines.empty() ? nullptr : s->matLines.data();
  d.numTris = triTotal; d.numInstances = uint32_t(s->inst.size());
  s->dsFlat           = d;
  s->dsFlat.wide      = s->flat.wide.data();
  s->dsFlat.tris      = s->flat.tris.data();
  s->dsFlat.alphaRecs = s->flatAlpha.data();
  s->dsTwo             = d;
  s->dsTwo.wide        = s->blasWide.data();
  s->dsTwo.tris        = s->blasTris.data();
  s->dsTwo.alphaRecs   = s->blasAlpha.data();
  s->dsTwo.tlas        = s->tlas.wide.data();
  s->dsTwo.tlasLeaves  = s->tlasLeaves.data();
  s->dsTwo.instTriBase = s->instTriBase.data();
  s->dsTwo.twoLevel    = 1;
  const size_t entries = (size_t(triTotal) >> PT_INST_BLOCK_SHIFT) + 2;
  s->instBlock.assign(entries, 0u);
  uint32_t at = 0;
  for(size_t e = 0; e < entries; ++e)
  {
    const uint64_t first = uint64_t(e) << PT_INST_BLOCK_SHIFT;
    while(at + 1 < s->instTriBase.size() && uint64_t(s->instTriBase[at + 1]) <= first)
      ++at;
    s->instBlock[e] = at;
  }
  s->dsTwo.instBlock = s->instBlock.data();
}

// TH_COMPACT_NODES: the nodes of the three structures in the 80-byte form.  A structure is walked on them only if every node of it could be
// encoded, the two-level structure only if the flat one's could too
inline void encode_compact_nodes(Scene* s)
{
  auto encode = [](const std::vector<WideNode>& wide, std::vector<CompactNode>& cn) {
    bool ok = true;
    cn.resize(wide.size());
    for(size_t i = 0; i < wide.size(); ++i)
      ok = cn_encode(wide[i], cn[i]) && ok;
    return ok;
  };
  s->compactOk = encode(s->flat.wide, s->flatCNodes);
  if(!s->compactOk)
    return;
  s->dsFlat.cnodes = s->flatCNodes.data();
  const bool okBlas = encode(s->blasWide, s->blasCNodes), okTlas = encode(s->tlas.wide, s->tlasCNodes);
  s->compactOk      = okBlas && okTlas;
  if(s->compactOk && !s->blasCNodes.empty() && !s->tlasCNodes.empty())
  {
    s->dsTwo.cnodes = s->blasCNodes.data();
    s->dsTwo.ctlas  = s->tlasCNodes.data();
  }
}

// flat + two-level structures over s->inst, s->pad, s->numPrimMeshes and s->options (already filled)
inline void build_structures(Scene* s)
{
  build_flat(s);
  TwoLevelPlan plan;
  plan.isMerged.assign(s->inst.size(), 0);
  plan.nodeBaseOf.assign(s->numPrimMeshes, -1);
  if(s->options & TH_MERGE_SINGLES)
    build_merged_singles(s, plan);
  build_blases(s, plan);
  build_tlas(s, plan);
  bind_device_scenes(s);
  // the tables of the read-back: node base per instance from the plan, BLAS ranges from the bases (a BLAS ends where the next one starts)
  s->instNodeBase.assign(s->inst.size(), 0u);
  for(uint32_t i = 0; i < uint32_t(s->inst.size()); ++i)
  {
    if(plan.isMerged[i])
      s->mergedList.push_back(i);
    else if(s->inst[i].triCount)
    {
      s->instNodeBase[i] = uint32_t(plan.nodeBaseOf[s->inst[i].primMesh]);
      ++s->numActive;
    }
  }
  std::vector<uint32_t> bases;
  for(int64_t b : plan.nodeBaseOf)
    if(b >= 0)
      bases.push_back(uint32_t(b));
  std::sort(bases.begin(), bases.end());
  for(size_t k = 0; k < bases.size(); ++k)
  {
    s->blasRanges.push_back(bases[k]);
    s->blasRanges.push_back((k + 1 < bases.size() ? bases[k + 1] : uint32_t(s->blasWide.size())) - bases[k]);
  }
  if(plan.haveMerged)
  {
    for(uint32_t i : s->mergedList)
      s->mergedTris += s->inst[i].triCount;
    s->mergedWide = bases.empty() ? uint32_t(s->blasWide.size()) : bases[0];
    for(int a = 0; a < 3; ++a)
    {
      s->mergedBox[a]     = plan.mlo[a];
      s->mergedBox[3 + a] = plan.mhi[a];
    }
  }
  if(s->options & TH_COMPACT_NODES)
    encode_compact_nodes(s);
}
