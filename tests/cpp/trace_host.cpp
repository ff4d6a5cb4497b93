// CPU harness around the PRODUCT's traversal source (test infrastructure; tests/host_harness.py builds it into libtracehost.so together with
// render_host.cpp, probe_host.cpp, query_host.cpp and handover_host.cpp).  This unit: scene creation, th_candidates and th_settle.
//
// vk_raytrace_amd/csrc/pt_trace.h -- traverse<MODE, TWO>, wide_node_step, make_raybox, enter_instance, world_tri, tri_test -- is plain
// inline C++ apart from a handful of intrinsics (th_shims.h), so it is compiled here for the host (g++, -ffp-contract=off like the device build)
// and run against a brute-force loop over every world triangle with the same tri_test.  What the GPU parity tests can only show through images is
// checked ray by ray without a GPU: the flat walk and the two-level walk (TLAS + object-space BLASes, per-instance box padding from
// pt_scene_records.cpp's two_level_pad) must report exactly the candidates brute force reports -- every candidate along the ray, in key order.
// The structures are assembled by th_scene.h; the walk context, the parallel loop and the machine leg are th_walk.h's.
#include "th_walk.h"
#include "pt_accel_dump.h"

extern "C" int pt_debug_two_level_pad(const float* worldMatrix16, float Bo, float* out27);
extern "C" int pt_debug_mat_lines(const pt_SceneDesc* d, void* linesOut, char* err, size_t errLen);
extern "C" int pt_debug_scene_records(const pt_SceneDesc* d, unsigned long long* counts5, void* instOut, float* padOut, void* alphaMatsOut, uint32_t* alphaMapsOut, uint32_t* texelsOut,
                                      void* texRecsOut, char* err, size_t errLen);

static std::atomic<unsigned long long> g_spHist[65];  // machine walks of th_settle: rays by the deepest traversal-stack level they used

extern "C" {

void th_take_sp_hist(unsigned long long* out65) { for(int i = 0; i < 65; ++i) out65[i] = g_spHist[i].exchange(0); }

// Number of (node, child, axis, side) planes of the compact nodes that lie INSIDE the fp32 box they stand for, evaluated in double (must be 0: the
// decoded box has to enclose the original), plus the nodes whose child references differ; also reports how loose the boxes are.
unsigned long long th_cnode_violations(void* p, double* meanExtraExtent)
{
  const Scene*       s     = static_cast<const Scene*>(p);
  unsigned long long bad   = 0;
  double             extra = 0.0;
  unsigned long long n     = 0;
  auto check = [&](const std::vector<WideNode>& wide, const std::vector<CompactNode>& cn) {
    for(size_t i = 0; i < wide.size() && i < cn.size(); ++i)
    {
      const WideNode&    w = wide[i];
      const CompactNode& c = cn[i];
      const float*    lo[3] = {&w.minx[0].x, &w.miny[0].x, &w.minz[0].x};
      const float*    hi[3] = {&w.maxx[0].x, &w.maxy[0].x, &w.maxz[0].x};
      const uint32_t* cc    = &w.child[0].x;
      const uint32_t* cd    = &c.child.x;
      const double    org[3] = {c.px, c.py, c.pz};
      for(int k = 0; k < 4; ++k)
      {
        if(cc[k] != cd[k])
          ++bad;
        if(cc[k] == BVH_NONE)
          continue;
        for(int a = 0; a < 3; ++a)
        {
          const double   step = std::ldexp(1.0, int((c.exps >> (8 * a)) & 0xffu) - 127);
          const uint32_t wl = (&c.ax[a].x)[k >> 1], wh = (&c.ax[a].x)[2 + (k >> 1)];
          const double   ql = cn_plane(wl, k & 1), qh = cn_plane(wh, k & 1);
          const double   dl = org[a] + ql * step, dh = org[a] + qh * step;
          if(dl > double(lo[a][k]) || dh < double(hi[a][k]))
            ++bad;
          const double ext = double(hi[a][k]) - double(lo[a][k]);
          extra += ((dh - dl) - ext) / (step * double(CN_GRID_MAX));  // growth of the child's extent in units of the node's grid extent
          ++n;
        }
      }
    }
  };
  check(s->flat.wide, s->flatCNodes);
  check(s->blasWide, s->blasCNodes);
  check(s->tlas.wide, s->tlasCNodes);
  if(meanExtraExtent)
    *meanExtraExtent = n ? extra / double(n) : 0.0;
  return bad;
}

// 1: the walk of that structure reads compact nodes
int th_compact_in_use(void* p, int two)
{
  const Scene* s = static_cast<const Scene*>(p);
  return two ? (s->dsTwo.cnodes != nullptr && s->dsTwo.ctlas != nullptr) : (s->dsFlat.cnodes != nullptr ? 1 : 0);
}
// 1: the scene was built with TH_COMPACT_NODES and every node of its three structures could be encoded
int th_compact_ok(void* p) { return static_cast<const Scene*>(p)->compactOk ? 1 : 0; }

// plain geometry + per-instance flags (every instance's material is the default: no any-hit evaluation is reachable with TRI_OPAQUE);
// options: TH_MERGE_SINGLES | TH_COMPACT_NODES
void* th_create(const float* vertices8, uint32_t numVerts, const uint32_t* indices, uint32_t numIdx, const InstIn* in, uint32_t numInst, const float* primBound, uint32_t numPrimMeshes,
                uint32_t options)
{
  Scene* s = new Scene();
  s->options       = options;
  s->numPrimMeshes = numPrimMeshes;
  s->vertices.resize(size_t(numVerts) * 2);
  std::memcpy(s->vertices.data(), vertices8, sizeof(float) * 8 * size_t(numVerts));
  s->indices.assign(indices, indices + numIdx);
  s->inst.resize(numInst);
  s->pad.resize(2 * size_t(numInst));
  uint32_t triTotal = 0;
  for(uint32_t i = 0; i < numInst; ++i)
  {
    InstanceRec& I = s->inst[i];
    std::memset(&I, 0, sizeof(I));
    float rec[27];
    if(in[i].primMesh < 0 || uint32_t(in[i].primMesh) >= numPrimMeshes || pt_debug_two_level_pad(in[i].worldMatrix, primBound[in[i].primMesh], rec) != 0)
    {
      delete s;
      return nullptr;
    }
    I.objectToWorld.r0 = make_float4(rec[0], rec[1], rec[2], rec[3]);
    I.objectToWorld.r1 = make_float4(rec[4], rec[5], rec[6], rec[7]);
    I.objectToWorld.r2 = make_float4(rec[8], rec[9], rec[10], rec[11]);
    I.worldToObject.r0 = make_float4(rec[12], rec[13], rec[14], rec[15]);
    I.worldToObject.r1 = make_float4(rec[16], rec[17], rec[18], rec[19]);
    I.worldToObject.r2 = make_float4(rec[20], rec[21], rec[22], rec[23]);
    s->pad[2 * i]      = rec[24];
    s->pad[2 * i + 1]  = rec[25];
    I.vertexOffset = in[i].vertexOffset; I.firstIndex = in[i].firstIndex; I.materialIndex = 0; I.primMesh = in[i].primMesh;
    I.triBase = triTotal; I.triCount = in[i].triCount;
    I.flags   = (in[i].flags & (TRI_OPAQUE | TRI_NOCULL)) | (uint32_t(rec[26]) & TRI_FLIP);
    triTotal += I.triCount;
  }
  build_structures(s);
  return s;
}

// a full scene description (materials, textures): instance records, flags, alpha view, opacity maps and texel pool are the PRODUCT's
// (pt_scene_records.cpp build_scene_records through pt_debug_scene_records), so the any-hit evaluation reads exactly what the GPU reads
void* th_create_scene(const pt_SceneDesc* d, char* err, size_t errLen, uint32_t options)
{
  unsigned long long counts[5] = {0, 0, 0, 0, 0};
  if(pt_debug_scene_records(d, counts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, err, errLen) != 0)
    return nullptr;
  Scene* s = new Scene();
  s->options       = options;
  s->numPrimMeshes = d->numPrimMeshes;
  s->vertices.resize(size_t(d->numVertices) * 2);
  std::memcpy(s->vertices.data(), d->vertices, sizeof(float) * 8 * size_t(d->numVertices));
  s->indices.assign(d->indices, d->indices + d->numIndices);
  s->inst.resize(counts[0]);
  s->alphaMats.resize(counts[1]);
  s->alphaMaps.resize(counts[2]);
  s->texels.resize(counts[3]);
  s->texRecs.resize(d->numTextures ? d->numTextures : 1);
  s->materials.assign(d->materials, d->materials + d->numMaterials);
  s->lights.assign(d->lights, d->lights + d->numLights);
  if(s->lights.empty())
    s->lights.emplace_back();
  s->pad.resize(2 * counts[0] + 2);
  if(pt_debug_scene_records(d, counts, s->inst.data(), s->pad.data(), s->alphaMats.data(), s->alphaMaps.data(), s->texels.data(), s->texRecs.data(), err, errLen) != 0)
  {
    delete s;
    return nullptr;
  }
  s->matLines.assign(size_t(PT_MAT_LINE_QUADS) * std::max<size_t>(1, s->materials.size()), uint4{0u, 0u, 0u, 0u});
  if(pt_debug_mat_lines(d, s->matLines.data(), err, errLen) != 0)  // the product's own lines: their descriptors point into the pool fetched above (plain copies + interleaved groups)
  {
    delete s;
    return nullptr;
  }
  build_structures(s);
  return s;
}

void th_destroy(void* p) { delete static_cast<Scene*>(p); }

uint32_t th_num_tris(void* p) { return uint32_t(static_cast<Scene*>(p)->world.size()); }
void     th_sizes(void* p, uint32_t* out4)
{
  Scene* s = static_cast<Scene*>(p);
  out4[0] = uint32_t(s->flat.wide.size()); out4[1] = uint32_t(s->blasWide.size()); out4[2] = uint32_t(s->tlas.wide.size()); out4[3] = uint32_t(s->blasTris.size());
}
// world record of triangle w (p0, e1, e2: 9 floats) and its flags -- for the test's double-precision re-evaluation of a disputed candidate
void th_world_tri(void* p, uint32_t w, float* out9, uint32_t* flags)
{
  const TriRec& r = static_cast<Scene*>(p)->world[w];
  const float   v[9] = {r.p0w.x, r.p0w.y, r.p0w.z, r.e1n.x, r.e1n.y, r.e1n.z, r.e2p.x, r.e2p.y, r.e2p.z};
  std::memcpy(out9, v, sizeof(v));
  *flags = __float_as_uint(r.p0w.w) >> 29;
}

// The harness's structures through the read-back interface of the product (pt_accel_dump.h; pt_debug_accel_info / pt_debug_accel_read): two = 0 the flat
// structure, 1 the two-level one.  The harness keeps no binary nodes in node form, no list of active instances, no pad table and no shading lines:
// those arrays hold 0 bytes.
int th_accel_info(void* p, int two, uint32_t* out, int words)
{
  const Scene* s = static_cast<const Scene*>(p);
  if(!out || words < 0)
    return -1;
  uint32_t v[PT_DUMPI_WORDS] = {};
  v[PT_DUMPI_ACCEL_MODE] = two ? 1u : 0u; v[PT_DUMPI_NUM_TRIS] = uint32_t(s->world.size()); v[PT_DUMPI_NUM_INSTANCES] = uint32_t(s->inst.size());
  v[PT_DUMPI_NUM_WIDE_NODES] = uint32_t(two ? s->blasWide.size() : s->flat.wide.size());
  v[PT_DUMPI_HAVE_CNODES] = th_compact_in_use(p, two) ? 1u : 0u;
  v[PT_DUMPI_BUILDER] = 3u;  // the device binned SAH, through its emulation
  if(two)
  {
    v[PT_DUMPI_NODE_CAPACITY] = uint32_t(s->blasWide.size()); v[PT_DUMPI_NUM_TLAS_NODES] = uint32_t(s->tlas.wide.size()); v[PT_DUMPI_NUM_ACTIVE] = s->numActive;
    v[PT_DUMPI_NUM_BLAS] = uint32_t(s->blasRanges.size() / 2) + (s->mergedTris ? 1u : 0u); v[PT_DUMPI_MERGED_TRIS] = s->mergedTris; v[PT_DUMPI_MERGED_WIDE] = s->mergedWide;
    v[PT_DUMPI_MERGED_ONLY] = s->mergedTris && s->numActive == 0 ? 1u : 0u;
    std::memcpy(&v[PT_DUMPI_MERGED_BOX], s->mergedBox, sizeof(s->mergedBox));
  }
  std::copy(v, v + std::min(words, int(PT_DUMPI_WORDS)), out);
  return PT_DUMPI_WORDS;
}
long long th_accel_read(void* p, int two, int which, void* dst, size_t bytes)
{
  const Scene* s    = static_cast<const Scene*>(p);
  const void*  src  = nullptr;
  size_t       have = 0;
  auto take = [&](const auto& vec, size_t count) { src = vec.data(); have = sizeof(vec[0]) * count; };
  const bool cn = th_compact_in_use(p, two) != 0;
  switch(which)
  {
    case PT_DUMP_WIDE: two ? take(s->blasWide, s->blasWide.size()) : take(s->flat.wide, s->flat.wide.size()); break;
    case PT_DUMP_CNODES: if(cn) { two ? take(s->blasCNodes, s->blasCNodes.size()) : take(s->flatCNodes, s->flatCNodes.size()); } break;
    case PT_DUMP_TRIS: two ? take(s->blasTris, s->blasTris.size()) : take(s->flat.tris, s->flat.tris.size()); break;
    case PT_DUMP_ALPHA_RECS: two ? take(s->blasAlpha, s->blasTris.size()) : take(s->flatAlpha, s->flat.tris.size()); break;
    case PT_DUMP_TLAS: if(two) take(s->tlas.wide, s->tlas.wide.size()); break;
    case PT_DUMP_CTLAS: if(two && cn) take(s->tlasCNodes, s->tlasCNodes.size()); break;
    case PT_DUMP_TLAS_LEAVES: if(two) take(s->tlasLeaves, s->tlas.tris.size()); break;
    case PT_DUMP_INST_TRI_BASE: if(two) take(s->instTriBase, s->inst.size()); break;
    case PT_DUMP_INST_BLOCK: if(two) take(s->instBlock, s->instBlock.size()); break;
    case PT_DUMP_INST_NODE_BASE: if(two) take(s->instNodeBase, s->instNodeBase.size()); break;
    case PT_DUMP_BLAS_RANGES: if(two) take(s->blasRanges, s->blasRanges.size()); break;
    case PT_DUMP_MERGED_LIST: if(two) take(s->mergedList, s->mergedList.size()); break;
    default: break;  // BVH2, INST_PAD, ACTIVE, SHADE_TRIS: the harness has none
  }
  if(have == 0)
    return 0;
  if(!dst || bytes < have)
    return -1;
  std::memcpy(dst, src, have);
  return (long long)have;
}

// Every candidate of every ray in key order (t, world index), at most maxCand per ray: mode 0 brute force over all world triangles with the
// product's tri_test, 1 the flat walk, 2 the two-level walk -- traverse<TM_RAW_ALL> restarted behind the previous candidate, exactly what the
// exact fallback kernels (k_closest_x / k_shadow_x) do.  outW / outT: nrays x maxCand (0xffffffff: no further candidate).  Returns the
// number of traversal-stack overflows (must be 0).
uint32_t th_candidates(void* p, int mode, uint32_t nrays, const float* org, const float* dir, float tmax, uint32_t maxCand, uint32_t* outW, float* outT)
{
  Scene* s = static_cast<Scene*>(p);
  return for_each_ray(nrays, 64, nullptr, [&](WalkCtx& ctx, long long r) {
    const f3 o = f3{org[3 * r], org[3 * r + 1], org[3 * r + 2]}, d = f3{dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    float    tPrev = 0.0f;
    uint32_t wPrev = 0xffffffffu;
    for(uint32_t c = 0; c < maxCand; ++c)
    {
      uint32_t bw = 0xffffffffu;
      float    bt = 0.f;
      if(mode == 0)
      {
        bool found = false;
        for(const TriRec& tr : s->world)
        {
          const uint32_t wbits = __float_as_uint(tr.p0w.w), w = wbits & TRI_INDEX_MASK;
          float          t, u, v;
          if(tri_test(tr, wbits >> 29, o, d, t, u, v) && t < tmax && key_less(tPrev, wPrev, t, w) && (!found || key_less(t, w, bt, bw)))
          {
            found = true;
            bt    = t;
            bw    = w;
          }
        }
      }
      else
      {
        RayHit h;
        bool   dummy;
        if(mode == 1)
          traverse<TM_RAW_ALL, false>(s->dsFlat, o, d, tmax, tPrev, wPrev, 0u, ctx.stack.data(), h, dummy, &ctx.cnt);
        else
          traverse<TM_RAW_ALL, true>(s->dsTwo, o, d, tmax, tPrev, wPrev, 0u, ctx.stack.data(), h, dummy, &ctx.cnt);
        if(h.slot != BVH_NONE)
        {
          bt = h.t;
          bw = h.w & TRI_INDEX_MASK;
        }
      }
      outW[size_t(r) * maxCand + c] = bw;
      outT[size_t(r) * maxCand + c] = bt;
      if(bw == 0xffffffffu)
      {
        for(uint32_t k = c + 1; k < maxCand; ++k)
        {
          outW[size_t(r) * maxCand + k] = 0xffffffffu;
          outT[size_t(r) * maxCand + k] = 0.f;
        }
        break;
      }
      tPrev = bt;
      wPrev = bw;
    }
  });
}

}  // extern "C"

// ---- th_settle: three ways to settle a ray, one record, one writer --------------------------------------------------------------------------------
namespace {

// what a ray ended with; closest-hit rays report the world triangle and t, u, v, shadow rays only whether something was found
struct Settled {
  bool     found;
  uint32_t w;
  float    t, u, v;
  uint32_t seed, draws;  // the RNG state afterwards, the alpha draws counted
};

void write_ray(int kind, const Settled& s, size_t r, uint32_t* outW, float* outTUV, uint32_t* outSeed, uint32_t* outDraws)
{
  const bool closest = kind == 0;
  outW[r]            = closest ? (s.found ? s.w : BVH_NONE) : (s.found ? 1u : 0u);
  outTUV[3 * r]      = closest ? (s.found ? s.t : PT_INFINITY) : 0.f;
  outTUV[3 * r + 1]  = closest && s.found ? s.u : 0.f;
  outTUV[3 * r + 2]  = closest && s.found ? s.v : 0.f;
  outSeed[r]         = s.seed;
  outDraws[r]        = s.draws;
}

// exact = 0: tail_closest / tail_shadow (pass A, pass B, consume_rejected_draws, fallback) on path slot r
template <bool TWO>
Settled settle_by_tail(const DeviceScene& S, int kind, int variant, uint32_t r, WalkCtx& c)
{
  Settled s{false, BVH_NONE, 0.f, 0.f, 0.f, 0u, 0u};
  if(kind == 0)
  {
    tail_closest<TWO>(S, c.rb, r, c.stack.data(), s.draws);
    const float4 h = c.rb.ps.hit[r];
    s.w            = __float_as_uint(h.y);  // flat: leaf slot; two-level: world index
    s.found        = s.w != BVH_NONE;
    if(s.found && !TWO)
      s.w = __float_as_uint(S.tris[s.w].p0w.w) & TRI_INDEX_MASK;
    s.t = h.x; s.u = h.z; s.v = h.w;
    s.seed = __float_as_uint(c.rb.ps.rayD[r].w);
  }
  else
    s.found = tail_shadow<TWO>(S, c.rb, r, c.stack.data(), variant, s.seed, s.draws);
  return s;
}

// exact = 1, trace contract T5 / T6 (k_closest_x / k_shadow_x = the definition): candidates strictly in key order, an opaque one commits, a
// non-opaque one draws once
template <bool TWO>
Settled settle_by_exact_loop(const DeviceScene& S, int kind, int variant, f3 o, f3 d, float lim, uint32_t seed0, WalkCtx& c)
{
  Settled  s{false, BVH_NONE, 0.f, 0.f, 0.f, seed0, 0u};
  float    tPrev = 0.0f;
  uint32_t wPrev = 0xffffffffu;
  RayHit   h;
  bool     dummy;
  for(;;)
  {
    traverse<TM_RAW_ALL, TWO>(S, o, d, lim, tPrev, wPrev, 0u, c.stack.data(), h, dummy, &c.cnt);
    if(h.slot == BVH_NONE)
      break;
    if((h.w >> 29) & TRI_OPAQUE)
    {
      s.found = true;
      break;
    }
    ++s.draws;
    if(alpha_test(S, h.slot, h.u, h.v, s.seed))
    {
      s.found = true;
      break;
    }
    tPrev = h.t;
    wPrev = h.w & TRI_INDEX_MASK;
  }
  s.w = h.w & TRI_INDEX_MASK; s.t = h.t; s.u = h.u; s.v = h.v;
  if(kind != 0 && variant == PT_VARIANT_RTX)
    s.seed = seed0;  // RT pipeline: the any-hit shader draws from a copy of the seed
  return s;
}

// exact = 2: the TRACE MACHINE of the persistent kernels (pt_machine.h), one lane fetched like k_closest_p / k_shadow_p fetch it and driven by
// drive_lane; a ray the machine cannot settle goes to the exact loop, as queueX / queueX2 hand it to the exact kernels
template <bool TWO>
Settled settle_by_machine(const DeviceScene& S, int kind, int variant, uint32_t r, f3 o, f3 d, float lim, WalkCtx& c)
{
  TraceLane L;
  uint32_t  seed = 0;
  if(kind == 0)
    lane_fetch_closest(S, c.rb, r, L, seed);
  else
    lane_fetch_shadow(S, c.rb, r, L, seed);
  const LaneVerdict v = drive_lane<TWO>(S, L, seed, c);
  g_spHist[v.maxSp < 64 ? v.maxSp : 64]++;
  if(!v.settled)
    return settle_by_exact_loop<TWO>(S, kind, variant, o, d, lim, seed, c);
  const uint32_t after = kind == 0 ? (v.nDraw ? v.s2 : seed) : (variant == PT_VARIANT_RTX ? seed : v.s2);
  return Settled{L.bslot != BVH_NONE, L.bw & TRI_INDEX_MASK, L.bt, L.bu, L.bv, after, v.nDraw};
}

template <bool TWO>
uint32_t settle_rays(const DeviceScene& S, int kind, int exact, int variant, uint32_t nrays, const float* org, const float* dir, const float* tmax, const uint32_t* seeds, uint32_t* outW,
                     float* outTUV, uint32_t* outSeed, uint32_t* outDraws)
{
  // the rays as path slots: what the tail functions and the machine's fetch read
  std::vector<float4> rayO(nrays), rayD(nrays), absorb(nrays), neeDir(nrays), hit(nrays);
  for(uint32_t r = 0; r < nrays; ++r)
  {
    rayO[r]   = make_float4(org[3 * r], org[3 * r + 1], org[3 * r + 2], 0.f);
    rayD[r]   = make_float4(dir[3 * r], dir[3 * r + 1], dir[3 * r + 2], __uint_as_float(seeds[r]));
    neeDir[r] = make_float4(dir[3 * r], dir[3 * r + 1], dir[3 * r + 2], 1.f);
    absorb[r] = make_float4(0.f, 0.f, 0.f, tmax ? tmax[r] : PT_INFINITY);
  }
  RenderBuffers rb;
  std::memset(&rb, 0, sizeof(rb));
  rb.ps.rayO.p = rayO.data(); rb.ps.rayD.p = rayD.data(); rb.ps.absorb.p = absorb.data(); rb.ps.neeDir.p = neeDir.data(); rb.ps.hit.p = hit.data();
  return for_each_ray(nrays, 64, &rb, [&](WalkCtx& c, long long r) {
    const f3    o = xyz(rayO[r]), d = xyz(rayD[r]);
    const float lim = kind == 0 ? PT_INFINITY : absorb[r].w;
    const Settled s = exact == 2 ? settle_by_machine<TWO>(S, kind, variant, uint32_t(r), o, d, lim, c)
                      : exact    ? settle_by_exact_loop<TWO>(S, kind, variant, o, d, lim, seeds[r], c)
                                 : settle_by_tail<TWO>(S, kind, variant, uint32_t(r), c);
    write_ray(kind, s, size_t(r), outW, outTUV, outSeed, outDraws);
  });
}

}  // namespace

// The product's per-ray settle functions (pt_settle.h: what k_tail runs per lane) and its trace machine against the contract's exact loop, ray by ray.
//   kind 0: closest-hit ray (T5), kind 1: shadow ray (T6, bounded by tmax[r]);  two: 0 flat structure, 1 two-level structure;
//   exact 0 / 1 / 2: settle_by_tail / settle_by_exact_loop / settle_by_machine above.
// out per ray: w (world triangle index of the hit, 0xffffffff none; for shadow rays 1 / 0 = in shadow or not), t, u, v, seed afterwards,
// number of alpha draws counted.  Returns the number of traversal-stack overflows.
extern "C" uint32_t th_settle(void* p, int kind, int two, int exact, int variant, uint32_t nrays, const float* org, const float* dir, const float* tmax, const uint32_t* seeds, uint32_t* outW,
                              float* outTUV, uint32_t* outSeed, uint32_t* outDraws)
{
  Scene* s = static_cast<Scene*>(p);
  return two ? settle_rays<true>(s->dsTwo, kind, exact, variant, nrays, org, dir, tmax, seeds, outW, outTUV, outSeed, outDraws)
             : settle_rays<false>(s->dsFlat, kind, exact, variant, nrays, org, dir, tmax, seeds, outW, outTUV, outSeed, outDraws);
}
