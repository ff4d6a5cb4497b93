// One caller ray through the trace contract ("Ray queries"): what pt_trace_rays runs per lane (pt_query.hip k_query).
// A plain inline function of plain values -- scene, kind, variant, one pt_Ray, the lane's traversal stack, the counters, where the ray's results
// go -- so that tests/cpp/query_host.cpp compiles it for the host, like pt_settle.h, and holds it ray by ray to brute force and to the exact loop.
//
// Nothing of the contract is stated here a second time.  PT_RAYS_CLOSEST and PT_RAYS_OCCLUDED run tail_closest / tail_shadow, the bodies k_tail
// runs per lane, on a path state of ONE slot: five float4 rows that live in the lane's registers (query_ray fills them from the ray and points a
// RenderBuffers at them; every function involved is inline, so the rows never reach memory).  PT_RAYS_NEAREST is k_pick's traverse<TM_PICK>,
// PT_RAYS_CANDIDATES the traverse<TM_RAW_ALL> restarted behind the previous key that the exact loops are made of.  The hit is decoded to
// (instance, primitive, prim-mesh) as k_pick decodes it for each structure.
#pragma once
#include "pt_settle.h"
#include "../../include/pt_types.h"

PT_DEV bool query_finite(float x) { return fabsf(x) <= 3.402823466e38f; }  // false for NaN and +-Inf

PT_DEV pt_RayHit query_miss(uint32_t seed, uint32_t status)
{
  pt_RayHit r;
  r.t = r.u = r.v = 0.0f;
  r.instanceID          = 0xffffffffu;
  r.primitiveID         = -1;
  r.instanceCustomIndex = -1;
  r.seed                = seed;
  r.status              = status;
  return r;
}

// `ref` names the triangle the way the hit record of the structure does (pt_settle.h store_hit): its leaf slot in the flat structure, its world
// triangle index in the two-level one.  The decode is k_pick's.
template <bool TWO>
PT_DEV pt_RayHit query_hit(const DeviceScene& S, uint32_t ref, float t, float u, float v, uint32_t seed)
{
  pt_RayHit r;
  r.t = t; r.u = u; r.v = v;
  if(TWO)
  {
    r.instanceID  = instance_of_world_tri(S, ref);
    r.primitiveID = int32_t(ref - S.instTriBase[r.instanceID]);
  }
  else
  {
    const TriRec tr = S.tris[ref];
    r.instanceID    = __float_as_uint(tr.e1n.w);
    r.primitiveID   = int32_t(__float_as_uint(tr.e2p.w));
  }
  r.instanceCustomIndex = S.instances[r.instanceID].primMesh;
  r.seed                = seed;
  r.status              = PT_RAY_HIT;
  return r;
}

// out: hitsPerRay records (1 unless kind == PT_RAYS_CANDIDATES).  stack: the lane's [level][lane] traversal stack (pt_trace.h).
template <bool TWO>
PT_DEV void query_ray(const DeviceScene& S, int kind, int variant, const pt_Ray& ray, uint32_t hitsPerRay, uint32_t* stack, Counters* counters, pt_RayHit* out)
{
  const f3   o       = f3{ray.origin[0], ray.origin[1], ray.origin[2]}, d = f3{ray.direction[0], ray.direction[1], ray.direction[2]};
  const bool bounded = kind != PT_RAYS_CLOSEST;
  // decided before any walk: a ray that cannot be walked (the box tests and T2 have no meaning on it) is reported, not traced
  const bool valid = query_finite(o.x) && query_finite(o.y) && query_finite(o.z) && query_finite(d.x) && query_finite(d.y) && query_finite(d.z) &&
                     !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) && !(bounded && ray.tmax != ray.tmax);
  if(!valid || (bounded && !(ray.tmax > 0.0f)))  // (tmax <= 0: the range (0, tmax) is empty)
  {
    for(uint32_t k = 0; k < hitsPerRay; ++k)
      out[k] = query_miss(ray.seed, valid ? 0u : PT_RAY_INVALID);
    return;
  }
  RayHit h;
  bool   dummy;
  if(kind == PT_RAYS_NEAREST)
  {
    traverse<TM_PICK, TWO>(S, o, d, ray.tmax, 0.0f, 0xffffffffu, 0u, stack, h, dummy, counters);
    out[0] = h.slot == BVH_NONE ? query_miss(ray.seed, 0u) : query_hit<TWO>(S, TWO ? (h.w & TRI_INDEX_MASK) : h.slot, h.t, h.u, h.v, ray.seed);
    return;
  }
  if(kind == PT_RAYS_CANDIDATES)
  {
    float    tPrev = 0.0f;
    uint32_t wPrev = 0xffffffffu, k = 0;
    for(; k < hitsPerRay; ++k)
    {
      traverse<TM_RAW_ALL, TWO>(S, o, d, ray.tmax, tPrev, wPrev, 0u, stack, h, dummy, counters);
      if(h.slot == BVH_NONE)
        break;
      out[k] = query_hit<TWO>(S, TWO ? (h.w & TRI_INDEX_MASK) : h.slot, h.t, h.u, h.v, ray.seed);
      tPrev  = h.t;
      wPrev  = h.w & TRI_INDEX_MASK;
    }
    for(; k < hitsPerRay; ++k)
      out[k] = query_miss(ray.seed, 0u);
    return;
  }
  // T5 / T6: a path state of one slot, filled the way k_shade leaves it for the trace stages (pt_device.h PathStateT)
  float4        rayO = make_float4(o.x, o.y, o.z, 0.0f), rayD = make_float4(d.x, d.y, d.z, __uint_as_float(ray.seed));
  float4        absorb = make_float4(0.0f, 0.0f, 0.0f, ray.tmax), neeDir = make_float4(d.x, d.y, d.z, 1.0f), hit = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  RenderBuffers rb{};
  rb.ps.rayO.p   = &rayO;
  rb.ps.rayD.p   = &rayD;
  rb.ps.absorb.p = &absorb;
  rb.ps.neeDir.p = &neeDir;
  rb.ps.hit.p    = &hit;
  rb.counters    = counters;
  uint32_t nAlpha = 0;  // (the draws a frame would count into pt_Stats::alphaTests: a query touches no statistic)
  if(kind == PT_RAYS_CLOSEST)
  {
    tail_closest<TWO>(S, rb, 0u, stack, nAlpha);
    const float4   hr   = rb.ps.hit[0];
    const uint32_t seed = __float_as_uint(float4(rb.ps.rayD[0]).w);
    const uint32_t ref  = __float_as_uint(hr.y);
    out[0]              = ref == BVH_NONE ? query_miss(seed, 0u) : query_hit<TWO>(S, ref, hr.x, hr.z, hr.w, seed);
  }
  else
  {
    uint32_t   seed;
    const bool inShadow = tail_shadow<TWO>(S, rb, 0u, stack, variant, seed, nAlpha);
    out[0]              = query_miss(seed, inShadow ? PT_RAY_HIT : 0u);
  }
}
