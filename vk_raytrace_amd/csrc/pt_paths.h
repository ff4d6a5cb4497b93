// One caller ray through the path loop ("Path queries"): what pt_trace_paths runs per lane (pt_paths.hip k_paths).
// Plain inline functions of plain values -- scene, frame parameters, variant, one pt_Ray, the lane's traversal stack, the counters, where the
// result goes -- so that tests/cpp/paths_host.cpp compiles them for the host, like pt_query.h, and holds them ray by ray to the oracle's frames.
//
// Nothing of the path loop is stated here a second time.  The per-bounce body is the sequence k_tail (pt_render.hip) and trace_path
// (tests/cpp/render_host.cpp) run -- tail_closest -> shade_path<-1> -> tail_shadow -> finish_bounce_core -- on a path state of ONE slot: the eight
// float4 rows of PathStateT without `sum`, which live in the lane (a RenderBuffers is pointed at them, as query_ray does with its five).
// What this header adds is section 3.2's frame around that body: the sample loop on one chained seed, the firefly clamp and the mean of
// accumulate_pixel, and the record.
//
// The loop is cut at the bounce: path_begin, then path_step until it says the ray is finished, then path_end.  path_query is exactly that and is
// what the host build runs; the kernel runs the same three functions with its ray supply between the steps, so that a lane whose ray is finished
// takes the next one while its neighbours are still on theirs.
#pragma once
#include "pt_shade.h"
#include "pt_query.h"  // query_finite: one rule for what makes a caller's ray invalid

// what path_step reports to a caller who wants to see the rays of a path (tests/cpp/paths_host.cpp ph_path_segments); the kernel passes the default,
// which compiles to nothing
struct PathNoSegments {
  PT_DEV void operator()(int /*kind: PT_RAYS_CLOSEST / PT_RAYS_OCCLUDED*/, f3 /*origin*/, f3 /*direction*/, float /*bound*/) const {}
};

// a ray on its way: the one-slot path state and what section 3.2 carries from sample to sample
struct PathLane {
  float4   rayO, rayD, thr, rad, absorb, neeDir, neeRad, hit;  // pt_device.h PathStateT (no `sum`: the sample sum is below)
  f3       o, d;                                               // the caller's ray: every sample starts on it
  f3       sum;
  float    firstT;
  uint32_t status, closestRays;
  int      sample, depth;
};

PT_DEV pt_PathResult path_result(f3 radiance, float firstT, uint32_t seed, uint32_t status, uint32_t closestRays)
{
  pt_PathResult r;
  r.radiance[0] = radiance.x; r.radiance[1] = radiance.y; r.radiance[2] = radiance.z;
  r.firstT      = firstT;
  r.seed        = seed;
  r.status      = status;
  r.closestRays = closestRays;
  r._pad        = 0u;
  return r;
}

// the path state as generate_ray leaves it: the same ray for every sample, the stream continues from `seed`
PT_DEV void path_start_sample(const FrameParams& fp, PathLane& L, uint32_t seed)
{
  L.rayO = make_float4(L.o.x, L.o.y, L.o.z, 0.0f);
  L.rayD = make_float4(L.d.x, L.d.y, L.d.z, __uint_as_float(seed));
  if(fp.st.maxDepth == 0)
    L.rad = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  L.depth = 0;
}

// false: the ray is invalid -- decided before any walk, by pt_trace_rays' rule (tmax is ignored: the first ray is unbounded, like
// PT_RAYS_CLOSEST) -- and `out` is its record; true: L is at the start of its first sample
PT_DEV bool path_begin(const FrameParams& fp, const pt_Ray& ray, PathLane& L, pt_PathResult& out)
{
  const f3   o = f3{ray.origin[0], ray.origin[1], ray.origin[2]}, d = f3{ray.direction[0], ray.direction[1], ray.direction[2]};
  const bool valid = query_finite(o.x) && query_finite(o.y) && query_finite(o.z) && query_finite(d.x) && query_finite(d.y) && query_finite(d.z) &&
                     !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
  if(!valid)
  {
    out = path_result(splat3(0.0f), 0.0f, ray.seed, PT_RAY_INVALID, 0u);
    return false;
  }
  L.o = o;
  L.d = d;
  L.thr = L.rad = L.absorb = L.neeDir = L.neeRad = L.hit = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (each is written before it is read: shade_path knows the depth-0 values)
  L.sum         = splat3(0.0f);
  L.firstT      = 0.0f;
  L.status      = 0u;
  L.closestRays = 0u;
  L.sample      = 0;
  path_start_sample(fp, L, ray.seed);
  return true;
}

// One bounce of the current sample (none when maxDepth == 0) and, where the path ends with it, the end of the sample: seed, clamp, sum, and the
// start of the next sample.  Returns true when the last sample has ended.  fp: st (maxDepth, maxSamples, fireflyClampThreshold, hdrMultiplier,
// pbrMode, debugging_mode are read) -- the entry point has validated it.  stack: the lane's [level][lane] traversal stack (pt_trace.h).
template <bool TWO, class SEG = PathNoSegments>
PT_DEV bool path_step(const DeviceScene& S, const FrameParams& fp, int variant, PathLane& L, uint32_t* stack, Counters* counters, SEG seg = SEG())
{
  RenderBuffers rb{};
  rb.ps.rayO.p   = &L.rayO;
  rb.ps.rayD.p   = &L.rayD;
  rb.ps.thr.p    = &L.thr;
  rb.ps.rad.p    = &L.rad;
  rb.ps.absorb.p = &L.absorb;
  rb.ps.neeDir.p = &L.neeDir;
  rb.ps.neeRad.p = &L.neeRad;
  rb.ps.hit.p    = &L.hit;
  rb.counters    = counters;
  const int maxDepth = fp.st.maxDepth;
  if(maxDepth != 0)  // (a step is a bounce; which bounce is the last is `survive`'s to say, as in k_tail)
  {
    uint32_t nAlpha = 0;  // (the draws a frame would count into pt_Stats::alphaTests: a query touches no statistic)
    seg(PT_RAYS_CLOSEST, xyz(float4(rb.ps.rayO[0])), xyz(float4(rb.ps.rayD[0])), PT_INFINITY);
    tail_closest<TWO>(S, rb, 0u, stack, nAlpha);
    ++L.closestRays;
    if(L.sample == 0 && L.depth == 0)
    {
      const float4 hr = rb.ps.hit[0];
      if(__float_as_uint(hr.y) != BVH_NONE)
      {
        L.status = PT_RAY_HIT;
        L.firstT = hr.x;
      }
    }
    uint32_t  events  = 0;
    const int to      = shade_path<-1>(S, rb, fp, 0u, L.depth, events);
    bool      survive = to == SHADE_TO_NEXT;
    if(to == SHADE_TO_SHADOW)
    {
      seg(PT_RAYS_OCCLUDED, xyz(float4(rb.ps.rayO[0])), xyz(float4(rb.ps.neeDir[0])), float4(rb.ps.absorb[0]).w);
      uint32_t   sd;
      const bool inShadow = tail_shadow<TWO>(S, rb, 0u, stack, variant, sd, nAlpha);
      survive             = finish_bounce_core(rb, 0u, inShadow, sd) && L.depth != maxDepth - 1;
    }
    ++L.depth;
    if(survive)  // (never at the last bounce: shade_path ends a SHADE_TO_NEXT path there itself, as in k_tail)
      return false;
  }
  // the path has ended: accumulate_pixel's clamp and sum, in sample order
  const uint32_t seed = __float_as_uint(float4(rb.ps.rayD[0]).w);
  f3             r    = xyz(float4(rb.ps.rad[0]));
  const float    lum  = dot3(r, f3{0.212671f, 0.715160f, 0.072169f});
  if(lum > fp.st.fireflyClampThreshold)
    r *= fp.st.fireflyClampThreshold / lum;
  L.sum += r;
  if(++L.sample == fp.st.maxSamples)
    return true;
  path_start_sample(fp, L, seed);
  return false;
}

// after the last sample: the mean (the division happens for one sample too, as in accumulate_pixel) and the stream's state
PT_DEV pt_PathResult path_end(const FrameParams& fp, const PathLane& L)
{
  return path_result(L.sum / float(fp.st.maxSamples), L.firstT, __float_as_uint(L.rayD.w), L.status, L.closestRays);
}

template <bool TWO, class SEG = PathNoSegments>
PT_DEV void path_query(const DeviceScene& S, const FrameParams& fp, int variant, const pt_Ray& ray, uint32_t* stack, Counters* counters, pt_PathResult& out, SEG seg = SEG())
{
  PathLane L;
  if(!path_begin(fp, ray, L, out))
    return;
  while(!path_step<TWO>(S, fp, variant, L, stack, counters, seg))
  {
  }
  out = path_end(fp, L);
}
