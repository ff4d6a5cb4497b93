// One caller point through the path loop ("Gather queries"): what pt_gather runs per lane (pt_gather.hip k_gather).
// Plain inline functions of plain values, like pt_paths.h, so that tests/cpp/gather_host.cpp compiles them for the host and holds them point by
// point to the host build of section 3.2.
//
// Nothing of the path loop is stated here, not even the sequence of its four functions: a sample's path IS pt_paths.h's path_step, unchanged, run
// as a one-sample query (FrameParams with maxSamples = 1) on the PathLane the GatherLane holds, with its sum and sample counter cleared where the
// sample starts -- so path_step's "last sample has ended" is the end of THIS sample, the lane's `sum` is the sample's clamped radiance (0 + r) and
// its `status` says whether the sample's first ray hit.  (Cutting path_step into bounce and end of sample was tried first: k_paths' device code
// moved, so pt_paths.h stays as it is.)  What this header adds is section 3.3's frame around it: the direction each sample draws before its path,
// the seed chained through draws and paths, and the reduction -- the sum of PT_GATHER_HEMISPHERE in the lane, the 27 spherical-harmonic sums of
// PT_GATHER_SPHERE in the point's own record (which only this lane touches: plain vector loads and stores, fp32, in sample order), so that the
// probe kind carries no more registers through shade_path than the other.
//
// The loop is cut at the bounce like path_query's: gather_begin, gather_step until it says the point is finished, gather_end; gather_point is
// exactly that and is what the host build runs.  `rec` is the point's record as float4 rows: 2 (pt_GatherResult) or 8 (pt_ProbeResult).
#pragma once
#include "pt_paths.h"

// what gather_step reports to a caller who wants to see the sample rays (tests/cpp/gather_host.cpp gh_gather_rays); the kernel passes the default
struct GatherNoRays {
  PT_DEV void operator()(f3 /*origin*/, f3 /*direction*/, uint32_t /*seed at the start of the path*/) const {}
};

// a point on its way: the one-slot path state, and what section 3.3 carries from sample to sample
struct GatherLane {
  PathLane P;        // P.o: the origin of every sample; P.d: the current sample's direction; P.closestRays counts over all samples.
                     // P.sum, P.sample, P.status are one sample's: cleared where it starts, read where it ends
  f3       N, T, B;  // HEMISPHERE: the frame about the unit normal (SPHERE: unused)
  f3       sum;      // HEMISPHERE: the clamped radiances, in sample order
  uint32_t hits;     // samples whose first ray hit geometry
  int      sample;
};

// the parameters of a sample's path: the call's, as a one-sample query
PT_DEV FrameParams gather_one_sample(const FrameParams& fp)
{
  FrameParams one    = fp;
  one.st.maxSamples = 1;
  return one;
}

// the nine real spherical-harmonic basis functions of bands 0 .. 2 at direction d (section 3.3: fp32 constants, one product order each)
PT_DEV void gather_sh_basis(f3 d, float Y[9])
{
  Y[0] = 0.282095f;
  Y[1] = 0.488603f * d.y;
  Y[2] = 0.488603f * d.z;
  Y[3] = 0.488603f * d.x;
  Y[4] = 1.092548f * (d.x * d.y);
  Y[5] = 1.092548f * (d.y * d.z);
  Y[6] = 0.315392f * (3.0f * (d.z * d.z) - 1.0f);
  Y[7] = 1.092548f * (d.x * d.z);
  Y[8] = 0.546274f * (d.x * d.x - d.y * d.y);
}

// the last row of a record: seed, status, closestRays, _pad (hitFraction is the .w of the row before it)
PT_DEV float4 gather_tail(uint32_t seed, uint32_t status, uint32_t closestRays)
{
  return make_float4(__uint_as_float(seed), __uint_as_float(status), __uint_as_float(closestRays), __uint_as_float(0u));
}

// where a sample starts: two draws, the direction, and the path state as path_start_sample leaves it for (o, d) and the seed after the draws
template <uint32_t KIND, class RAYS>
PT_DEV void gather_start_sample(const FrameParams& fp, GatherLane& G, uint32_t seed, RAYS rays)
{
  const float r1 = rng_next(seed), r2 = rng_next(seed);
  if(KIND == PT_GATHER_HEMISPHERE)
  {
    const f3 l = sample_cosine_hemisphere(r1, r2);
    G.P.d      = (G.T * l.x + G.B * l.y) + G.N * l.z;  // (not re-normalised)
  }
  else
  {
    const float z = 1.0f - 2.0f * r1, q = sqrtf(fmax2(0.0f, 1.0f - z * z)), phi = PT_TWO_PI * r2;
    G.P.d         = f3{q * pt_cos(phi), q * pt_sin(phi), z};
  }
  G.P.status = 0u;
  G.P.firstT = 0.0f;
  G.P.sum    = splat3(0.0f);
  G.P.sample = 0;
  path_start_sample(fp, G.P, seed);
  rays(G.P.o, G.P.d, seed);
}

// false: the point is invalid -- decided before any walk -- and its record is written; true: G is at the start of its first sample
template <uint32_t KIND, class RAYS = GatherNoRays>
PT_DEV bool gather_begin(const FrameParams& fp, const pt_GatherPoint& pt, GatherLane& G, float4* rec, RAYS rays = RAYS())
{
  const f3 p     = f3{pt.position[0], pt.position[1], pt.position[2]};
  bool     valid = query_finite(p.x) && query_finite(p.y) && query_finite(p.z);
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if(KIND == PT_GATHER_HEMISPHERE)
  {
    const f3 n = f3{pt.normal[0], pt.normal[1], pt.normal[2]};
    valid      = valid && query_finite(n.x) && query_finite(n.y) && query_finite(n.z) && !(n.x == 0.0f && n.y == 0.0f && n.z == 0.0f);
    // ... and a normal unit() cannot normalise is no normal either: unit squares the components, so a squared length that underflows makes N
    // Inf / NaN and one that overflows makes it zero (lengths outside about 1e-19 .. 1.8e19) -- the directions path_begin refuses for a path query
    G.N   = unit(n);
    valid = valid && query_finite(G.N.x) && query_finite(G.N.y) && query_finite(G.N.z) && !(G.N.x == 0.0f && G.N.y == 0.0f && G.N.z == 0.0f);
    if(valid)
    {
      make_frame(G.N, G.T, G.B);
      G.P.o = offset_ray(p, G.N);
    }
  }
  else
  {
    G.P.o = p;  // a probe floats: not offset
#pragma unroll
    for(int j = 0; j < 7; ++j)  // the sums start at zero, in the record
      rec[j] = zero;
  }
  if(!valid)
  {
    rec[KIND == PT_GATHER_HEMISPHERE ? 0 : 6] = zero;
    rec[KIND == PT_GATHER_HEMISPHERE ? 1 : 7] = gather_tail(pt.seed, PT_RAY_INVALID, 0u);
    return false;
  }
  G.P.thr = G.P.rad = G.P.absorb = G.P.neeDir = G.P.neeRad = G.P.hit = zero;  // (each is written before it is read, as in path_begin)
  G.P.closestRays = 0u;
  G.sum           = splat3(0.0f);
  G.hits          = 0u;
  G.sample        = 0;
  gather_start_sample<KIND>(fp, G, pt.seed, rays);
  return true;
}

// One bounce of the current sample (none when maxDepth == 0) and, where the path ends with it, the end of the sample: seed, clamp, reduction, and
// the next sample's draws.  Returns true when the last sample has ended.
template <bool TWO, uint32_t KIND, class RAYS = GatherNoRays>
PT_DEV bool gather_step(const DeviceScene& S, const FrameParams& fp, int variant, GatherLane& G, float4* rec, uint32_t* stack, Counters* counters, RAYS rays = RAYS())
{
  if(!path_step<TWO>(S, gather_one_sample(fp), variant, G.P, stack, counters))
    return false;
  // the sample's path has ended: path_step has clamped its radiance into P.sum (0 + r) and left the stream's state in rayD.w
  const uint32_t seed = __float_as_uint(G.P.rayD.w);
  const f3       r    = G.P.sum;
  G.hits += G.P.status & PT_RAY_HIT;
  if(KIND == PT_GATHER_HEMISPHERE)
    G.sum += r;
  else
  {
    float Y[9], c[28];
    gather_sh_basis(G.P.d, Y);
#pragma unroll
    for(int k = 0; k < 9; ++k)
    {
      c[3 * k]     = r.x * Y[k];
      c[3 * k + 1] = r.y * Y[k];
      c[3 * k + 2] = r.z * Y[k];
    }
    c[27] = 0.0f;
#pragma unroll
    for(int j = 0; j < 7; ++j)
    {
      const float4 a = rec[j];
      rec[j]         = make_float4(a.x + c[4 * j], a.y + c[4 * j + 1], a.z + c[4 * j + 2], j == 6 ? a.w : a.w + c[4 * j + 3]);
    }
  }
  if(++G.sample == fp.st.maxSamples)
    return true;
  gather_start_sample<KIND>(fp, G, seed, rays);
  return false;
}

// after the last sample: the estimator's factor and the record
template <uint32_t KIND>
PT_DEV void gather_end(const FrameParams& fp, const GatherLane& G, float4* rec)
{
  const float  S    = float(fp.st.maxSamples), hitFraction = float(G.hits) / S;
  const float4 tail = gather_tail(__float_as_uint(G.P.rayD.w), 0u, G.P.closestRays);
  if(KIND == PT_GATHER_HEMISPHERE)
  {
    const f3 e = (G.sum / S) * PT_PI;  // the pdf is cos / pi: the cosine cancels
    rec[0]     = make_float4(e.x, e.y, e.z, hitFraction);
    rec[1]     = tail;
  }
  else
  {
    const float fourPi = 4.0f * PT_PI;  // 1 / pdf of the uniform sphere
#pragma unroll
    for(int j = 0; j < 7; ++j)
    {
      const float4 a = rec[j];
      rec[j]         = make_float4((a.x / S) * fourPi, (a.y / S) * fourPi, (a.z / S) * fourPi, j == 6 ? hitFraction : (a.w / S) * fourPi);
    }
    rec[7] = tail;
  }
}

template <bool TWO, uint32_t KIND, class RAYS = GatherNoRays>
PT_DEV void gather_point(const DeviceScene& S, const FrameParams& fp, int variant, const pt_GatherPoint& pt, float4* rec, uint32_t* stack, Counters* counters, RAYS rays = RAYS())
{
  GatherLane G;
  if(!gather_begin<KIND>(fp, pt, G, rec, rays))
    return;
  while(!gather_step<TWO, KIND>(S, fp, variant, G, rec, stack, counters, rays))
  {
  }
  gather_end<KIND>(fp, G, rec);
}
