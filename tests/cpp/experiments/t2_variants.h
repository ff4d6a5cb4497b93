// EXPERIMENTS (tools/t2_robust_experiment.py; not the contract): two candidate replacements of the triangle test T2, compiled only into the harness
// flavours "robust" (-DTH_ROBUST_T2) and "certified" (-DTH_CERTIFIED_T2).  Included by th_shims.h before the product's headers, so that pt_trace.h
// sees PT_TRI_TEST_OVERRIDE in every unit.  The counters are read through th_t2_stats / th_t2_accepts (t2_experiment.cpp).
#pragma once
#include "pt_device.h"
// [tests, tests re-evaluated in double (robust) / fp32 accepts that certification turned into misses (certified)], fp32 accepts (certified);
// counted per thread and folded after every parallel loop over rays (th_walk.h for_each_ray)
inline std::atomic<unsigned long long> g_t2Calls{0}, g_t2Double{0}, g_t2Accepts{0};
inline thread_local unsigned long long tl_t2Calls = 0, tl_t2Double = 0, tl_t2Accepts = 0;
inline void th_t2_fold()
{
  g_t2Calls += tl_t2Calls; g_t2Double += tl_t2Double; g_t2Accepts += tl_t2Accepts;
  tl_t2Calls = tl_t2Double = tl_t2Accepts = 0;
}
// forward error bounds of det and of the three numerators, componentwise: a cross product's component a_i b_j - a_j b_i is off by at most
// 2 ulp of |a_i b_j| + |a_j b_i|, a 3-term dot by 3 ulp of sum |x_i y_i| plus |x| . (error of y); 8 ulp covers every chain of the tests below
struct T2Bounds {
  float edet, eu, ev, et;
};
static inline T2Bounds t2_bounds(f3 e1, f3 e2, f3 d, f3 tv)
{
  const f3    apv = f3{fabsf(d.y) * fabsf(e2.z) + fabsf(d.z) * fabsf(e2.y), fabsf(d.z) * fabsf(e2.x) + fabsf(d.x) * fabsf(e2.z), fabsf(d.x) * fabsf(e2.y) + fabsf(d.y) * fabsf(e2.x)};
  const f3    atv = f3{fabsf(tv.x), fabsf(tv.y), fabsf(tv.z)};
  const f3    aqv = f3{atv.y * fabsf(e1.z) + atv.z * fabsf(e1.y), atv.z * fabsf(e1.x) + atv.x * fabsf(e1.z), atv.x * fabsf(e1.y) + atv.y * fabsf(e1.x)};
  const float k   = 8.0f * 5.9604645e-8f;
  return T2Bounds{k * (fabsf(e1.x) * apv.x + fabsf(e1.y) * apv.y + fabsf(e1.z) * apv.z), k * (atv.x * apv.x + atv.y * apv.y + atv.z * apv.z),
                  k * (fabsf(d.x) * aqv.x + fabsf(d.y) * aqv.y + fabsf(d.z) * aqv.z), k * (fabsf(e2.x) * aqv.x + fabsf(e2.y) * aqv.y + fabsf(e2.z) * aqv.z)};
}
#ifdef TH_ROBUST_T2
// EXPERIMENT (tools/t2_robust_experiment.py; not the contract): T2 with a forward error bound.  The fp32 evaluation is kept whenever its verdict
// cannot be an artefact of rounding: |det|, u, v, 1 - u - v and t are further from their decision boundaries than the rounding error of their
// numerators allows.  Otherwise the same formulas are evaluated in double precision (IEEE, so identical on every side) and rounded once.
static inline bool th_tri_test_robust(const TriRec& tr, uint32_t flags, f3 o, f3 d, float& t, float& u, float& v)
{
  const f3    e1 = xyz(tr.e1n), e2 = xyz(tr.e2p), p0 = xyz(tr.p0w);
  const f3    pv = cross3(d, e2);
  const float det = dot3(e1, pv);
  const f3    tv = o - p0;
  const f3    qv = cross3(tv, e1);
  const float nu = dot3(tv, pv), nv = dot3(d, qv), nt = dot3(e2, qv);
  const T2Bounds b    = t2_bounds(e1, e2, d, tv);
  const float    edet = b.edet, eu = b.eu, ev = b.ev, et = b.et, adet = fabsf(det);
  ++tl_t2Calls;
  bool        sure = adet > 4.0f * edet;
  if(sure)
  {
    const float s  = det < 0.0f ? -1.0f : 1.0f;
    const float su = nu * s, sv = nv * s;  // compare numerators against 0 and |det| (no division needed for the verdict)
    const bool  inside  = su > eu && sv > ev && (adet - su - sv) > (eu + ev + edet);
    const bool  outside = su < -eu || sv < -ev || (su + sv - adet) > (eu + ev + edet);
    const bool  tOk     = et <= 4.0e-6f * fabsf(nt);  // relative error of t below the slack of the box tests (leaf padding 4e-6 |coordinate|)
    sure = outside || (inside && tOk);
  }
  if(sure)
  {
    if(det == 0.0f)
      return false;
    if(!(flags & TRI_NOCULL))
    {
      const bool front = (flags & TRI_FLIP) ? (det < 0.0f) : (det > 0.0f);
      if(!front)
        return false;
    }
    const float inv = 1.0f / det;
    u = nu * inv;
    if(u < 0.0f || u > 1.0f)
      return false;
    v = nv * inv;
    if(v < 0.0f || u + v > 1.0f)
      return false;
    t = nt * inv;
    return true;
  }
  // ambiguous in fp32: the same test in double
  ++tl_t2Double;
  const double E1[3] = {e1.x, e1.y, e1.z}, E2[3] = {e2.x, e2.y, e2.z}, D[3] = {d.x, d.y, d.z}, TV[3] = {double(o.x) - p0.x, double(o.y) - p0.y, double(o.z) - p0.z};
  const double PV[3] = {D[1] * E2[2] - D[2] * E2[1], D[2] * E2[0] - D[0] * E2[2], D[0] * E2[1] - D[1] * E2[0]};
  const double DET   = E1[0] * PV[0] + E1[1] * PV[1] + E1[2] * PV[2];
  if(DET == 0.0)
    return false;
  if(!(flags & TRI_NOCULL))
  {
    const bool front = (flags & TRI_FLIP) ? (DET < 0.0) : (DET > 0.0);
    if(!front)
      return false;
  }
  const double U = (TV[0] * PV[0] + TV[1] * PV[1] + TV[2] * PV[2]) / DET;
  if(U < 0.0 || U > 1.0)
    return false;
  const double QV[3] = {TV[1] * E1[2] - TV[2] * E1[1], TV[2] * E1[0] - TV[0] * E1[2], TV[0] * E1[1] - TV[1] * E1[0]};
  const double V     = (D[0] * QV[0] + D[1] * QV[1] + D[2] * QV[2]) / DET;
  if(V < 0.0 || U + V > 1.0)
    return false;
  u = float(U);
  v = float(V);
  t = float((E2[0] * QV[0] + E2[1] * QV[1] + E2[2] * QV[2]) / DET);
  return true;
}
#define PT_TRI_TEST_OVERRIDE th_tri_test_robust
#endif
#ifdef TH_CERTIFIED_T2
// EXPERIMENT (tools/t2_robust_experiment.py; not the contract): "certified" T2 -- the contract's fp32 Moeller-Trumbore, whose ACCEPTED candidates are kept
// only when the forward error bound of round 2's experiment certifies their barycentrics to TH_TAU (and their distance to TH_TAU relative): no fp64, no
// second code path for a wavefront to diverge into, ~35 more fp32 operations per test.  A candidate that fp32 cannot certify counts as a miss ON EVERY SIDE
// (brute force, every walk), so what is left of "BVH-dependent" is a hit that lies up to TH_TAU of its triangle's extent outside the triangle's box.
#ifndef TH_TAU
#define TH_TAU 0.0078125f  // 2^-7
#endif
static inline bool th_tri_test_certified(const TriRec& tr, uint32_t flags, f3 o, f3 d, float& t, float& u, float& v)
{
  const f3    e1 = xyz(tr.e1n), e2 = xyz(tr.e2p), p0 = xyz(tr.p0w);
  const f3    pv = cross3(d, e2);
  const float det = dot3(e1, pv);
  ++tl_t2Calls;
  if(det == 0.0f)
    return false;
  if(!(flags & TRI_NOCULL))
  {
    const bool front = (flags & TRI_FLIP) ? (det < 0.0f) : (det > 0.0f);
    if(!front)
      return false;
  }
  const float inv = 1.0f / det;
  const f3    tv  = o - p0;
  const float nu  = dot3(tv, pv);
  u               = nu * inv;
  if(u < 0.0f || u > 1.0f)
    return false;
  const f3    qv = cross3(tv, e1);
  const float nv = dot3(d, qv);
  v              = nv * inv;
  if(v < 0.0f || u + v > 1.0f)
    return false;
  const float nt = dot3(e2, qv);
  t              = nt * inv;
  // certification of the accepted candidate
  const T2Bounds b    = t2_bounds(e1, e2, d, tv);
  const float    edet = b.edet, eu = b.eu, ev = b.ev, et = b.et, adet = fabsf(det);
  ++tl_t2Accepts;
  const bool ok = (eu + ev + 2.0f * edet) <= TH_TAU * adet && (et * adet + fabsf(nt) * edet) <= TH_TAU * fabsf(nt) * adet;
  if(!ok)
    ++tl_t2Double;
  return ok;
}
#define PT_TRI_TEST_OVERRIDE th_tri_test_certified
#endif
