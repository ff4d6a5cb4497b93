// Motion of moving instances for the temporal stage (DESIGN.md section 5.5 is the definition): the per-instance motion table the host makes from the
// instance transforms the history was made with and the current ones, and ONE output pixel of pt_temporal_accumulate_moving -- pt_temporal.h's step 1,
// the table applied to the point and the normal, then pt_temporal.h's steps 2 to 4.  Plain inline functions of plain values, compiled by hipcc for the
// device (pt_motion.hip) and by g++ for the host (tests/cpp/motion_host.cpp), like pt_temporal.h: -ffp-contract=off, no fast math, IEEE / and sqrtf only.
// No reference counterpart.
#pragma once
#include <string.h>
#include "pt_temporal.h"

// An instance as the table function reads it: the 12 words of InstanceRec::objectToWorld, then the 12 of worldToObject (pt_device.h; three rows of four,
// row r = (m[0][r], m[1][r], m[2][r], m[3][r]) of the column-major matrix)
#define PT_MOTION_INSTANCE_WORDS 24

// toPrev takes a current world point of the instance to where that point of the object was when the history was made; normalToPrev (rows of three words
// and a zero) does the same for a normal.  Both in the row layout of Affine (pt_math.h).  moved = 0: the record is not read.
struct alignas(16) MotionRec {
  float    toPrev[12];
  float    normalToPrev[12];
  uint32_t moved;
  uint32_t pad[3];
};

// entry (r, c) of the product A B of two affine transforms given as rows, composed in double from the fp32 words: ((a0 b0c + a1 b1c) + a2 b2c) + a3 [c = 3]
static inline double motion_compose(const float* A, const float* B, int r, int c)
{
  const double s = (double(A[4 * r]) * double(B[c]) + double(A[4 * r + 1]) * double(B[4 + c])) + double(A[4 * r + 2]) * double(B[8 + c]);
  return c == 3 ? s + double(A[4 * r + 3]) : s;
}

// The record of one instance: hist / cur are its PT_MOTION_INSTANCE_WORDS words when the history was made and now.
//   moved        = a bit of objectToWorld differs
//   toPrev       = objectToWorld_h o worldToObject_cur
//   normalToPrev = transpose of the 3 x 3 part of objectToWorld_cur o worldToObject_h: the inverse transpose of toPrev's, so that non-uniform scales are right
// each entry rounded once from the double product.
static inline MotionRec motion_record(const float* hist, const float* cur)
{
  MotionRec m;
  m.moved  = memcmp(hist, cur, 12 * sizeof(float)) != 0 ? 1u : 0u;
  m.pad[0] = m.pad[1] = m.pad[2] = 0u;
  for(int r = 0; r < 3; ++r)
  {
    for(int c = 0; c < 4; ++c)
      m.toPrev[4 * r + c] = float(motion_compose(hist, cur + 12, r, c));
    for(int c = 0; c < 3; ++c)
      m.normalToPrev[4 * r + c] = float(motion_compose(cur, hist + 12, c, r));
    m.normalToPrev[4 * r + 3] = 0.0f;
  }
  return m;
}

// The table of n instances: out[i] = motion_record of instance i
static inline void motion_table(const float* hist, const float* cur, uint32_t n, MotionRec* out)
{
  for(uint32_t i = 0; i < n; ++i)
    out[i] = motion_record(hist + size_t(i) * PT_MOTION_INSTANCE_WORDS, cur + size_t(i) * PT_MOTION_INSTANCE_WORDS);
}

// Pixel (px, py) of pt_temporal_accumulate_moving.  src is temporal_pixel's and has instance(px, py) besides, the instance plane's word at the pixel;
// table holds numInstances records (numInstances = 0: no table, nothing is read).  The word is tested against numInstances before anything of the table
// is read, whatever its bits (PT_INSTANCE_NONE included); the record beyond `moved` is read only where it is applied.
template <class Src>
PT_DN TemporalOut temporal_pixel_moving(const Src& src, const TemporalConst& k, const MotionRec* table, uint32_t numInstances, int px, int py, int w, int h,
                                        TemporalProbe* probe)
{
  const DnPx    c = src.colour(px, py), g1 = src.normal(px, py);
  const float   t = src.depth(px, py).x;
  PT_TEMPORAL_STEP_1
  TemporalPoint q{Px, Py, Pz};
  DnPx          gn = g1;
  const uint32_t i = src.instance(px, py);
  if(i < numInstances && table[i].moved)
  {
    const float* M = table[i].toPrev;
    q.Px = ((M[0] * Px + M[1] * Py) + M[2] * Pz) + M[3];
    q.Py = ((M[4] * Px + M[5] * Py) + M[6] * Pz) + M[7];
    q.Pz = ((M[8] * Px + M[9] * Py) + M[10] * Pz) + M[11];
    const float* N = table[i].normalToPrev;
    const float  sx = g1.x * 2.0f - 1.0f, sy = g1.y * 2.0f - 1.0f, sz = g1.z * 2.0f - 1.0f;  // the current normal
    const float  mx = (N[0] * sx + N[1] * sy) + N[2] * sz, my = (N[4] * sx + N[5] * sy) + N[6] * sz, mz = (N[8] * sx + N[9] * sy) + N[10] * sz;
    const float  minv = 1.0f / sqrtf(tp_dot3(mx, my, mz, mx, my, mz));  // unit()
    gn.x = (mx * minv + 1.0f) * 0.5f;
    gn.y = (my * minv + 1.0f) * 0.5f;
    gn.z = (mz * minv + 1.0f) * 0.5f;
  }
  TemporalOut o;
  temporal_resolve(src, k, c, g1, t, ox, oy, oz, q, gn, w, h, probe, o);
  return o;
}

// Src over row-major planes in ordinary memory, with the instance plane (the host build)
struct MoRowMajor : TpRowMajor {
  const uint32_t* ids;
  PT_DN_MEMBER uint32_t instance(int x, int y) const { return ids[size_t(y) * size_t(w) + size_t(x)]; }
};
