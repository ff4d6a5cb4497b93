// The device intrinsics the product's headers use, for g++ (test infrastructure: the host harness of the trace source, tests/host_harness.py).
// Every unit of the harness includes this first, then the product's headers through th_scene.h.
#pragma once
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime.h>  // vector types; nothing is launched
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

static inline unsigned int __float_as_uint(float f) { unsigned int u; std::memcpy(&u, &f, 4); return u; }
static inline float        __uint_as_float(unsigned int u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline int          __float_as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }
static inline float        __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }
template <class T>
static inline T atomicAdd(T* p, T v) { T o = *p; *p += v; return o; }
// a one-lane "wavefront" for the wave-level helpers of pt_machine.h (the ray supply is not used here; the per-lane state machine is)
static inline unsigned long long __ballot(int p) { return p ? 1ull : 0ull; }
static inline int                __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline unsigned int       __builtin_amdgcn_readfirstlane(unsigned int x) { return x; }
static const struct { unsigned x, y, z; } threadIdx = {0, 0, 0};

// experiment flavours only (tools/t2_robust_experiment.py): a candidate replacement of T2 takes the place of the contract's tri_test in every unit
#if defined(TH_ROBUST_T2) || defined(TH_CERTIFIED_T2)
#include "experiments/t2_variants.h"
#define TH_AFTER_RAYS() th_t2_fold()
#else
#define TH_AFTER_RAYS() ((void)0)
#endif
