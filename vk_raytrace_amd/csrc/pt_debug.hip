// Device code that is not the product: the on-box calibration of the two rooflines (pt_measure_peaks), the fp32 transcendental contract evaluated
// on the device (pt_fpmath_eval) and the probe kernels that run single functions of the render path row by row for the tests (pt_probe.h).
#include <algorithm>
#include "pt_context.h"
#include "pt_probe.h"
#include "pt_accel_dump.h"

extern "C" {

// ---- on-box calibration of the two rooflines bench.py prices against (no reference counterpart) ------------------------------------------
// VALU issue: every lane runs 8 independent v_fmac_f32 chains (the form with the highest measured issue rate, tools/valu_peak.hip; inline asm: the
// compiler can neither pack two of them into v_pk_fma_f32 nor drop them), 8 waves per SIMD on every CU; the result is wave-instructions per second over the whole chip.
__global__ void __launch_bounds__(256) k_calib_valu(int iters, float* out)
{
  float a0 = threadIdx.x, a1 = a0 + 1.f, a2 = a0 + 2.f, a3 = a0 + 3.f, a4 = a0 + 4.f, a5 = a0 + 5.f, a6 = a0 + 6.f, a7 = a0 + 7.f;
  const float m = 0.999f, c = 0.001f;
  for(int i = 0; i < iters; ++i)
  {
    asm volatile("v_fmac_f32 %0, %8, %9\n v_fmac_f32 %1, %8, %9\n v_fmac_f32 %2, %8, %9\n v_fmac_f32 %3, %8, %9\n"
                 "v_fmac_f32 %4, %8, %9\n v_fmac_f32 %5, %8, %9\n v_fmac_f32 %6, %8, %9\n v_fmac_f32 %7, %8, %9\n"
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                 : "v"(m), "v"(c));
  }
  float s = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
  if(s == 12345.678f)
    out[0] = s;
}
// HBM streaming: float4 copy (read + write) and float4 read-only reduction over buffers far larger than the 256 MB Infinity Cache
__global__ void __launch_bounds__(256) k_calib_copy(const float4* __restrict__ src, float4* __restrict__ dst, size_t n)
{
  for(size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
    dst[i] = src[i];
}
__global__ void __launch_bounds__(256) k_calib_read(const float4* __restrict__ src, size_t n, float* out)
{
  float acc = 0.f;
  for(size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
  {
    float4 v = src[i];
    acc += (v.x + v.y) + (v.z + v.w);
  }
  if(acc == 12345.678f)
    out[0] = acc;
}
int pt_measure_peaks(pt_context* c, pt_Peaks* out)
{
  CTX_CHECK(c);
  if(!out)
    return c->fail(PT_ERR_INVALID, "pt_measure_peaks: null");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  hipDeviceProp_t prop;
  HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
  const int    cus = prop.multiProcessorCount;
  const size_t n   = size_t(1) << 26;  // 2^26 float4 = 1 GiB per buffer
  float4 *     a = nullptr, *b = nullptr;
  float*       sink = nullptr;
  hipEvent_t   e0 = nullptr, e1 = nullptr;
  auto         done = [&](int rc) {
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(sink);
    if(e0) (void)hipEventDestroy(e0);
    if(e1) (void)hipEventDestroy(e1);
    return rc;
  };
  if(hipMalloc(&a, n * 16) != hipSuccess || hipMalloc(&b, n * 16) != hipSuccess || hipMalloc(&sink, 64) != hipSuccess)
    return done(c->fail(PT_ERR_OOM, "pt_measure_peaks: out of device memory"));
  if(hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipMemsetAsync(a, 0, n * 16, c->stream) != hipSuccess)
    return done(c->fail(PT_ERR_HIP, "pt_measure_peaks: setup failed"));
  auto timed = [&](auto&& launch, int reps) -> double {
    launch();  // warm-up
    (void)hipEventRecord(e0, c->stream);
    for(int i = 0; i < reps; ++i)
      launch();
    (void)hipEventRecord(e1, c->stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    return double(ms) * 1e-3 / reps;
  };
  const int      iters = 4096;
  const unsigned blocks = unsigned(cus) * 8u;  // 8 blocks of 4 waves per CU = 8 waves per SIMD
  double         t = timed([&] { k_calib_valu<<<blocks, 256, 0, c->stream>>>(iters, sink); }, 5);
  out->valuWaveInstrPerSec = double(blocks) * 4.0 * double(iters) * 8.0 / t;
  t = timed([&] { k_calib_copy<<<unsigned(cus) * 16u, 256, 0, c->stream>>>(a, b, n); }, 5);
  out->hbmCopyBytesPerSec = 2.0 * double(n) * 16.0 / t;
  t = timed([&] { k_calib_read<<<unsigned(cus) * 16u, 256, 0, c->stream>>>(a, n, sink); }, 5);
  out->hbmReadBytesPerSec = double(n) * 16.0 / t;
  out->computeUnits = cus;
  out->clockMHz     = prop.clockRate / 1000;
  if(hipGetLastError() != hipSuccess)
    return done(c->fail(PT_ERR_HIP, "pt_measure_peaks: kernel failed"));
  return done(PT_OK);
}

// The fp32 transcendental contract evaluated on the device (include/pt_fpmath.h); tests hold it bit for bit to the host evaluation.
__global__ void k_fpmath(int fn, uint64_t n, const float* a, const float* b, float* out)
{
  uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  float x = a[i], y = b ? b[i] : 0.0f, r;
  switch(fn)
  {
    case PT_FN_SIN: r = pt_sin(x); break;
    case PT_FN_COS: r = pt_cos(x); break;
    case PT_FN_TAN: r = pt_tan(x); break;
    case PT_FN_ASIN: r = pt_asin(x); break;
    case PT_FN_ACOS: r = pt_acos(x); break;
    case PT_FN_ATAN2: r = pt_atan2(x, y); break;
    case PT_FN_EXP: r = pt_exp(x); break;
    case PT_FN_LOG: r = pt_log(x); break;
    default: r = pt_pow(x, y); break;
  }
  out[i] = r;
}
int pt_fpmath_eval(pt_context* c, int fn, uint64_t n, const float* a, const float* b, float* out)
{
  CTX_CHECK(c);
  if(fn < PT_FN_SIN || fn > PT_FN_POW || !a || !out || ((fn == PT_FN_ATAN2 || fn == PT_FN_POW) && !b))
    return c->fail(PT_ERR_INVALID, "pt_fpmath_eval: bad arguments");
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  float *dA = nullptr, *dB = nullptr, *dO = nullptr;
  int    rc = PT_OK;
  auto   done = [&](int r) {
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dO);
    return r;
  };
  if(hipMalloc(&dA, n * 4) != hipSuccess || hipMalloc(&dO, n * 4) != hipSuccess || (b && hipMalloc(&dB, n * 4) != hipSuccess))
    return done(c->fail(PT_ERR_OOM, "pt_fpmath_eval: out of device memory"));
  if(hipMemcpy(dA, a, n * 4, hipMemcpyHostToDevice) != hipSuccess || (b && hipMemcpy(dB, b, n * 4, hipMemcpyHostToDevice) != hipSuccess))
    return done(c->fail(PT_ERR_HIP, "pt_fpmath_eval: upload failed"));
  k_fpmath<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(fn, n, dA, dB, dO);
  if(hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(out, dO, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return done(c->fail(PT_ERR_HIP, "pt_fpmath_eval: kernel failed"));
  return done(rc);
}

}  // extern "C"

// ---- row probes (test hooks, not part of the ABI): one function of the render path per lane, row i of `in` -> row i of `out` ------------------
// The host side of a probe: `in` and `out` (n rows of in_stride / out_stride floats) go to the device -- `out` too, the kernels read it --,
// launch(dIn, dOut) enqueues the kernel on the context's stream, and `out` comes back.  Errors carry the entry point's name.
template <class Launch>
static int run_rows(pt_context* c, const char* who, uint32_t n, const float* in, int in_stride, float* out, int out_stride, Launch&& launch)
{
  float *dIn = nullptr, *dOut = nullptr;
  auto   done = [&](int r) {
    (void)hipFree(dIn); (void)hipFree(dOut);
    return r;
  };
  const size_t inBytes = size_t(n) * in_stride * 4, outBytes = size_t(n) * out_stride * 4;
  if(hipMalloc(&dIn, inBytes) != hipSuccess || hipMalloc(&dOut, outBytes) != hipSuccess)
    return done(c->fail(PT_ERR_OOM, "%s: out of device memory", who));
  if(hipMemcpy(dIn, in, inBytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dOut, out, outBytes, hipMemcpyHostToDevice) != hipSuccess)
    return done(c->fail(PT_ERR_HIP, "%s: upload failed", who));
  launch(dIn, dOut);
  if(hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost) != hipSuccess)
    return done(c->fail(PT_ERR_HIP, "%s: kernel failed", who));
  return done(PT_OK);
}
// The shading functions one at a time on the device (pt_probe.h: the functions shade_path calls, no formula of its own): one state per lane, row i of
// `in` -> row i of `out`.  tests/test_float_kat.py holds the result bit for bit to the host build of the same function (tests/cpp/trace_host.cpp).
__global__ void k_shading_probe(int fn, uint32_t n, const float* __restrict__ in, int inStride, float* __restrict__ out, int outStride, int inWords, int outWords)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  float row[PROBE_BSDF_IN], res[8];
  for(int k = 0; k < PROBE_BSDF_IN; ++k)
    row[k] = k < inWords ? in[size_t(i) * inStride + k] : 0.0f;
  for(int k = 0; k < 8; ++k)
    res[k] = 0.0f;
  shading_probe(fn, row, res);
  for(int k = 0; k < outWords; ++k)
    out[size_t(i) * outStride + k] = res[k];
}
extern "C" __attribute__((visibility("default"))) int pt_debug_shading_probe(pt_context* c, int fn, uint32_t n, const float* in, int in_stride, float* out, int out_stride)
{
  CTX_CHECK(c);
  int inWords = 0, outWords = 0;
  probe_row_words(fn, inWords, outWords);
  if(inWords == 0 || inWords > PROBE_BSDF_IN || outWords > 8 || !in || !out || in_stride < inWords || out_stride < outWords || n > (1u << 24))
    return c->fail(PT_ERR_INVALID, "pt_debug_shading_probe: bad arguments");
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return run_rows(c, "pt_debug_shading_probe", n, in, in_stride, out, out_stride, [&](const float* dIn, float* dOut) {
    k_shading_probe<<<dim3((n + 63) / 64), dim3(64), 0, c->stream>>>(fn, n, dIn, in_stride, dOut, out_stride, inWords, outWords);
  });
}
// The software texture path one call at a time on the device (pt_probe.h texture_probe), on the scene the context holds: one row per lane.  tests/test_texture_model.py
// holds the result bit for bit to the host build of the same function (tests/cpp/trace_host.cpp th_texture_probe); this is where the device's own index
// arithmetic (tex_index's 24-bit multiply) is seen.  Not part of the ABI.
__global__ void k_texture_probe(DeviceScene S, TexProbeLimits lim, int kind, uint32_t n, const float* __restrict__ in, int inStride, float* __restrict__ out, int outStride)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  float row[TEXP_IN], res[TEXP_OUT];
  for(int k = 0; k < TEXP_IN; ++k)
    row[k] = in[size_t(i) * inStride + k];
  for(int k = 0; k < TEXP_OUT; ++k)
    res[k] = out[size_t(i) * outStride + k];
  texture_probe(S, lim, kind, row, res);
  for(int k = 0; k < TEXP_OUT; ++k)
    out[size_t(i) * outStride + k] = res[k];
}
extern "C" __attribute__((visibility("default"))) int pt_debug_texture_probe(pt_context* c, int kind, uint32_t n, const float* in, int in_stride, float* out, int out_stride)
{
  CTX_CHECK(c);
  if(kind < 0 || kind >= TEXP_COUNT || !in || !out || in_stride < TEXP_IN || out_stride < TEXP_OUT || n > (1u << 24))
    return c->fail(PT_ERR_INVALID, "pt_debug_texture_probe: bad arguments");
  if(!c->haveScene)
    return c->fail(PT_ERR_STATE, "pt_debug_texture_probe before pt_set_scene");
  if(kind == TEXP_ENV && !c->haveEnv)
    return c->fail(PT_ERR_STATE, "pt_debug_texture_probe: no environment");
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  // what the device arrays are known to hold (an allocation is at least as large as its last upload)
  const size_t         mats = std::min(c->dMatLines.bytes / (sizeof(uint4) * PT_MAT_LINE_QUADS), std::min(c->dAlphaMats.bytes / sizeof(AlphaMat), c->dMaterials.bytes / sizeof(pt_GltfShadeMaterial)));
  const TexProbeLimits lim{uint32_t(c->dTexRecs.bytes / sizeof(TexRec)), uint32_t(mats), uint32_t(std::min<size_t>(c->dTexels.bytes / 4, 0xffffffffu))};
  return run_rows(c, "pt_debug_texture_probe", n, in, in_stride, out, out_stride, [&](const float* dIn, float* dOut) {
    k_texture_probe<<<dim3((n + 63) / 64), dim3(64), 0, c->stream>>>(c->scene, lim, kind, n, dIn, in_stride, dOut, out_stride);
  });
}
// A hit turned into a Surface on the device (pt_probe.h surface_probe), on the scene the context holds: one row per lane.  tests/test_surface_model.py holds the
// result bit for bit to the host build of the same function (tests/cpp/trace_host.cpp th_surface_probe) and reads the per-slot shading lines through it.
// Returns SURF_NO_DATA (1, no error) for SURF_SLOT when the scene has no shading lines.  Not part of the ABI.
__global__ void k_surface_probe(DeviceScene S, SurfProbeLimits lim, int kind, uint32_t n, const float* __restrict__ in, int inStride, float* __restrict__ out, int outStride)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  float row[SURF_IN], res[SURF_OUT];
  for(int k = 0; k < SURF_IN; ++k)
    row[k] = in[size_t(i) * inStride + k];
  for(int k = 0; k < SURF_OUT; ++k)
    res[k] = out[size_t(i) * outStride + k];
  (void)surface_probe(S, lim, kind, row, res);
  for(int k = 0; k < SURF_OUT; ++k)
    out[size_t(i) * outStride + k] = res[k];
}
extern "C" __attribute__((visibility("default"))) int pt_debug_surface_probe(pt_context* c, int kind, uint32_t n, const float* in, int in_stride, float* out, int out_stride)
{
  CTX_CHECK(c);
  if(kind < 0 || kind >= SURF_COUNT || !in || !out || in_stride < SURF_IN || out_stride < SURF_OUT || n > (1u << 24))
    return c->fail(PT_ERR_INVALID, "pt_debug_surface_probe: bad arguments");
  if(!c->haveScene)
    return c->fail(PT_ERR_STATE, "pt_debug_surface_probe before pt_set_scene");
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  if(kind == SURF_SLOT && c->scene.shadeTris == nullptr)
    return SURF_NO_DATA;
  // what the device arrays are known to hold (an allocation is at least as large as its last upload)
  const size_t mats = std::min(c->dMatLines.bytes / (sizeof(uint4) * PT_MAT_LINE_QUADS), c->dMaterials.bytes / sizeof(pt_GltfShadeMaterial));
  const size_t slots = c->scene.shadeTris ? std::min<size_t>(c->numTris, c->dShadeTris.bytes / (sizeof(float4) * PT_SHADE_REC_QUADS)) : 0;
  const SurfProbeLimits lim{uint32_t(std::min<size_t>(c->numInstances, c->dInstances.bytes / sizeof(InstanceRec))), uint32_t(std::min<size_t>(c->dIndices.bytes / 4, 0xffffffffu)),
                            uint32_t(std::min<size_t>(c->dVertices.bytes / 32, 0xffffffffu)), uint32_t(mats), uint32_t(c->dTexRecs.bytes / sizeof(TexRec)),
                            uint32_t(std::min<size_t>(c->dTexels.bytes / 4, 0xffffffffu)), uint32_t(slots)};
  return run_rows(c, "pt_debug_surface_probe", n, in, in_stride, out, out_stride, [&](const float* dIn, float* dOut) {
    k_surface_probe<<<dim3((n + 63) / 64), dim3(64), 0, c->stream>>>(c->scene, lim, kind, n, dIn, in_stride, dOut, out_stride);
  });
}
// The intersection arithmetic one call at a time on the device (pt_probe.h trace_probe: tri_test, world_tri, make_raybox, a node visit in both node forms, cn_plane,
// enter_instance), one row per lane; a row reads nothing but its own words.  tests/test_trace_gpu.py holds the result bit for bit to the host build of the same
// function (tests/cpp/trace_host.cpp th_trace_probe) and to the exact model of tests/golden/gen_trace_kat.py.  Not part of the ABI.
__global__ void k_trace_probe(int kind, uint32_t n, const float* __restrict__ in, int inStride, float* __restrict__ out, int outStride, int inWords, int outWords)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  float row[TRP_IN], res[TRP_OUT];
  for(int k = 0; k < TRP_IN; ++k)
    row[k] = k < inWords ? in[size_t(i) * inStride + k] : 0.0f;
  for(int k = 0; k < TRP_OUT; ++k)
    res[k] = k < outWords ? out[size_t(i) * outStride + k] : 0.0f;
  trace_probe(kind, row, res);
  for(int k = 0; k < outWords; ++k)
    out[size_t(i) * outStride + k] = res[k];
}
extern "C" __attribute__((visibility("default"))) int pt_debug_trace_probe(pt_context* c, int kind, uint32_t n, const float* in, int in_stride, float* out, int out_stride)
{
  CTX_CHECK(c);
  int inWords = 0, outWords = 0;
  trace_row_words(kind, inWords, outWords);
  if(inWords == 0 || inWords > TRP_IN || outWords > TRP_OUT || !in || !out || in_stride < inWords || out_stride < outWords || n > (1u << 24))
    return c->fail(PT_ERR_INVALID, "pt_debug_trace_probe: bad arguments");
  if(n == 0)
    return PT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return run_rows(c, "pt_debug_trace_probe", n, in, in_stride, out, out_stride, [&](const float* dIn, float* dOut) {
    k_trace_probe<<<dim3((n + 63) / 64), dim3(64), 0, c->stream>>>(kind, n, dIn, in_stride, dOut, out_stride, inWords, outWords);
  });
}
// One level of the offscreen image the display pass samples (pt_capi.hip display_chain: the very function pt_tonemap_zoom runs), copied back for
// tests/test_display_gpu.py: the zero padding of a de-scaled viewport and every vkCmdBlitImage(LINEAR) level, which the RGBA8 image only shows through
// the exposure.  Returns the number of levels of the full chain; a level outside it copies nothing.
extern "C" __attribute__((visibility("default"))) int pt_debug_display_level(pt_context* c, int disp_w, int disp_h, int level, float* out, int* w, int* h)
{
  CTX_CHECK(c);
  MipView mv{};
  int     rc = display_chain(c, disp_w, disp_h, true, nullptr, mv);
  if(rc != PT_OK)
    return rc;
  if(level >= 0 && level < mv.n)
  {
    if(w) *w = mv.w[level];
    if(h) *h = mv.h[level];
    if(out)
      HIP_TRY(c, hipMemcpyAsync(out, mv.level[level], sizeof(float4) * size_t(mv.w[level]) * mv.h[level], hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, sync_all(c));
  rc = check_traversal(c);
  return rc != PT_OK ? rc : mv.n;
}
// The per-bounce counter block (pt_internal.h CNT_*, CNT_STRIDE words per bounce) of the newest launch sequence that has finished, as it came back for the
// queue-size feedback: queue sizes, the rays the packet stage handed on (CNT_REDO, CNT_HANDOVER) and the rays sent to the exact loops.  Launches what is
// pending and waits.  Returns the number of bounces the sequence ran staged (at most max_bounces are copied); 0: no sequence has run.  Not part of the ABI.
extern "C" __attribute__((visibility("default"))) int pt_debug_bounce_counts(pt_context* c, uint32_t* out, int max_bounces)
{
  CTX_CHECK(c);
  if(!out || max_bounces < 0)
    return c->fail(PT_ERR_INVALID, "pt_debug_bounce_counts: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  const pt_context::FrameSlot* newest = nullptr;
  for(const pt_context::FrameSlot& fs : c->slots)
    if(fs.hCounts && fs.countsSeq > 0 && (!newest || fs.countsSeq > newest->countsSeq))
      newest = &fs;
  if(!newest)
    return 0;
  const int n = std::min(newest->countsDepths, PT_MAX_DEPTH);
  std::copy(newest->hCounts, newest->hCounts + size_t(CNT_STRIDE) * size_t(std::min(n, max_bounces)), out);
  return n;
}
// The acceleration structure as it was built, copied back for tests/accel_audit.py (ids and info layout: pt_accel_dump.h).  Copies of buffers the context
// holds, no kernel.  pt_debug_accel_info fills at most `words` words of the info record and returns PT_DUMPI_WORDS.  Not part of the ABI.
extern "C" __attribute__((visibility("default"))) int pt_debug_accel_info(pt_context* c, uint32_t* out, int words)
{
  CTX_CHECK(c);
  if(!out || words < 0)
    return c->fail(PT_ERR_INVALID, "pt_debug_accel_info: bad arguments");
  if(!c->haveAccel)
    return c->fail(PT_ERR_STATE, "pt_debug_accel_info before pt_build_accel");
  uint32_t v[PT_DUMPI_WORDS] = {};
  v[PT_DUMPI_ACCEL_MODE] = uint32_t(c->accelMode); v[PT_DUMPI_NUM_TRIS] = c->numTris; v[PT_DUMPI_NUM_INSTANCES] = c->numInstances;
  v[PT_DUMPI_NUM_WIDE_NODES] = c->numWideNodes; v[PT_DUMPI_NODE_CAPACITY] = c->nodeCapacity; v[PT_DUMPI_NUM_BVH_NODES] = c->numBvhNodes;
  v[PT_DUMPI_NUM_TLAS_NODES] = c->numTlasNodes; v[PT_DUMPI_NUM_ACTIVE] = c->numActive; v[PT_DUMPI_NUM_BLAS] = c->numBlas;
  v[PT_DUMPI_MERGED_TRIS] = c->mergedTris; v[PT_DUMPI_MERGED_WIDE] = c->mergedWide; v[PT_DUMPI_MERGED_ONLY] = c->mergedOnly ? 1u : 0u;
  v[PT_DUMPI_HAVE_CNODES] = c->haveCNodes ? 1u : 0u; v[PT_DUMPI_HAVE_SHADE_TRIS] = c->haveShadeTris ? 1u : 0u;
  std::memcpy(&v[PT_DUMPI_MERGED_BOX], c->mergedBox, sizeof(c->mergedBox));
  v[PT_DUMPI_BUILDER] = uint32_t(c->tune.sahBuild);
  std::copy(v, v + std::min(words, int(PT_DUMPI_WORDS)), out);
  return PT_DUMPI_WORDS;
}
// Array `which` of the structure -> dst.  Returns the number of bytes the array holds (0: no such array in the current mode); copies nothing and returns
// PT_ERR_INVALID when `bytes` is smaller than that.
extern "C" __attribute__((visibility("default"))) long long pt_debug_accel_read(pt_context* c, int which, void* dst, size_t bytes)
{
  CTX_CHECK(c);
  if(which < 0 || which >= PT_DUMP_COUNT)
    return c->fail(PT_ERR_INVALID, "pt_debug_accel_read: no array %d", which);
  if(!c->haveAccel)
    return c->fail(PT_ERR_STATE, "pt_debug_accel_read before pt_build_accel");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  const bool two = c->accelMode == PT_ACCEL_TWO_LEVEL;
  size_t     slots = c->numTris;  // leaf records: every world triangle, or the merged structure's + one set per prim-mesh with an object-space BLAS
  if(two)
  {
    std::vector<char> merged(c->hInstances.size(), 0), seen;
    for(uint32_t i : c->hMerged)
      merged[i] = 1;
    slots = c->mergedTris;
    for(size_t i = 0; i < c->hInstances.size(); ++i)
    {
      const InstanceRec& I = c->hInstances[i];
      if(I.triCount == 0 || merged[i] || I.primMesh < 0)
        continue;
      if(seen.size() <= size_t(I.primMesh))
        seen.resize(size_t(I.primMesh) + 1, 0);
      if(!seen[I.primMesh])
        slots += I.triCount;
      seen[I.primMesh] = 1;
    }
  }
  const size_t   nodes = two ? c->nodeCapacity : c->numWideNodes;
  const size_t   cnodes = !c->haveCNodes ? 0 : (two && c->mergedOnly) ? c->mergedWide : nodes;
  const void*    src  = nullptr;
  bool           host = false;
  size_t         have = 0;
  const DevBuf*  buf  = nullptr;
  switch(which)
  {
    case PT_DUMP_WIDE: buf = &c->dWide; have = sizeof(WideNode) * nodes; break;
    case PT_DUMP_CNODES: buf = &c->dCNodes; have = sizeof(CompactNode) * cnodes; break;
    case PT_DUMP_TRIS: buf = &c->dTris; have = sizeof(TriRec) * slots; break;
    case PT_DUMP_ALPHA_RECS: buf = &c->dAlphaRecs; have = sizeof(AlphaRec) * slots; break;
    case PT_DUMP_BVH2: buf = &c->dBvh; have = two || !c->dBvh.p ? 0 : sizeof(BvhNode) * size_t(c->numBvhNodes); break;  // (released by a refit: stale)
    case PT_DUMP_TLAS: buf = &c->dTlas; have = two ? sizeof(WideNode) * size_t(c->numTlasNodes) : 0; break;
    case PT_DUMP_CTLAS: buf = &c->dCTlas; have = two && c->haveCNodes && !c->mergedOnly ? sizeof(CompactNode) * size_t(c->numTlasNodes) : 0; break;
    case PT_DUMP_TLAS_LEAVES: buf = &c->dTlasLeaves; have = two ? sizeof(TlasLeaf) * (size_t(c->numActive) + (c->mergedTris ? 1 : 0)) : 0; break;
    case PT_DUMP_INST_TRI_BASE: buf = &c->dInstTriBase; have = two ? 4 * size_t(c->numInstances) : 0; break;
    case PT_DUMP_INST_BLOCK: buf = &c->dInstBlock; have = two ? 4 * ((size_t(c->numTris) >> PT_INST_BLOCK_SHIFT) + 2) : 0; break;
    case PT_DUMP_INST_PAD: buf = &c->dInstPad; have = two ? 8 * size_t(c->numInstances) : 0; break;
    case PT_DUMP_ACTIVE: buf = &c->dActive; have = two ? 4 * size_t(c->numActive) : 0; break;
    case PT_DUMP_SHADE_TRIS: buf = &c->dShadeTris; have = c->haveShadeTris ? sizeof(float4) * PT_SHADE_REC_QUADS * size_t(two ? c->mergedTris : c->numTris) : 0; break;
    case PT_DUMP_INST_NODE_BASE: host = true; src = c->hInstNodeBase.data(); have = two ? 4 * c->hInstNodeBase.size() : 0; break;
    case PT_DUMP_BLAS_RANGES: host = true; src = c->hBlasRanges.data(); have = two ? 4 * c->hBlasRanges.size() : 0; break;
    default: host = true; src = c->hMerged.data(); have = two ? 4 * c->hMerged.size() : 0; break;  // PT_DUMP_MERGED_LIST
  }
  if(have == 0)
    return 0;
  if(!dst || bytes < have)
    return c->fail(PT_ERR_INVALID, "pt_debug_accel_read: array %d holds %zu bytes, the buffer %zu", which, have, bytes);
  if(host)
    std::memcpy(dst, src, have);
  else
  {
    if(!buf->p || buf->bytes < have)
      return c->fail(PT_ERR_STATE, "pt_debug_accel_read: array %d is not allocated", which);
    HIP_TRY(c, hipMemcpy(dst, buf->p, have, hipMemcpyDeviceToHost));
  }
  return (long long)have;
}
