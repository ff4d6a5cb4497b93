// The product's gather-query body on the host (a unit of tests/gather_host.py's library, next to the units of the host harness and paths_host.cpp;
// the reference of tests/test_gather_host.py and, for the device runs, of tests/test_gather_gpu.py).  vk_raytrace_amd/csrc/pt_gather.h --
// gather_point<TWO, KIND>, what pt_gather's kernel runs per lane -- on the structures th_scene.h assembles, with the
// environment and camera th_set_env / th_set_camera (render_host.cpp) installed.
#include "th_walk.h"
#include "pt_gather.h"

namespace {
FrameParams gather_params(const pt_RtxState* st, int variant)
{
  FrameParams fp;
  std::memset(&fp, 0, sizeof(fp));
  fp.st      = *st;
  fp.batch   = 1;
  fp.variant = variant;
  return fp;
}

// the (origin, direction, seed at the start of the path) of every sample of a point, in sample order, as pt_Ray records (tmax = PT_INFINITY)
struct RayList {
  pt_Ray*   out;
  uint32_t  cap;
  uint32_t* n;
  void operator()(f3 o, f3 d, uint32_t seed) const
  {
    if(*n < cap)
    {
      pt_Ray& r = out[*n];
      r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z; r.tmax = PT_INFINITY;
      r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z; r.seed = seed;
    }
    ++*n;
  }
};

// one point into a 16-byte aligned record of its own (the SPHERE sums live in the record between samples, as float4 rows), then copied out: the
// caller's array may have any alignment
template <bool TWO, uint32_t KIND, class RAYS>
void one_point(const DeviceScene& S, const FrameParams& fp, int variant, const pt_GatherPoint& pt, WalkCtx& c, void* out, RAYS rays)
{
  constexpr size_t ROWS = KIND == PT_GATHER_HEMISPHERE ? 2 : 8;
  alignas(16) float4 rec[ROWS];
  std::memset(rec, 0, sizeof(rec));
  gather_point<TWO, KIND>(S, fp, variant, pt, rec, c.stack.data(), &c.cnt, rays);
  std::memcpy(out, rec, sizeof(rec));
}

template <class RAYS>
void dispatch(const DeviceScene& S, int two, uint32_t kind, const FrameParams& fp, int variant, const pt_GatherPoint& pt, WalkCtx& c, void* out, RAYS rays)
{
  if(kind == PT_GATHER_HEMISPHERE)
  {
    if(two)
      one_point<true, PT_GATHER_HEMISPHERE>(S, fp, variant, pt, c, out, rays);
    else
      one_point<false, PT_GATHER_HEMISPHERE>(S, fp, variant, pt, c, out, rays);
  }
  else
  {
    if(two)
      one_point<true, PT_GATHER_SPHERE>(S, fp, variant, pt, c, out, rays);
    else
      one_point<false, PT_GATHER_SPHERE>(S, fp, variant, pt, c, out, rays);
  }
}
}  // namespace

extern "C" {

// n points of `kind` on the flat (two = 0) or the two-level structure under `st` (the fields section 3.3 reads); results: pt_GatherResult[n] or
// pt_ProbeResult[n]; returns the traversal-stack overflows counted
uint32_t gh_gather(void* p, int two, const pt_RtxState* st, int variant, uint32_t kind, uint64_t n, const pt_GatherPoint* points, void* results)
{
  Scene*             s    = static_cast<Scene*>(p);
  const DeviceScene& S    = two ? s->dsTwo : s->dsFlat;
  const FrameParams  fp   = gather_params(st, variant);
  const size_t       recb = kind == PT_GATHER_HEMISPHERE ? sizeof(pt_GatherResult) : sizeof(pt_ProbeResult);
  return for_each_ray((long long)n, 4, nullptr, [&](WalkCtx& c, long long r) { dispatch(S, two, kind, fp, variant, points[r], c, (char*)results + size_t(r) * recb, GatherNoRays()); });
}

// the rays of the samples of one point (RayList above): up to `cap` records in out; returns how many there were (0 for an invalid point)
uint32_t gh_gather_rays(void* p, int two, const pt_RtxState* st, int variant, uint32_t kind, const pt_GatherPoint* point, pt_Ray* out, uint32_t cap)
{
  Scene*             s  = static_cast<Scene*>(p);
  const DeviceScene& S  = two ? s->dsTwo : s->dsFlat;
  const FrameParams  fp = gather_params(st, variant);
  WalkCtx            c(nullptr);
  uint32_t           n = 0;
  pt_ProbeResult     r;
  dispatch(S, two, kind, fp, variant, *point, c, &r, RayList{out, cap, &n});
  return n;
}

}  // extern "C"
