// The product's path-query body on the host (a unit of tests/paths_host.py's library, next to the units of the host harness; the reference of
// tests/test_paths_host.py and, for the device runs, of tests/test_paths_gpu.py).  vk_raytrace_amd/csrc/pt_paths.h -- path_query<TWO>, what
// pt_trace_paths' kernel runs per lane -- on the structures th_scene.h assembles, with the environment and camera
// th_set_env / th_set_camera (render_host.cpp) installed.
#include "th_walk.h"
#include "pt_paths.h"

namespace {
FrameParams path_params(const pt_RtxState* st, int variant)
{
  FrameParams fp;
  std::memset(&fp, 0, sizeof(fp));
  fp.st      = *st;
  fp.batch   = 1;
  fp.variant = variant;
  return fp;
}

// the rays of one path, in the order they are traced, as pt_Ray records: origin, direction, tmax = the ray's bound (PT_INFINITY for a closest-hit
// ray), seed = its kind (PT_RAYS_CLOSEST / PT_RAYS_OCCLUDED)
struct SegmentList {
  pt_Ray*   out;
  uint32_t  cap;
  uint32_t* n;
  void operator()(int kind, f3 o, f3 d, float bound) const
  {
    if(*n < cap)
    {
      pt_Ray& r = out[*n];
      r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z; r.tmax = bound;
      r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z; r.seed = uint32_t(kind);
    }
    ++*n;
  }
};
}  // namespace

extern "C" {

// n rays on the flat (two = 0) or the two-level structure under `st` (the fields section 3.2 reads); returns the traversal-stack overflows counted
uint32_t ph_paths(void* p, int two, const pt_RtxState* st, int variant, uint64_t n, const pt_Ray* rays, pt_PathResult* results)
{
  Scene*             s  = static_cast<Scene*>(p);
  const DeviceScene& S  = two ? s->dsTwo : s->dsFlat;
  const FrameParams  fp = path_params(st, variant);
  return for_each_ray((long long)n, 16, nullptr, [&](WalkCtx& c, long long r) {
    if(two)
      path_query<true>(S, fp, variant, rays[r], c.stack.data(), &c.cnt, results[r]);
    else
      path_query<false>(S, fp, variant, rays[r], c.stack.data(), &c.cnt, results[r]);
  });
}

// the camera rays of frame st->frame, sample 0, of a st->size image, row-major: camera_ray of pt_shade.h per pixel -> origin, direction and the seed
// after the camera's draws (what generate_ray stores); tmax = PT_INFINITY
void ph_camera_rays(void* p, const pt_RtxState* st, int variant, pt_Ray* out)
{
  Scene*             s  = static_cast<Scene*>(p);
  const DeviceScene& S  = s->dsFlat;  // (the camera is the same in both)
  const FrameParams  fp = path_params(st, variant);
  const int          W = st->size[0], H = st->size[1];
#pragma omp parallel for schedule(static)
  for(int py = 0; py < H; ++py)
    for(int px = 0; px < W; ++px)
    {
      uint32_t seed = 0u;
      f3       o, d;
      camera_ray(S, fp, 0u, px, py, seed, o, d);
      pt_Ray& r = out[size_t(py) * W + px];
      r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z; r.tmax = PT_INFINITY;
      r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z; r.seed = seed;
    }
}

// every ray the path(s) of `ray` traced, in order (SegmentList above): up to `cap` records in out; returns how many there were
uint32_t ph_path_segments(void* p, int two, const pt_RtxState* st, int variant, const pt_Ray* ray, pt_Ray* out, uint32_t cap)
{
  Scene*             s  = static_cast<Scene*>(p);
  const DeviceScene& S  = two ? s->dsTwo : s->dsFlat;
  const FrameParams  fp = path_params(st, variant);
  WalkCtx            c(nullptr);
  uint32_t           n = 0;
  pt_PathResult      r;
  const SegmentList  seg{out, cap, &n};
  if(two)
    path_query<true>(S, fp, variant, *ray, c.stack.data(), &c.cnt, r, seg);
  else
    path_query<false>(S, fp, variant, *ray, c.stack.data(), &c.cnt, r, seg);
  return n;
}

}  // extern "C"
