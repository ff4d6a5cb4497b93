// One pixel of the guide pass ("Guide pass"): what pt_render_guides runs per lane (pt_guides.hip k_guides) to fill the denoiser's
// guide planes -- base colour, normal, depth -- from the first hit of the pixel's first camera ray.  Plain inline functions of plain values -- scene,
// image size, pixel, the lane's traversal stack, the counters -- so that tests/cpp/guides_host.cpp compiles them for the host, like pt_query.h, and
// tests/test_guides_host.py holds them pixel by pixel to the oracle's first-hit debug frames and to its closest-hit trace.
//
// Nothing of the trace contract is stated here: the ray is camera_ray's (pt_shade.h) for the first sample of frame 0, the walk is tail_closest on a
// path state of ONE slot in the lane's registers, exactly as query_ray sets it up (pt_query.h).  What IS stated a second time is the hit decode of
// shade_path: guide_surface below.  The render kernels compile from text this pass does not touch, so the decode is repeated instead of shared; the
// oracle comparison is what keeps the two from drifting apart.
#pragma once
#include "pt_shade.h"
#include "../../include/pt_api.h"  // PT_GUIDES_*

// the pixel's ray and what its walk found: `hit` is the path state's hit row (t, bits(ref | BVH_NONE), u, v), seedCamera / seedWalk the RNG state
// before and after the walk's alpha draws
struct GuideRay {
  f3       org, dir;
  float4   hit;
  uint32_t seedCamera, seedWalk;
};

// Camera ray of pixel (px, py) of a W x H image as generate_ray builds it for frame 0, sample 0 -- seed rng_tea(W * py + px, 0) in either variant,
// jitter (0.5, 0.5), then the two depth-of-field draws -- and its closest hit under the trace contract T5 (culling by instance flags, stochastic
// alpha drawn in key order from the running seed; no draw when every instance is opaque).
template <bool TWO>
PT_DEV GuideRay guide_ray(const DeviceScene& S, int W, int H, int px, int py, uint32_t* stack, Counters* counters)
{
  FrameParams fp{};  // frame 0, sample 0, PT_VARIANT_RAYQUERY: all camera_ray reads besides the size
  fp.st.size[0]    = W;
  fp.st.size[1]    = H;
  fp.st.maxSamples = 1;
  GuideRay g;
  uint32_t seed = 0u;
  camera_ray(S, fp, 0u, px, py, seed, g.org, g.dir);
  g.seedCamera = seed;
  // a path state of one slot, filled the way k_generate leaves it for the trace stages (pt_query.h query_ray)
  float4        rayO = make_float4(g.org.x, g.org.y, g.org.z, 0.0f), rayD = make_float4(g.dir.x, g.dir.y, g.dir.z, __uint_as_float(seed));
  float4        absorb = make_float4(0.0f, 0.0f, 0.0f, 0.0f), neeDir = make_float4(g.dir.x, g.dir.y, g.dir.z, 1.0f), hit = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  RenderBuffers rb{};
  rb.ps.rayO.p   = &rayO;
  rb.ps.rayD.p   = &rayD;
  rb.ps.absorb.p = &absorb;
  rb.ps.neeDir.p = &neeDir;
  rb.ps.hit.p    = &hit;
  rb.counters    = counters;
  uint32_t nAlpha = 0;  // (the draws a frame would count into pt_Stats::alphaTests: the guide pass touches no statistic)
  tail_closest<TWO>(S, rb, 0u, stack, nAlpha);
  g.hit      = rb.ps.hit[0];
  g.seedWalk = __float_as_uint(float4(rb.ps.rayD[0]).w);
  return g;
}

// The surface at a hit, as shade_path (pt_shade.h) has it when it reaches its debug exit: this restates its lines from "uint32_t hitInst, hitPrim"
// to "sf.albedo *= vcolor" -- instance / primitive from the hit reference (two-level: world triangle; flat: the slot's shading line when the
// structure carries them, its TriRec otherwise), the vertex triple, surface_at_hit, the face-forward normal, resolve_material_at, vertex colour.
PT_DEV Surface guide_surface(const DeviceScene& S, const float4& hit, f3 rdir)
{
  uint32_t     hitInst, hitPrim;
  int          hitMat = -2;  // material index when the shading line carries it (-2: take it from the instance record)
  VertexTriple vt;
  bool         haveVt = false;
  if(S.twoLevel)
  {
    const uint32_t w = __float_as_uint(hit.y);
    hitInst          = instance_of_world_tri(S, w);
    hitPrim          = w - S.instTriBase[hitInst];
  }
  else
  {
    const uint32_t hslot = __float_as_uint(hit.y);
    if(S.shadeTris)
    {
      vt              = fetch_triangle_slot(S, hslot);
      haveVt          = true;
      const float4 id = S.shadeTris[size_t(hslot) * PT_SHADE_REC_QUADS + 6];
      hitInst         = __float_as_uint(id.x);
      hitPrim         = __float_as_uint(id.y);
      hitMat          = int(__float_as_uint(id.z));
    }
    else
    {
      const TriRec tr = S.tris[hslot];
      hitInst         = __float_as_uint(tr.e1n.w);
      hitPrim         = __float_as_uint(tr.e2p.w);
    }
  }
  const InstanceRec& I = S.instances[hitInst];
  Surface            sf;
  f3                 vcolor;
  if(!haveVt)
    vt = fetch_triangle(S, I, hitPrim);
  surface_at_hit(S, I, vt, hit.z, hit.w, sf, vcolor);
  sf.ffnormal        = dot3(sf.normal, rdir) <= 0.0f ? sf.normal : -sf.normal;
  const int matIndex = hitMat != -2 ? hitMat : I.materialIndex;
  resolve_material_at(S, matIndex < 0 ? 0 : matIndex, rdir, sf);
  sf.albedo *= vcolor;
  return sf;
}

// the three planes of a pixel; a plane outside `planes` is left as it is
struct GuidePixel {
  float4 plane[PT_DENOISE_GUIDES];
};

// planes: PT_GUIDES_* mask of the planes wanted (the surface is only reconstructed for base colour or normal).  A hit gives (albedo, 1),
// ((normal + 1) / 2, 1) -- the eNormal encoding -- and (t, 0, 0, 0); a miss (0, 0, 0, 1) twice, what a debug frame with maxDepth >= 2 accumulates,
// and (missDepth, 0, 0, 0).  No clamp, no accumulation, no environment, no BSDF.
PT_DEV void guide_planes(const DeviceScene& S, const GuideRay& g, uint32_t planes, float missDepth, GuidePixel& out)
{
  const bool hit = __float_as_uint(g.hit.y) != BVH_NONE;
  if(planes & PT_GUIDES_DEPTH)
    out.plane[2] = make_float4(hit ? g.hit.x : missDepth, 0.0f, 0.0f, 0.0f);
  if(!(planes & (PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL)))
    return;
  f3 albedo = splat3(0.0f), normal = splat3(0.0f);
  if(hit)
  {
    const Surface sf = guide_surface(S, g.hit, g.dir);
    // 0 + value: a debug frame's pixel is the sample sum of accumulate_pixel, which starts at +0 (a component of -0 comes out as +0)
    albedo = splat3(0.0f) + sf.albedo;
    normal = splat3(0.0f) + (sf.normal + splat3(1.0f)) * .5f;
  }
  if(planes & PT_GUIDES_BASECOLOR)
    out.plane[0] = make_float4(albedo.x, albedo.y, albedo.z, 1.0f);
  if(planes & PT_GUIDES_NORMAL)
    out.plane[1] = make_float4(normal.x, normal.y, normal.z, 1.0f);
}
template <bool TWO>
PT_DEV void guide_pixel(const DeviceScene& S, int W, int H, int px, int py, uint32_t planes, float missDepth, uint32_t* stack, Counters* counters, GuidePixel& out)
{
  const GuideRay g = guide_ray<TWO>(S, W, H, px, py, stack, counters);
  guide_planes(S, g, planes, missDepth, out);
}

// The instance plane of DESIGN.md section 5.5: the node index of the hit guide_ray found -- guide_surface's hitInst, what pt_RayHit::instanceID reports for
// the same ray -- or PT_INSTANCE_NONE for a miss.  This restates the first lines of guide_surface for the instance alone (two-level: the world triangle's;
// flat: the slot's shading line when the structure carries them, its TriRec otherwise): sharing them as a function of their own changes the device code
// of k_guides (tools/device_code_diff.sh), and tests/test_instances_host.py holds both to the oracle on the same rays.
PT_DEV uint32_t guide_instance(const DeviceScene& S, const float4& hit)
{
  const uint32_t ref = __float_as_uint(hit.y);
  if(ref == BVH_NONE)
    return PT_INSTANCE_NONE;
  if(S.twoLevel)
    return instance_of_world_tri(S, ref);
  if(S.shadeTris)
    return __float_as_uint(S.shadeTris[size_t(ref) * PT_SHADE_REC_QUADS + 6].x);
  return __float_as_uint(S.tris[ref].e1n.w);
}
// One pixel of pt_render_instance_plane: guide_pixel's walk and planes (`planes` may be 0), and the instance plane's entry returned
template <bool TWO>
PT_DEV uint32_t instance_pixel(const DeviceScene& S, int W, int H, int px, int py, uint32_t planes, float missDepth, uint32_t* stack, Counters* counters, GuidePixel& out)
{
  const GuideRay g = guide_ray<TWO>(S, W, H, px, py, stack, counters);
  guide_planes(S, g, planes, missDepth, out);
  return guide_instance(S, g.hit);
}
