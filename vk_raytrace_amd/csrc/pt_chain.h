// One pixel of the chained guide pass (DESIGN.md section 5.8 is the definition): what pt_render_guides_chain runs per lane (pt_chain.hip k_guides_chain).
// The pixel's camera ray is followed through mirrors and clear glass -- the deterministic specular chain -- to the first surface that is neither, and the
// guide planes are written for THAT surface: plane 0 the product of the base colours along the chain, plane 1 the end surface's normal, plane 2 the
// summed length (the virtual depth: for a planar mirror org + dir * plane2 is the mirror image of the reflected point, which is what the temporal step
// reprojects).  Plain inline functions of plain values, like pt_guides.h, so that tests/cpp/chain_host.cpp compiles them for the host.
//
// Nothing of the trace contract or of the hit decode is stated here: the camera ray and its walk are guide_ray's, the surface is guide_surface's
// (pt_guides.h), every later walk is tail_closest on the one-slot path state query_ray sets up (pt_query.h), the directions are mirror / bend / unit
// (pt_math.h) and the next origin is the two lines shade_path uses for its next ray (pt_shade.h offset_ray).  With maxLinks == 0, or where nothing is
// followable, every plane is bit for bit guide_pixel's: 1 * x and +0 + t are exact.
#pragma once
#include "pt_guides.h"
#include "../../include/pt_types.h"  // pt_GuideChain, PT_GUIDE_CHAIN_*

// the checked parameters of a call
struct ChainConst {
  uint32_t maxLinks;
  float    maxRoughness, minMetallic, minTransmission;
};

PT_DEV bool chain_finite(float x) { return fabsf(x) <= 3.402823466e38f; }  // false for NaN and +-Inf

// PT_OK, or why the parameters cannot be used (`why`: static text).  Fills k when it is not NULL and the parameters are accepted.
inline int chain_constants(const pt_GuideChain* p, ChainConst* k, const char** why)
{
  if(!p)
    return *why = "null chain parameters", PT_ERR_INVALID;
  if(p->maxLinks > PT_GUIDE_CHAIN_MAX_LINKS)
    return *why = "maxLinks must be at most PT_GUIDE_CHAIN_MAX_LINKS (8)", PT_ERR_INVALID;
  if(!(p->maxRoughness >= 0.0f && p->maxRoughness <= 3.402823466e38f))  // (false for a NaN)
    return *why = "maxRoughness must be non-negative and finite", PT_ERR_INVALID;
  if(!(p->minMetallic >= 0.0f && p->minMetallic <= 3.402823466e38f))  // (false for a NaN)
    return *why = "minMetallic must be non-negative and finite", PT_ERR_INVALID;
  if(!(p->minTransmission >= 0.0f && p->minTransmission <= 3.402823466e38f))  // (false for a NaN)
    return *why = "minTransmission must be non-negative and finite", PT_ERR_INVALID;
  if(p->flags != 0u)
    return *why = "unknown flag bits", PT_ERR_INVALID;
  if(k)
    *k = ChainConst{p->maxLinks, p->maxRoughness, p->minMetallic, p->minTransmission};
  return PT_OK;
}
// pt_read_guide_chain without a link plane of the current size
inline int chain_need_plane(bool have, const char** why)
{
  if(!have)
    return *why = "no link plane (no pt_render_guides_chain since pt_resize)", PT_ERR_STATE;
  return PT_OK;
}

// what a surface is to the chain (a link record's class word)
#define CHAIN_END 0u     // not followed: the surface the planes are written for
#define CHAIN_MIRROR 1u  // followed along mirror(dir, ffnormal)
#define CHAIN_GLASS 2u   // followed along unit(bend(dir, ffnormal, eta))
#define CHAIN_THIN 3u    // thin-walled glass: the direction is kept
#define CHAIN_TIR 4u     // glass whose bend is the zero vector (total internal reflection): followed along mirror(dir, ffnormal)

// 0 (end), CHAIN_MIRROR or CHAIN_GLASS.  Every comparison is false for a NaN, which therefore gives `end`.
PT_DEV uint32_t chain_classify(const ChainConst& k, const Surface& sf)
{
  if(sf.unlit)
    return CHAIN_END;
  if(!(sf.roughness <= k.maxRoughness))
    return CHAIN_END;
  if(sf.metallic >= k.minMetallic)
    return CHAIN_MIRROR;
  if((1.0f - sf.metallic) * sf.transmission >= k.minTransmission)
    return CHAIN_GLASS;
  return CHAIN_END;
}

// One hit of a chain as the host build reports it (tests/cpp/chain_host.cpp ch_links): the ray that was walked with the RNG state before the walk, what
// the walk found, the surface values the step reads and the class.  The device passes no record: nothing of this is compiled there.
struct ChainLink {
  f3       org, dir;
  uint32_t seed;
  float4   hit;  // the path state's hit row: (t, bits(ref | BVH_NONE), u, v)
  f3       ffnormal, position, albedo;
  float    roughness, metallic, transmission, eta;
  uint32_t thin, cls;
};

#define CHAIN_END_SURFACE 0u  // a surface that is not followed
#define CHAIN_END_MISS 1u
#define CHAIN_END_LIMIT 2u    // a followable surface with links == maxLinks
#define CHAIN_END_DIR 3u      // a followable surface whose new direction is zero or not finite

// One walk of the chain after the camera ray's: tail_closest on the path state reset as query_ray sets it, from the running seed
template <bool TWO>
PT_DEV float4 chain_walk(const DeviceScene& S, f3 o, f3 d, uint32_t& seed, uint32_t* stack, Counters* counters)
{
  float4        rayO = make_float4(o.x, o.y, o.z, 0.0f), rayD = make_float4(d.x, d.y, d.z, __uint_as_float(seed));
  float4        absorb = make_float4(0.0f, 0.0f, 0.0f, 0.0f), neeDir = make_float4(d.x, d.y, d.z, 1.0f), hit = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  RenderBuffers rb{};
  rb.ps.rayO.p   = &rayO;
  rb.ps.rayD.p   = &rayD;
  rb.ps.absorb.p = &absorb;
  rb.ps.neeDir.p = &neeDir;
  rb.ps.hit.p    = &hit;
  rb.counters    = counters;
  uint32_t nAlpha = 0;  // (the chained pass touches no statistic either)
  tail_closest<TWO>(S, rb, 0u, stack, nAlpha);
  seed = __float_as_uint(float4(rb.ps.rayD[0]).w);
  return rb.ps.hit[0];
}

// The pixel's planes in `out` (a plane outside `planes` is left as it is) and its link word returned: links | end << 8.  rec / maxRec: where the host
// build wants the link records (one per hit, the end surface included; at most maxRec), *nRec their number; NULL on the device.
template <bool TWO>
PT_DEV uint32_t chain_pixel(const DeviceScene& S, const ChainConst& k, int W, int H, int px, int py, uint32_t planes, float missDepth, uint32_t* stack, Counters* counters,
                            GuidePixel& out, ChainLink* rec = nullptr, uint32_t maxRec = 0u, uint32_t* nRec = nullptr)
{
  const GuideRay g    = guide_ray<TWO>(S, W, H, px, py, stack, counters);
  f3             org  = g.org, dir = g.dir, tint = splat3(1.0f);
  float4         hit  = g.hit;
  uint32_t       seed = g.seedWalk, seedBefore = g.seedCamera, links = 0u, end = CHAIN_END_SURFACE, n = 0u;
  float          dist = 0.0f;
  Surface        sf{};
  for(;;)
  {
    if(__float_as_uint(hit.y) == BVH_NONE)
    {
      end = CHAIN_END_MISS;
      break;
    }
    sf           = guide_surface(S, hit, dir);
    uint32_t cls = chain_classify(k, sf);
    f3       L   = dir;
    if(cls != CHAIN_END && links == k.maxLinks)
    {
      cls = CHAIN_END;
      end = CHAIN_END_LIMIT;
    }
    else if(cls == CHAIN_MIRROR)
      L = mirror(dir, sf.ffnormal);
    else if(cls == CHAIN_GLASS)
    {
      if(sf.thinwalled)
        cls = CHAIN_THIN;
      else
      {
        const f3 b = bend(dir, sf.ffnormal, sf.eta);
        if(b.x == 0.0f && b.y == 0.0f && b.z == 0.0f)
        {
          cls = CHAIN_TIR;
          L   = mirror(dir, sf.ffnormal);
        }
        else
          L = unit(b);
      }
    }
    if(cls != CHAIN_END && (!(chain_finite(L.x) && chain_finite(L.y) && chain_finite(L.z)) || (L.x == 0.0f && L.y == 0.0f && L.z == 0.0f)))
    {
      cls = CHAIN_END;  // (tint, dist and links are still what they were before this hit)
      end = CHAIN_END_DIR;
    }
    if(rec && n < maxRec)
      rec[n++] = ChainLink{org, dir, seedBefore, hit, sf.ffnormal, sf.position, sf.albedo, sf.roughness, sf.metallic, sf.transmission, sf.eta, sf.thinwalled ? 1u : 0u, cls};
    if(cls == CHAIN_END)
      break;
    tint = tint * sf.albedo;
    dist = dist + hit.x;
    links += 1u;
    org        = offset_ray(sf.position, dot3(L, sf.ffnormal) > 0 ? sf.ffnormal : -sf.ffnormal);
    dir        = L;
    seedBefore = seed;
    hit        = chain_walk<TWO>(S, org, dir, seed, stack, counters);
  }
  if(nRec)
    *nRec = n;
  const bool miss = end == CHAIN_END_MISS;
  if(planes & PT_GUIDES_DEPTH)
    out.plane[2] = make_float4(miss ? (links == 0u ? missDepth : dist + missDepth) : dist + hit.x, 0.0f, 0.0f, 0.0f);
  f3 albedo = splat3(0.0f), normal = splat3(0.0f);
  if(!miss)
  {
    albedo = splat3(0.0f) + tint * sf.albedo;  // (0 + value, as guide_planes has it)
    normal = splat3(0.0f) + (sf.normal + splat3(1.0f)) * .5f;
  }
  else if(links != 0u)
    albedo = splat3(0.0f) + tint;
  if(planes & PT_GUIDES_BASECOLOR)
    out.plane[0] = make_float4(albedo.x, albedo.y, albedo.z, 1.0f);
  if(planes & PT_GUIDES_NORMAL)
    out.plane[1] = make_float4(normal.x, normal.y, normal.z, 1.0f);
  return links | end << 8;
}
