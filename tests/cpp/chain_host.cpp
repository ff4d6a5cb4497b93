// The host build of the chained guide pass: vk_raytrace_amd/csrc/pt_chain.h -- chain_pixel<TWO>, what pt_render_guides_chain's kernel runs per lane --
// compiled by g++, on the structures th_scene.h assembles.  A library of its own (tests/chain_host.py compiles and binds it); the
// scene handle is the one tests/host_harness.py TracedScene creates, the camera the one th_set_camera put into it.  tests/test_chain_host.py holds it to
// the first-hit guide pass, to the query host build and to a float32 restatement of the step; tests/test_chain_gpu.py holds the device to it.
#include "th_walk.h"
#include "pt_query.h"  // query_hit: (instance, primitive) of a link record's hit
#include "pt_chain.h"
#include "stage/stage_host_common.h"  // copy_why

#define CH_LINK_WORDS 28                                  // 32-bit words of a link record, see ch_links
#define CH_LINK_SLOTS (PT_GUIDE_CHAIN_MAX_LINKS + 1)      // records a pixel can have: one per followed surface and the end surface

extern "C" {

// chain_constants: the status, and the static reason in why_out (why_len bytes, may be NULL)
int ch_constants(const pt_GuideChain* chain, char* why_out, int why_len)
{
  const char* why = "";
  ChainConst  k;
  const int   rc = chain_constants(chain, &k, &why);
  copy_why(why, why_out, why_len);
  return rc;
}
// chain_need_plane
int ch_need_plane(int have, char* why_out, int why_len)
{
  const char* why = "";
  const int   rc  = chain_need_plane(have != 0, &why);
  copy_why(why, why_out, why_len);
  return rc;
}

// The planes of a W x H image on the flat (two = 0) or the two-level structure and its link plane; out0 / out1 / out2: W * H * 4 floats each, written
// only for the planes in `planes` (the others may be NULL); links: W * H words, always written.  *overflow: the traversal-stack overflows counted.
// Returns what chain_constants returns; nothing is written when that is not PT_OK.
int ch_chain(void* p, int two, int W, int H, const pt_GuideChain* chain, uint32_t planes, float miss_depth, float* out0, float* out1, float* out2, uint32_t* links,
             uint32_t* overflow)
{
  const char* why = "";
  ChainConst  k;
  const int   rc = chain_constants(chain, &k, &why);
  if(rc != PT_OK)
    return rc;
  Scene*             s = static_cast<Scene*>(p);
  const DeviceScene& S = two ? s->dsTwo : s->dsFlat;
  float* const       out[PT_DENOISE_GUIDES] = {out0, out1, out2};
  *overflow = for_each_ray((long long)W * H, 64, nullptr, [&](WalkCtx& c, long long i) {
    const int  px = int(i % W), py = int(i / W);
    GuidePixel g;
    links[i] = two ? chain_pixel<true>(S, k, W, H, px, py, planes, miss_depth, c.stack.data(), &c.cnt, g)
                   : chain_pixel<false>(S, k, W, H, px, py, planes, miss_depth, c.stack.data(), &c.cnt, g);
    for(int j = 0; j < PT_DENOISE_GUIDES; ++j)
      if(planes & (1u << j))
        std::memcpy(out[j] + size_t(i) * 4, &g.plane[j], 16);
  });
  return PT_OK;
}

// The link records of n pixels (pixels[i] = W * y + x): counts[i] records for pixel i -- one per surface its chain hit, the end surface included, none for
// a miss of the camera ray -- at out + (i * CH_LINK_SLOTS + r) * CH_LINK_WORDS.  A record, in 32-bit words: 0-2 origin, 3-5 direction, 6 the RNG state
// before the walk, 7 t, 8 instance, 9 primitive, 10-12 ffnormal, 13-15 position, 16 roughness, 17 metallic, 18 transmission, 19 eta, 20 thin-walled,
// 21-23 albedo (after *= vcolor), 24 class (CHAIN_END / MIRROR / GLASS / THIN / TIR), 25 u, 26 v, 27 the hit reference.  Returns like ch_chain.
int ch_links(void* p, int two, int W, int H, const pt_GuideChain* chain, float miss_depth, int n, const uint32_t* pixels, uint32_t* out, uint32_t* counts, uint32_t* overflow)
{
  const char* why = "";
  ChainConst  k;
  const int   rc = chain_constants(chain, &k, &why);
  if(rc != PT_OK)
    return rc;
  Scene*             s = static_cast<Scene*>(p);
  const DeviceScene& S = two ? s->dsTwo : s->dsFlat;
  *overflow = for_each_ray(n, 64, nullptr, [&](WalkCtx& c, long long i) {
    const int  px = int(pixels[i] % uint32_t(W)), py = int(pixels[i] / uint32_t(W));
    GuidePixel g;
    ChainLink  rec[CH_LINK_SLOTS];
    uint32_t   nr = 0;
    if(two)
      chain_pixel<true>(S, k, W, H, px, py, 0u, miss_depth, c.stack.data(), &c.cnt, g, rec, CH_LINK_SLOTS, &nr);
    else
      chain_pixel<false>(S, k, W, H, px, py, 0u, miss_depth, c.stack.data(), &c.cnt, g, rec, CH_LINK_SLOTS, &nr);
    counts[i] = nr;
    for(uint32_t r = 0; r < nr; ++r)
    {
      const ChainLink& l   = rec[r];
      const uint32_t   ref = __float_as_uint(l.hit.y);
      const pt_RayHit  h   = two ? query_hit<true>(S, ref, l.hit.x, l.hit.z, l.hit.w, 0u) : query_hit<false>(S, ref, l.hit.x, l.hit.z, l.hit.w, 0u);
      const float      f[CH_LINK_WORDS] = {l.org.x, l.org.y, l.org.z, l.dir.x, l.dir.y, l.dir.z, 0.0f, l.hit.x, 0.0f, 0.0f, l.ffnormal.x, l.ffnormal.y, l.ffnormal.z,
                                           l.position.x, l.position.y, l.position.z, l.roughness, l.metallic, l.transmission, l.eta, 0.0f, l.albedo.x, l.albedo.y, l.albedo.z,
                                           0.0f, l.hit.z, l.hit.w, 0.0f};
      uint32_t*        w = out + (size_t(i) * CH_LINK_SLOTS + r) * CH_LINK_WORDS;
      std::memcpy(w, f, sizeof(f));
      w[6] = l.seed; w[8] = h.instanceID; w[9] = uint32_t(h.primitiveID); w[20] = l.thin; w[24] = l.cls; w[27] = ref;
    }
  });
  return PT_OK;
}
}
