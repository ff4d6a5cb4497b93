// Whole frames with the product's shading source on the host (unit of the host harness, tests/host_harness.py): environment, camera, th_render_shard.
// What k_generate / k_tail / k_accumulate do per lane (pt_shade.h, pt_settle.h), run as a loop over the path slots of one frame at a time:
// camera ray, then per bounce closest hit -> shade_path -> shadow ray -> NEE add + Russian roulette, then the running mean.  Same tile / slot
// layout as the device (32 x 32 pixel tiles of 16 8x8 blocks).  The caller compares the image with the oracle bit for bit.
#include "th_walk.h"

extern "C" int pt_build_env_accel(const float* rgba32f, int width, int height, pt_EnvAccel* out, float* out_integral, float* out_average);

namespace {
// one path from its camera ray to its end (what the trace / shade stages do to a slot between k_generate and k_accumulate)
template <bool TWO>
void trace_path(const DeviceScene& S, const FrameParams& fp, int variant, uint32_t slot, WalkCtx& c)
{
  int px, py;
  if(!slot_pixel(fp, c.rb.slotTile, slot, px, py))
    return;
  generate_ray(S, c.rb, fp, slot, 0u, px, py);
  uint32_t nAlpha = 0;
  for(int depth = 0; depth < fp.st.maxDepth; ++depth)
  {
    tail_closest<TWO>(S, c.rb, slot, c.stack.data(), nAlpha);
    uint32_t  events = 0;
    const int to     = shade_path<-1>(S, c.rb, fp, slot, depth, events);
    bool      survive = to == SHADE_TO_NEXT;
    if(to == SHADE_TO_SHADOW)
    {
      uint32_t   seed;
      const bool inShadow = tail_shadow<TWO>(S, c.rb, slot, c.stack.data(), variant, seed, nAlpha);
      survive             = finish_bounce_core(c.rb, slot, inShadow, seed) && depth != fp.st.maxDepth - 1;
    }
    if(!survive)
      break;
  }
}
}  // namespace

extern "C" {

int th_set_env(void* p, const float* rgba, int w, int h, float* integral)
{
  Scene* s = static_cast<Scene*>(p);
  s->env.resize(size_t(w) * h);
  std::memcpy(s->env.data(), rgba, sizeof(float) * 4 * size_t(w) * h);
  s->envAccel.resize(size_t(w) * h);
  float avg = 0.f;
  const int rc = pt_build_env_accel(rgba, w, h, s->envAccel.data(), integral, &avg);
  for(DeviceScene* d : {&s->dsFlat, &s->dsTwo})
  {
    d->env = s->env.data(); d->envAccel = s->envAccel.data(); d->envW = w; d->envH = h;
  }
  return rc;
}
void th_set_camera(void* p, const pt_SceneCamera* cam, const pt_SunAndSky* ss)
{
  Scene* s = static_cast<Scene*>(p);
  for(DeviceScene* d : {&s->dsFlat, &s->dsTwo})
  {
    d->camera = *cam;
    d->sunsky = *ss;
  }
}
// frames 0 .. frames-1 of `st` (st->frame is ignored) accumulated like the device does; out: row-major width x height x 4.
// rank / nranks: the image-tile shard of pt_set_shard (tiles with (tx + ty) % nranks == rank, in increasing order: pt_resize); only the pixels
// of the rank's own tiles are written.
uint32_t th_render_shard(void* p, int two, const pt_RtxState* stIn, int variant, int frames, int rank, int nranks, float* out)
{
  Scene*             s = static_cast<Scene*>(p);
  const DeviceScene& S = two ? s->dsTwo : s->dsFlat;
  const int          W = stIn->size[0], H = stIn->size[1];
  FrameParams        fp;
  std::memset(&fp, 0, sizeof(fp));
  fp.st = *stIn; fp.width = W; fp.height = H; fp.tilesX = (W + PT_TILE - 1) / PT_TILE; fp.tilesY = (H + PT_TILE - 1) / PT_TILE;
  std::vector<uint32_t> slotTile;
  for(int ty = 0; ty < fp.tilesY; ++ty)
    for(int tx = 0; tx < fp.tilesX; ++tx)
      if((tx + ty) % nranks == rank)
        slotTile.push_back(uint32_t(ty * fp.tilesX + tx));
  fp.rank = rank; fp.nranks = nranks; fp.numLocalTiles = uint32_t(slotTile.size()); fp.numSlots = fp.numLocalTiles * 1024u; fp.batch = 1; fp.variant = variant;
  if(slotTile.empty())
    return 0;
  const uint32_t        n = fp.numSlots;
  std::vector<float4>   st9[9];
  for(auto& v : st9)
    v.assign(n, make_float4(0, 0, 0, 0));
  std::vector<float4>   frame(n, make_float4(0, 0, 0, 0));
  uint32_t      overflow = 0;
  RenderBuffers rb;
  std::memset(&rb, 0, sizeof(rb));
  rb.ps.rayO.p = st9[0].data(); rb.ps.rayD.p = st9[1].data(); rb.ps.thr.p = st9[2].data(); rb.ps.rad.p = st9[3].data(); rb.ps.absorb.p = st9[4].data();
  rb.ps.neeDir.p = st9[5].data(); rb.ps.neeRad.p = st9[6].data(); rb.ps.hit.p = st9[7].data(); rb.ps.sum.p = st9[8].data();
  rb.frame = frame.data(); rb.slotTile = slotTile.data();
  for(int f = 0; f < frames; ++f)
  {
    fp.st.frame = f;
    for(int smp = 0; smp < fp.st.maxSamples; ++smp)
    {
      fp.sample = smp;
      overflow += for_each_ray(n, 256, &rb, [&](WalkCtx& c, long long sl) {
        if(two)
          trace_path<true>(S, fp, variant, uint32_t(sl), c);
        else
          trace_path<false>(S, fp, variant, uint32_t(sl), c);
      });
#pragma omp parallel for schedule(static)
      for(long long ps = 0; ps < (long long)n; ++ps)
      {
        int px, py;
        if(slot_pixel(fp, rb.slotTile, uint32_t(ps), px, py))
          accumulate_pixel(rb, fp, uint32_t(ps));
      }
    }
  }
  for(uint32_t slot = 0; slot < n; ++slot)
  {  // k_untile
    int px, py;
    if(slot_pixel(fp, rb.slotTile, slot, px, py))
      std::memcpy(out + (size_t(py) * W + px) * 4, &frame[slot], 16);
  }
  return overflow;
}

}  // extern "C"
