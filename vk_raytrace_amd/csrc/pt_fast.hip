// The kernel of the responsive history: the clamp of the long history the temporal step has just written to the local mean and
// spread of the fast history written beside it.  The per-pixel body is pt_fast.h; this unit holds the kernel and its launch.  The entry points and the
// two temporal steps stay in pt_temporal.hip.  No existing kernel is involved and none is compiled from other text than before.
#include "pt_stage.h"
#include "pt_fast.h"

// k_denoise's 32 x 16 tile (pt_denoise.hip), one pixel per lane: a wave covers two rows of 32 pixels.  The tile and its halo of R of the fast history
// are staged in LDS as fast_tap gives them -- 16 bytes per pixel: .rgb, and in .w whether the tap counts, so that the length plane is read once per
// pixel and not once per tap: (32 + 2 R) x (16 + 2 R) x 16 B = 9 792, 11 520 and 13 376 B for R = 1, 2, 3.  The taps of one lane are one 16-byte LDS
// read each; the 16 lanes a 16-byte read serves together lie in one row of the tile, on 256 consecutive bytes but for a rotation, which is every bank
// once: no row padding is needed for any R.  On the global side every lane loads and stores one float4 and one float, adjacent lanes adjacent pixels.
#define FC_TX 32
#define FC_TY 16
#define FC_BLOCK (FC_TX * FC_TY)

struct FcArgs {
  const float4* hf;   // Hf': read at the tile and its halo; nothing writes it in this launch
  const float*  hnf;  // Hnf': likewise
  float4*       hc;   // Hc': read and written by each lane at its own pixel only -- which is why in place is not a race
  float*        hn;   // Hn': likewise
  int           w, h;
  FastConst     k;
};

// taps read from the block's tile; pixel (ox, oy) of the image first
struct FcTile {
  const float4* tile;
  int           ox, oy, tw;
  __device__ DnPx tap(int x, int y) const { return stage_px(tile[(y - oy) * tw + (x - ox)]); }
};

// R: the radius as a template argument -- the tile's extent is then a constant and the window's two loops unroll (profiles/fast_kernel_usage.txt)
template <int R>
__global__ void __launch_bounds__(FC_BLOCK) k_fast_clamp(FcArgs a)
{
  constexpr int TW = FC_TX + 2 * R, TH = FC_TY + 2 * R;
  __shared__ float4 tile[TW * TH];
  const int x = int(blockIdx.x) * FC_TX + int(threadIdx.x), y = int(blockIdx.y) * FC_TY + int(threadIdx.y);
  const int ox = int(blockIdx.x) * FC_TX - R, oy = int(blockIdx.y) * FC_TY - R;
  for(int t = int(threadIdx.y) * FC_TX + int(threadIdx.x); t < TW * TH; t += FC_BLOCK)
  {
    const int gx = ox + t % TW, gy = oy + t / TW;
    if(gx < 0 || gx >= a.w || gy < 0 || gy >= a.h)
      continue;  // outside the image: no tap ever asks for it
    const size_t at = size_t(gy) * size_t(a.w) + size_t(gx);
    const DnPx   f  = fast_tap(stage_px(a.hf[at]), a.hnf[at]);
    tile[t]         = make_float4(f.x, f.y, f.z, f.w);
  }
  __syncthreads();
  if(x >= a.w || y >= a.h)
    return;
  const size_t at = size_t(y) * size_t(a.w) + size_t(x);
  FastConst    k  = a.k;
  k.radius        = R;
  const FastOut o = fast_clamp_pixel(FcTile{tile, ox, oy, TW}, k, stage_px(a.hc[at]), a.hn[at], x, y, a.w, a.h, nullptr);
  a.hc[at]        = make_float4(o.colour.x, o.colour.y, o.colour.z, o.colour.w);
  a.hn[at]        = o.length;
}

// k.radius is 1 .. PT_FAST_MAX_RADIUS (fast_constants)
void launch_fast_clamp(hipStream_t stream, const float4* hf, const float* hnf, float4* hc, float* hn, int w, int h, const FastConst& k)
{
  const dim3   grid = stage_grid(w, h, FC_TX, FC_TY), block(FC_TX, FC_TY);
  const FcArgs a{hf, hnf, hc, hn, w, h, k};
  if(k.radius == 1)
    k_fast_clamp<1><<<grid, block, 0, stream>>>(a);
  else if(k.radius == 2)
    k_fast_clamp<2><<<grid, block, 0, stream>>>(a);
  else
    k_fast_clamp<3><<<grid, block, 0, stream>>>(a);
}
