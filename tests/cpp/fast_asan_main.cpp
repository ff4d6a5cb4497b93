// A stand-alone program around vk_raytrace_amd/csrc/pt_fast.h for g++ -fsanitize=address,undefined (tests/test_fast_model.py builds and runs it):
// fast_clamp_pixel over hostile planes -- NaN, +-Inf, 3e38 whose square overflows, denormals, random words in the colours and in the lengths -- at image
// sizes narrower than the window, with every plane in a heap block of exactly w * h pixels.  Every tap has to be tested against the image before it is
// read: a read past a block ends the program.  Each result is also checked against what the definition leaves no freedom in: alpha untouched, a pixel
// that is not clamped returned bit for bit, a clamped channel inside [lo, hi], the length either kept or min(length, maxFast).
#include <cstdio>
#include <cstring>
#include <vector>
#include "pt_fast.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int main()
{
  const float special[] = {0.0f, -0.0f, nanf(""), INFINITY, -INFINITY, 3.0e38f, -3.0e38f, 1.0e-45f, 1.0e-39f, 1.0f, -1.0f, 0.5f, 1.0e18f, 2.0f, 7.0f};
  const int   ns = int(sizeof(special) / sizeof(special[0]));
  const int   sizes[][2] = {{1, 1}, {2, 1}, {1, 7}, {3, 40}, {13, 9}, {38, 22}, {5, 5}};
  uint32_t    seed = 97531u;
  auto        word = [&](int hostile) {
    const uint32_t r = lcg(seed);
    if(int((r >> 8) % 100u) >= hostile)
      return 1.0f + 0.25f * (float((r >> 16) & 0xffu) / 128.0f - 1.0f);  // an ordinary colour: 1 +- 25 %
    if(r & 0x10000u)
      return special[(r >> 20) % uint32_t(ns)];
    float    f;
    uint32_t u = lcg(seed);
    std::memcpy(&f, &u, 4);
    return f;
  };
  long pixels = 0, moved = 0, left = 0, skipped = 0;
  for(int round = 0; round < 400; ++round)
  {
    const int* sz = sizes[round % int(sizeof(sizes) / sizeof(sizes[0]))];
    const int  w = sz[0], h = sz[1], n = w * h;
    const int  hostile = (round / 7) % 3 == 0 ? 0 : (round / 7) % 3 == 1 ? 10 : 60;  // per cent of hostile words
    DnPx*      hf  = new DnPx[n];
    DnPx*      hc  = new DnPx[n];
    float*     hnf = new float[n];
    float*     hn  = new float[n];
    for(int p = 0; p < n; ++p)
    {
      hf[p]  = DnPx{word(hostile), word(hostile), word(hostile), word(hostile)};
      hc[p]  = DnPx{word(hostile), word(hostile), word(hostile), word(hostile)};
      hnf[p] = hostile && lcg(seed) % 5u == 0 ? word(100) : float(1u + lcg(seed) % 4u);
      hn[p]  = hostile && lcg(seed) % 5u == 0 ? word(100) : float(1u + lcg(seed) % 32u);
    }
    pt_FastParams prm{float(1u + lcg(seed) % 6u), float(lcg(seed) % 4u), 1 + int(lcg(seed) % 3u), 0u};
    FastConst     k;
    const char*   why = "";
    if(fast_constants(&prm, &k, &why) != PT_OK)
      return std::printf("parameters refused: %s\n", why), 4;
    const FcRowMajor src{hf, hnf, w};
    for(int y = 0; y < h; ++y)
      for(int x = 0; x < w; ++x)
      {
        const int     p = y * w + x;
        FastProbe     pr;
        const FastOut o = fast_clamp_pixel(src, k, hc[p], hn[p], x, y, w, h, &pr);
        pixels++;
        const int window = (2 * k.radius + 1) * (2 * k.radius + 1);
        if(!(pr.n >= 0.0f && pr.n <= float(window < n ? window : n)))
          return std::printf("pixel (%d, %d) of %d x %d: %g taps counted\n", x, y, w, h, pr.n), 2;
        skipped += pr.n < float(window);
        if(std::memcmp(&o.colour.w, &hc[p].w, 4) != 0)
          return std::printf("pixel (%d, %d): alpha changed\n", x, y), 2;
        if(!pr.moved)
        {
          left++;
          if(std::memcmp(&o.colour, &hc[p], sizeof(DnPx)) != 0 || std::memcmp(&o.length, &hn[p], 4) != 0)
            return std::printf("pixel (%d, %d): not moved, yet changed\n", x, y), 2;
          continue;
        }
        moved++;
        const float c[3] = {o.colour.x, o.colour.y, o.colour.z};
        for(int j = 0; j < 3; ++j)
          if(!(c[j] >= pr.lo[j] && c[j] <= pr.hi[j]))
            return std::printf("pixel (%d, %d) channel %d: %g outside [%g, %g]\n", x, y, j, c[j], pr.lo[j], pr.hi[j]), 2;
        if(!(pr.n >= 2.0f) || o.length != (k.maxFast < hn[p] ? k.maxFast : hn[p]))
          return std::printf("pixel (%d, %d): moved with %g taps, length %g from %g\n", x, y, pr.n, o.length, hn[p]), 2;
      }
    delete[] hf;
    delete[] hc;
    delete[] hnf;
    delete[] hn;
  }
  std::printf("%ld pixels, %ld moved, %ld left, %ld with skipped taps\n", pixels, moved, left, skipped);
  return moved > 0 && left > 0 && skipped > 0 ? 0 : 3;
}
