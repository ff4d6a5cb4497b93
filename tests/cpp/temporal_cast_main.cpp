// A stand-alone program around vk_raytrace_amd/csrc/pt_temporal.h for g++ -fsanitize=float-cast-overflow (tests/test_temporal_model.py builds and runs
// it): temporal_pixel over hostile cameras and depths.  Every index the header forms must come from a float that passed its range tests first; a
// conversion of anything else -- NaN, Inf, 3e38 -- is undefined behaviour that gives plausible numbers on x86 and is only seen by the sanitizer.
#include <cstdio>
#include <cstring>
#include <vector>
#include "pt_temporal.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int main()
{
  const float special[] = {0.0f, -0.0f, nanf(""), INFINITY, -INFINITY, 3.0e38f, -3.0e38f, 1.0e-45f, -1.0e-45f, 1.0e-39f, 1.0f, -1.0f, 0.5f, 1.0e18f, 1.0e19f, 7.0e9f, 2.2e9f, -2.2e9f};
  const int   ns = int(sizeof(special) / sizeof(special[0]));
  const int   w = 13, h = 9;
  uint32_t    seed = 12345u;
  auto        word = [&]() {
    const uint32_t r = lcg(seed);
    if(r & 0x10000u)
      return special[(r >> 20) % uint32_t(ns)];
    float    f;
    uint32_t u = lcg(seed);
    std::memcpy(&f, &u, 4);
    return f;
  };
  std::vector<DnPx>  c(w * h, DnPx{1, 1, 1, 1}), g1(w * h, DnPx{0.5f, 1, 0.5f, 1}), g2(w * h), hc(w * h, DnPx{2, 2, 2, 1}), hg(w * h, DnPx{0.5f, 1, 0.5f, 3});
  std::vector<float> hn(w * h, 1.0f);
  long               pixels = 0, history = 0;
  for(int round = 0; round < 400; ++round)
  {
    TemporalConst k;
    std::memset(&k, 0, sizeof(k));
    const float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(k.viewInverse, id, sizeof(id));
    std::memcpy(k.projInverse, id, sizeof(id));
    for(int i = 0; i < 16; ++i)
    {
      k.worldToClipH[i] = (round & 1) ? word() : ((lcg(seed) & 0x30000u) ? id[i] : word());
      if(round % 5 == 0 && (lcg(seed) & 0x70000u) == 0)
        k.viewInverse[i] = word();
    }
    for(int i = 0; i < 3; ++i)
      k.eyeH[i] = (round & 2) ? word() : 0.0f;
    k.haveHistory = 1;
    k.depthTol    = 1.0e30f;
    k.normalDist2 = 1.0f;
    k.maxHistory  = 8.0f;
    for(DnPx& d : g2)
      d = DnPx{(round % 3 == 0) ? 1.0f + float(lcg(seed) >> 24) : word(), 0, 0, 0};
    const TpRowMajor src{c.data(), g1.data(), g2.data(), hc.data(), hg.data(), hn.data(), w};
    for(int y = 0; y < h; ++y)
      for(int x = 0; x < w; ++x)
      {
        TemporalProbe pr;
        (void)temporal_pixel(src, k, x, y, w, h, &pr);
        for(int i = 0; i < 4; ++i)
          if(pr.verdict[i] != 0 && pr.verdict[i] != 2 && (pr.tapX[i] < 0 || pr.tapX[i] >= w || pr.tapY[i] < 0 || pr.tapY[i] >= h))
            return std::printf("tap (%d, %d) read outside the %d x %d image\n", pr.tapX[i], pr.tapY[i], w, h), 2;
        pixels++;
        history += pr.outcome <= PT_TEMPORAL_HISTORY_ONLY;
      }
  }
  std::printf("%ld pixels, %ld with history\n", pixels, history);
  return history > 0 ? 0 : 3;  // (a run in which nothing ever reaches the gather would prove nothing)
}
