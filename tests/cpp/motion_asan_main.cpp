// A stand-alone program around vk_raytrace_amd/csrc/pt_motion.h for g++ -fsanitize=address,undefined (tests/test_motion_model.py builds and runs it):
// temporal_pixel_moving over hostile instance planes -- words at numInstances, at 0x7fffffff, PT_INSTANCE_NONE, random words -- and hostile tables (huge
// translations, near-singular matrices, NaN), with the table in a heap block of exactly numInstances records.  The index bound has to come before any
// table read: a read past the block ends the program.  Each result is also compared with temporal_pixel's wherever the table must not have been applied.
#include <cstdio>
#include <cstring>
#include <vector>
#include "pt_motion.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int main()
{
  const float special[] = {0.0f, -0.0f, nanf(""), INFINITY, -INFINITY, 3.0e38f, -3.0e38f, 1.0e-45f, 1.0e-39f, 1.0f, -1.0f, 0.5f, 1.0e18f, 7.0e9f};
  const int   ns = int(sizeof(special) / sizeof(special[0]));
  const int   w = 13, h = 9, n = w * h;
  uint32_t    seed = 4321u;
  auto        word = [&]() {
    const uint32_t r = lcg(seed);
    if(r & 0x10000u)
      return special[(r >> 20) % uint32_t(ns)];
    float    f;
    uint32_t u = lcg(seed);
    std::memcpy(&f, &u, 4);
    return f;
  };
  std::vector<DnPx>     c(n, DnPx{1, 1, 1, 1}), g1(n, DnPx{0.5f, 1, 0.5f, 1}), g2(n), hc(n, DnPx{2, 2, 2, 1}), hg(n, DnPx{0.5f, 1, 0.5f, 3});
  std::vector<float>    hn(n, 1.0f);
  std::vector<uint32_t> ids(n);
  long                  pixels = 0, applied = 0, refused = 0, history = 0;
  for(int round = 0; round < 300; ++round)
  {
    const uint32_t num = uint32_t(round % 5);  // 0 .. 4 instances; the block below holds exactly that many records
    std::vector<float> hist(size_t(num) * PT_MOTION_INSTANCE_WORDS), cur(hist.size());
    const float        id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for(uint32_t i = 0; i < num; ++i)
      for(int part = 0; part < 2; ++part)
        for(int k = 0; k < 12; ++k)
        {
          hist[i * PT_MOTION_INSTANCE_WORDS + part * 12 + k] = id[k];
          cur[i * PT_MOTION_INSTANCE_WORDS + part * 12 + k]  = (round & 1) && (lcg(seed) & 0x30000u) == 0 ? word() : id[k] + ((i & 1) && k == 3 ? 0.25f : 0.0f);
        }
    MotionRec* table = num ? new MotionRec[num] : nullptr;
    motion_table(hist.data(), cur.data(), num, table);
    TemporalConst k;
    std::memset(&k, 0, sizeof(k));
    const float id4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(k.viewInverse, id4, sizeof(id4));
    std::memcpy(k.projInverse, id4, sizeof(id4));
    std::memcpy(k.worldToClipH, id4, sizeof(id4));
    k.haveHistory = 1;
    k.depthTol    = 1.0e30f;
    k.normalDist2 = 4.0f;
    k.maxHistory  = 8.0f;
    for(int p = 0; p < n; ++p)
    {
      g2[p] = DnPx{1.0f + float(lcg(seed) >> 26), 0, 0, 0};
      const uint32_t r = lcg(seed) >> 16;
      ids[p] = r % 6 == 0 ? num : r % 6 == 1 ? 0x7fffffffu : r % 6 == 2 ? 0xffffffffu : r % 6 == 3 ? lcg(seed) : r % 6 == 4 ? num + 1u + (lcg(seed) >> 8) : (num ? lcg(seed) % num : 0x80000000u);
    }
    MoRowMajor src{{c.data(), g1.data(), g2.data(), hc.data(), hg.data(), hn.data(), w}, ids.data()};
    for(int y = 0; y < h; ++y)
      for(int x = 0; x < w; ++x)
      {
        TemporalProbe     pr;
        const TemporalOut o = temporal_pixel_moving(src, k, table, num, x, y, w, h, &pr);
        const uint32_t    i = ids[size_t(y) * w + x];
        pixels++;
        history += pr.outcome <= PT_TEMPORAL_HISTORY_ONLY;
        if(i < num && table[i].moved)
        {
          applied++;
          continue;
        }
        refused++;
        const TemporalOut s = temporal_pixel(src, k, x, y, w, h, nullptr);
        if(std::memcmp(&o, &s, sizeof(o)) != 0)
          return std::printf("pixel (%d, %d), instance word 0x%x of %u: differs from the static form\n", x, y, i, num), 2;
      }
    delete[] table;
  }
  std::printf("%ld pixels, %ld applied, %ld not, %ld with history\n", pixels, applied, refused, history);
  return applied > 0 && refused > 0 && history > 0 ? 0 : 3;
}
