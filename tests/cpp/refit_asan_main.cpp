// A stand-alone program around tests/cpp/refit_host.cpp for g++ -fsanitize=address,undefined (tests/test_refit_host.py builds and runs it): rfh_refit on
// structures the test wrote to a file -- a header of 9 uint32 counts (nodes, slots, node ranges, slot ranges, instances, vertices, indices, compact
// nodes present, shading lines), then the arrays in the order of rfh_refit's arguments -- each array in a heap block of exactly its size, so that a read
// or write past any of them ends the program.  The refit runs twice: the second one, over its own output with the same vertices, must change no word.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "refit_host.cpp"

static bool read_block(FILE* f, std::vector<uint32_t>& v, size_t words)
{
  v.resize(words);
  return words == 0 || fread(v.data(), 4, words, f) == words;
}

int main(int argc, char** argv)
{
  int cases = 0;
  for(int a = 1; a < argc; ++a)
  {
    FILE* f = fopen(argv[a], "rb");
    uint32_t n[9];
    if(!f || fread(n, 4, 9, f) != 9)
      return 2;
    std::vector<uint32_t> wide, tris, alpha, ranges, slots, inst, vertices, indices, cnodes, shade;
    if(!(read_block(f, wide, size_t(n[0]) * 32) && read_block(f, tris, size_t(n[1]) * 12) && read_block(f, alpha, size_t(n[1]) * 8) && read_block(f, ranges, size_t(n[2]) * 2) &&
         read_block(f, slots, size_t(n[3]) * 5) && read_block(f, inst, size_t(n[4]) * 32) && read_block(f, vertices, size_t(n[5]) * 8) && read_block(f, indices, n[6]) &&
         read_block(f, cnodes, n[7] ? size_t(n[0]) * 20 : 0) && read_block(f, shade, size_t(n[8]) * 32)))
      return 3;
    fclose(f);
    std::vector<float> rootBox(6 * size_t(n[2]));
    double             costs[2], again[2];
    auto run = [&](double* c) {
      return rfh_refit(n[0], wide.data(), n[1], tris.data(), alpha.data(), n[2], ranges.data(), n[3], slots.data(), n[4], inst.data(), n[5], reinterpret_cast<const float*>(vertices.data()), n[6],
                       indices.data(), n[7] ? cnodes.data() : nullptr, n[8], n[8] ? shade.data() : nullptr, rootBox.data(), c);
    };
    if(run(costs) != 0)
      return 4;
    const std::vector<uint32_t> w1 = wide, t1 = tris, a1 = alpha, c1 = cnodes, s1 = shade;
    if(run(again) != 0 || w1 != wide || t1 != tris || a1 != alpha || c1 != cnodes || s1 != shade || !(again[0] >= costs[1] * (1.0 - 1e-12) && again[0] <= costs[1] * (1.0 + 1e-12)))
      return 5;
    // a malformed input is refused, not read past: a primitive beyond the index buffer, a node range beyond the nodes
    const uint32_t keep = tris[slots[2] == RF_WORLD ? 11 : 3];
    tris[slots[2] == RF_WORLD ? 11 : 3] = 0x7fffffffu;
    if(run(again) != -4)
      return 6;
    tris[slots[2] == RF_WORLD ? 11 : 3] = keep;
    ranges[1] += n[0];
    if(run(again) != -2)
      return 7;
    printf("%s: %u nodes %u slots cost %.17g -> %.17g\n", argv[a], n[0], n[1], costs[0], costs[1]);
    ++cases;
  }
  printf("refit cases %d\n", cases);
  return 0;
}
