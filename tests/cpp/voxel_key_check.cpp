// Stand-alone host check of the voxel key and its hash (fast_gicp_amd/csrc/voxel_key.hpp): the same functions the kernels build and look up
// their tables with. Prints, for a fixed list of coordinates -- 0, +-1, the largest legal index 2^20 - 4097 and its negative on every axis
// and together, and 4,000 pseudo-random ones over the whole legal range and near the origin -- the packed key and the home slot at
// capacities 1,024 / 8,192 / 65,536 ("K x y z key s1024 s8192 s65536"): tests/test_table_sim_cpu.py holds the numpy restatement
// (tests/table_sim.py) to these lines. Checked here: unpack_key(pack_key(.)) is the identity, keys are distinct from the empty key and stay
// within 63 bits, coord_in_range, and voxel_index_ok at limit - 1, at the limit, and for NaN and inf.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "voxel_key.hpp"

using namespace fvh;

static int fails = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      if (fails++ < 20) std::printf("MISMATCH line %d: %s\n", __LINE__, #cond); \
    }                                                                     \
  } while (0)

struct C3 { int x, y, z; };

int main() {
  const int lim = FVH_COORD_BIAS - 4096;  // voxel_index_ok refuses |index| >= lim
  const int big = lim - 1;
  std::vector<C3> list = {{0, 0, 0}, {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {1, 1, 1}, {-1, -1, -1},
                          {big, 0, 0}, {-big, 0, 0}, {0, big, 0}, {0, -big, 0}, {0, 0, big}, {0, 0, -big}, {big, big, big}, {-big, -big, -big}, {big, -big, big},
                          // what a neighbour offset of a legal base voxel can reach: past the limit, inside the 21 bits
                          {big + 3, 0, 0}, {0, -big - 3, 0}, {0, 0, -big - 3}, {FVH_COORD_BIAS - 1, FVH_COORD_BIAS - 1, FVH_COORD_BIAS - 1}, {-FVH_COORD_BIAS, -FVH_COORD_BIAS, -FVH_COORD_BIAS}};
  unsigned long long s = 0x243F6A8885A308D3ull;  // 64-bit LCG (Knuth's MMIX constants)
  auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); };
  for (int i = 0; i < 2000; i++) { C3 c; c.x = (int)(next() % (2u * big + 1u)) - big; c.y = (int)(next() % (2u * big + 1u)) - big; c.z = (int)(next() % (2u * big + 1u)) - big; list.push_back(c); }
  for (int i = 0; i < 2000; i++) { C3 c; c.x = (int)(next() % 129u) - 64; c.y = (int)(next() % 129u) - 64; c.z = (int)(next() % 33u) - 16; list.push_back(c); }  // a scene's worth of small consecutive integers
  for (const C3& c : list) {
    CHECK(coord_in_range(c.x, c.y, c.z));
    const unsigned long long k = pack_key(c.x, c.y, c.z);
    CHECK(k != FVH_EMPTY_KEY && k != FVH_EMPTY_KEY - 1 && (k >> 63) == 0);
    int x, y, z;
    unpack_key(k, x, y, z);
    CHECK(x == c.x && y == c.y && z == c.z);
    const unsigned s1 = hash_slot(k, 1023u), s2 = hash_slot(k, 8191u), s3 = hash_slot(k, 65535u);
    CHECK(s1 < 1024u && s2 < 8192u && s3 < 65536u && hash_slot(k, 0u) == 0u);
    CHECK(s1 == s2 >> 3 && s2 == s3 >> 3);  // the TOP bits of one hash
    std::printf("K %d %d %d %llu %u %u %u\n", c.x, c.y, c.z, k, s1, s2, s3);
  }
  // the 21-bit range itself
  CHECK(!coord_in_range(FVH_COORD_BIAS, 0, 0) && !coord_in_range(0, -FVH_COORD_BIAS - 1, 0) && !coord_in_range(0, 0, FVH_COORD_BIAS));
  // voxel_index_ok: the floating index is tested before any conversion to int
  const double dl = (double)lim, inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(voxel_index_ok(dl - 1.0, 0.0, 0.0) && voxel_index_ok(0.0, -(dl - 1.0), 0.0) && voxel_index_ok(0.0, 0.0, -(dl - 1.0)) && voxel_index_ok(dl - 1.0, dl - 1.0, dl - 1.0));
  CHECK(!voxel_index_ok(dl, 0.0, 0.0) && !voxel_index_ok(0.0, -dl, 0.0) && !voxel_index_ok(0.0, 0.0, dl) && !voxel_index_ok(0.0, 0.0, -dl));
  CHECK(!voxel_index_ok(nan, 0.0, 0.0) && !voxel_index_ok(0.0, nan, 0.0) && !voxel_index_ok(0.0, 0.0, nan));
  CHECK(!voxel_index_ok(inf, 0.0, 0.0) && !voxel_index_ok(0.0, -inf, 0.0) && !voxel_index_ok(0.0, 0.0, inf) && !voxel_index_ok(1e300, 0.0, 0.0));
  const float fl = (float)lim, finf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();  // (lim and lim - 1 are exact in float)
  CHECK(voxel_index_ok(fl - 1.0f, -(fl - 1.0f), fl - 1.0f) && !voxel_index_ok(fl, 0.0f, 0.0f) && !voxel_index_ok(0.0f, -fl, 0.0f) && !voxel_index_ok(0.0f, 0.0f, fl));
  CHECK(!voxel_index_ok(fnan, 0.0f, 0.0f) && !voxel_index_ok(0.0f, finf, 0.0f) && !voxel_index_ok(0.0f, 0.0f, -finf));
  // every legal index plus any offset the engine accepts (|offset| <= 511 in the packed form, far fewer in practice) stays inside the key
  CHECK(coord_in_range(big + 511, -big - 511, big + 511));
  std::printf("%zu coordinates checked, %d mismatches\n", list.size(), fails);
  return fails ? 1 : 0;
}
