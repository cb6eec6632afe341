// Host-only check of the grouped GEMM's tile map (csrc/gemm/tile_map.h: grouped_tile,
// grouped_grid_bound, grouped_clamp). For BM in {128, 256}, E in 1..9 and a few thousand seeded
// offset vectors (all-empty, single-row groups, exact multiples of BM, non-monotone vectors,
// negative offsets and offsets > T among them) it walks every workgroup index of the grid bound and
// asserts that each (group, m-tile, n-tile) of the clamped offsets is produced exactly once, that
// every other index says "no tile", and that no produced row range leaves [0, T). Built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_gemm_grouped_native_host.py: the
// offsets array is allocated at its exact size, so a read past o[E] is reported. The assertions
// are in this program: it prints "grouped map ok" and returns 0, or names what failed.
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "gemm/tile_map.h"

using namespace ddlb;

static int g_failed = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      if (++g_failed <= 20) {                                  \
        printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
        printf(__VA_ARGS__);                                   \
        printf("\n");                                          \
      }                                                        \
    }                                                          \
  } while (0)

static long g_vectors = 0, g_tiles = 0, g_surplus = 0;

static void check_vector(const std::vector<int>& offs_in, int T, int BM, int tiles_n) {
  const int E = (int)offs_in.size() - 1;
  // exact-size heap copy: one element past the end is an ASan report
  int* offs = new int[E + 1];
  for (int i = 0; i <= E; ++i) offs[i] = offs_in[i];
  // the clamped offsets, by the rule of gemm.h
  std::vector<int> o(E + 1);
  o[0] = grouped_clamp(offs[0], 0, T);
  for (int g = 0; g < E; ++g) o[g + 1] = grouped_clamp(offs[g + 1], o[g], T);
  for (int g = 0; g <= E; ++g) CHECK(o[g] >= 0 && o[g] <= T, "clamped offset %d", o[g]);
  std::map<std::tuple<int, int, int>, int> want;
  for (int g = 0; g < E; ++g)
    for (int tm = 0; tm * BM < o[g + 1] - o[g]; ++tm)
      for (int tn = 0; tn < tiles_n; ++tn) want[{g, tm, tn}] = 0;
  const int64_t grid = grouped_grid_bound(T, E, BM, tiles_n);
  CHECK((int64_t)want.size() <= grid, "T=%d E=%d BM=%d: %zu tiles > bound %lld", T, E, BM,
        want.size(), (long long)grid);
  for (int64_t wg = 0; wg < grid; ++wg) {
    GroupTile t{-1, -1, -1, -1, -1};
    if (!grouped_tile(offs, T, E, BM, tiles_n, (int)wg, t)) {
      ++g_surplus;
      continue;
    }
    ++g_tiles;
    auto it = want.find({t.g, t.tm, t.tn});
    CHECK(it != want.end(), "T=%d E=%d BM=%d wg=%lld: tile (%d, %d, %d) does not exist", T, E, BM,
          (long long)wg, t.g, t.tm, t.tn);
    if (it == want.end()) continue;
    ++it->second;
    CHECK(t.row0 == o[t.g] && t.rows == o[t.g + 1] - o[t.g] && t.rows > 0,
          "group %d: rows [%d, +%d), not [%d, %d)", t.g, t.row0, t.rows, o[t.g], o[t.g + 1]);
    // the rows the tile may touch: [row0 + tm BM, row0 + min(rows, (tm + 1) BM))
    const int64_t first = (int64_t)t.row0 + (int64_t)t.tm * BM;
    const int64_t last = (int64_t)t.row0 + (t.rows < (t.tm + 1) * (int64_t)BM ? t.rows
                                                                                 : (t.tm + 1) * (int64_t)BM);
    CHECK(first >= 0 && first < last && last <= T, "rows [%lld, %lld) leave [0, %d)",
          (long long)first, (long long)last, T);
  }
  for (const auto& kv : want)
    CHECK(kv.second == 1, "T=%d E=%d BM=%d: tile (%d, %d, %d) produced %d times", T, E, BM,
          std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), kv.second);
  delete[] offs;
  ++g_vectors;
}

int main() {
  std::mt19937 rng(20260601u);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  for (int BM : {128, 256}) {
    for (int E = 1; E <= 9; ++E) {
      for (int tiles_n : {1, 3}) {
        // hand-made vectors
        for (int T : {0, 1, BM - 1, BM, BM + 1, 5 * BM, 5 * BM + 7}) {
          check_vector(std::vector<int>(E + 1, 0), T, BM, tiles_n);       // all-empty at 0
          check_vector(std::vector<int>(E + 1, T), T, BM, tiles_n);       // all-empty at T
          check_vector(std::vector<int>(E + 1, T + 50), T, BM, tiles_n);  // all > T
          check_vector(std::vector<int>(E + 1, -7), T, BM, tiles_n);      // all negative
          std::vector<int> v(E + 1);
          for (int g = 0; g <= E; ++g) v[g] = g;  // single-row groups
          check_vector(v, T, BM, tiles_n);
          for (int g = 0; g <= E; ++g) v[g] = g * BM;  // exact multiples of BM
          check_vector(v, T, BM, tiles_n);
          for (int g = 0; g <= E; ++g) v[g] = g * BM + (g ? 1 : 0);  // one row over, first group
          check_vector(v, T, BM, tiles_n);
          for (int g = 0; g <= E; ++g) v[g] = (E - g) * BM;  // decreasing
          check_vector(v, T, BM, tiles_n);
          v.assign(E + 1, 0);
          v[E] = T;  // everything in the last group
          check_vector(v, T, BM, tiles_n);
          v.assign(E + 1, T);
          v[0] = 0;  // everything in the first group
          check_vector(v, T, BM, tiles_n);
          v[0] = INT32_MIN;
          v[E] = INT32_MAX;
          check_vector(v, T, BM, tiles_n);
        }
        // seeded vectors: monotone, non-monotone, beyond T, mixes
        for (int rep = 0; rep < 120; ++rep) {
          const int T = rnd(0, 6 * BM);
          std::vector<int> v(E + 1);
          const int kind = rep % 4;
          int run = kind == 1 ? rnd(0, 5) : 0;
          for (int g = 0; g <= E; ++g) {
            if (kind == 0) {            // anything in [-BM, T + BM]
              v[g] = rnd(-BM, T + BM);
            } else if (kind == 1) {     // monotone, steps of 0 / 1 / multiples of BM / anything
              v[g] = run;
              const int s = rnd(0, 3);
              run += s == 0 ? 0 : s == 1 ? 1 : s == 2 ? BM * rnd(0, 2) : rnd(0, 2 * BM);
            } else if (kind == 2) {     // a partition of [0, T], shuffled a little
              v[g] = (int)((int64_t)T * g / E) + (rnd(0, 4) == 0 ? rnd(-BM, BM) : 0);
            } else {                    // sorted random points of [0, T]
              v[g] = rnd(0, T);
            }
          }
          if (kind == 3) {
            for (int i = 0; i <= E; ++i)
              for (int j = i + 1; j <= E; ++j)
                if (v[j] < v[i]) std::swap(v[i], v[j]);
          }
          check_vector(v, T, BM, tiles_n);
        }
      }
    }
  }
  // the bound's two terms, each where it is the smaller one, and a T near 2^31
  CHECK(grouped_grid_bound(1000, 2, 128, 3) == 3 * 9, "T / BM + E");
  CHECK(grouped_grid_bound(100, 8, 128, 2) == 2 * 8, "ceil(T / BM) * E");
  CHECK(grouped_grid_bound(0, 8, 128, 2) == 0, "T = 0");
  CHECK(grouped_grid_bound(INT32_MAX, 1024, 128, 1 << 20) > 0x7FFFFFFFLL, "64-bit bound");
  {
    // T close to 2^31: the tile arithmetic stays in range (one huge group, first and last tile)
    const int T = INT32_MAX, BM = 128;
    int* offs = new int[2]{0, INT32_MAX};
    GroupTile t{};
    const int64_t grid = grouped_grid_bound(T, 1, BM, 1);
    CHECK(grid == (int64_t)(T / BM) + 1, "bound at T = 2^31 - 1");
    CHECK(grouped_tile(offs, T, 1, BM, 1, 0, t) && t.tm == 0 && t.rows == T, "first tile");
    CHECK(grouped_tile(offs, T, 1, BM, 1, (int)(grid - 1), t) && t.tm == T / BM, "last tile");
    delete[] offs;
  }
  printf("%ld vectors, %ld tiles, %ld surplus workgroups, %d checks failed\n", g_vectors, g_tiles,
         g_surplus, g_failed);
  if (g_failed == 0) printf("grouped map ok\n");
  fflush(stdout);
  return g_failed != 0 || ferror(stdout) ? 1 : 0;
}
