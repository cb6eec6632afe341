// Host-only check of the padded K layout of the K-grouped GEMM and the grouped transposing
// quantiser (csrc/gemm/tile_map.h: kgrouped_range, kgrouped_capacity, with grouped_tile at
// BM = MOD). For MOD in {128, 256}, E in 1..9 and a few thousand offset vectors (all-empty,
// single-row groups, multiples of MOD plus or minus 1, non-monotone, negative, beyond T) it asserts
// that the groups' column ranges are disjoint, ascending multiples of MOD, that kl_g covers n_g
// with less than MOD to spare, that k0_E stays within the capacity (and reaches it for some
// vector), and that the quantiser's map (row tile -> group, rows, destination column) and the
// GEMM's range agree for every tile of the grid bound. Built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_gemm_kgrouped_native_host.py: the offsets array is
// allocated at its exact size, so a read past o[E] is reported. The assertions are in this
// program: it prints "kgrouped map ok" and returns 0, or names what failed.
#include <cstdint>
#include <cstdio>
#include <random>
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

static long g_vectors = 0, g_tiles = 0, g_attained = 0;

static void check_vector(const std::vector<int>& offs_in, int T, int MOD) {
  const int E = (int)offs_in.size() - 1;
  int* offs = new int[E + 1];  // exact size: one element past the end is an ASan report
  for (int i = 0; i <= E; ++i) offs[i] = offs_in[i];
  std::vector<int> o(E + 1);
  o[0] = grouped_clamp(offs[0], 0, T);
  for (int g = 0; g < E; ++g) o[g + 1] = grouped_clamp(offs[g + 1], o[g], T);
  const int64_t cap = kgrouped_capacity(T, E, MOD);
  CHECK(cap == ((int64_t)(T / MOD) + E) * MOD, "capacity %lld", (long long)cap);
  // the ranges: ascending, disjoint, back to back, multiples of MOD, covering n_g
  std::vector<int64_t> k0(E + 1), kl(E + 1);
  int64_t next = 0;
  for (int g = 0; g < E; ++g) {
    kgrouped_range(offs, T, E, MOD, g, k0[g], kl[g]);
    const int n = o[g + 1] - o[g];
    CHECK(k0[g] == next, "T=%d E=%d MOD=%d g=%d: k0 %lld, expected %lld", T, E, MOD, g,
          (long long)k0[g], (long long)next);
    CHECK(k0[g] % MOD == 0 && kl[g] % MOD == 0, "g=%d: [%lld, +%lld) off MOD", g,
          (long long)k0[g], (long long)kl[g]);
    CHECK(kl[g] >= n && kl[g] - n < MOD, "g=%d: kl %lld for %d rows", g, (long long)kl[g], n);
    CHECK((kl[g] == 0) == (n == 0), "g=%d: empty group and empty range differ", g);
    next = k0[g] + kl[g];
  }
  // g = E (and anything outside [0, E)): the empty range at k0_E
  kgrouped_range(offs, T, E, MOD, E, k0[E], kl[E]);
  CHECK(k0[E] == next && kl[E] == 0, "k0_E %lld (+%lld), expected %lld", (long long)k0[E],
        (long long)kl[E], (long long)next);
  CHECK(k0[E] <= cap, "T=%d E=%d MOD=%d: k0_E %lld > capacity %lld", T, E, MOD,
        (long long)k0[E], (long long)cap);
  if (k0[E] == cap) ++g_attained;
  int64_t a, b;
  kgrouped_range(offs, T, E, MOD, -1, a, b);
  CHECK(a == next && b == 0, "g = -1");
  kgrouped_range(offs, T, E, MOD, E + 7, a, b);
  CHECK(a == next && b == 0, "g = E + 7");
  // the quantiser's map: launch-wide row tile mt (ctiles column tiles each) -> group, rows of x,
  // destination column MOD * mt, which must lie in the GEMM's range of that group at the tile's
  // offset; every column of every range is written by exactly one tile
  for (int ctiles : {1, 3}) {
    const int64_t grid = grouped_grid_bound(T, E, MOD, ctiles);
    CHECK(grid <= (cap / MOD) * ctiles, "grid bound %lld over the capacity", (long long)grid);
    std::vector<int> hits((size_t)(cap / MOD), 0);
    for (int64_t wg = 0; wg < grid; ++wg) {
      GroupTile t{-1, -1, -1, -1, -1};
      if (!grouped_tile(offs, T, E, MOD, ctiles, (int)wg, t)) continue;
      ++g_tiles;
      const int64_t mt = wg / ctiles, d0 = mt * MOD;
      CHECK(t.tn == wg % ctiles, "column tile %d", t.tn);
      CHECK(d0 + MOD <= cap, "destination %lld past the capacity %lld", (long long)d0,
            (long long)cap);
      CHECK(d0 == k0[t.g] + (int64_t)t.tm * MOD && d0 + MOD <= k0[t.g] + kl[t.g],
            "T=%d E=%d MOD=%d wg=%lld: tile %d of group %d goes to column %lld, the range is "
            "[%lld, +%lld)", T, E, MOD, (long long)wg, t.tm, t.g, (long long)d0,
            (long long)k0[t.g], (long long)kl[t.g]);
      CHECK(t.row0 == o[t.g] && t.rows == o[t.g + 1] - o[t.g], "group %d rows", t.g);
      const int64_t first = (int64_t)t.row0 + (int64_t)t.tm * MOD;
      CHECK(first >= 0 && first < (int64_t)t.row0 + t.rows && (int64_t)t.row0 + t.rows <= T,
            "source rows from %lld leave the group", (long long)first);
      if (t.tn == 0 && d0 + MOD <= cap) ++hits[(size_t)mt];
    }
    for (int64_t m = 0; m < cap / MOD; ++m)
      CHECK(hits[(size_t)m] == (m * MOD < k0[E] ? 1 : 0), "column tile %lld written %d times",
            (long long)m, hits[(size_t)m]);
  }
  delete[] offs;
  ++g_vectors;
}

int main() {
  std::mt19937 rng(20261021u);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  for (int MOD : {128, 256}) {
    for (int E = 1; E <= 9; ++E) {
      for (int T : {0, 1, MOD - 1, MOD, MOD + 1, 5 * MOD, 5 * MOD + 7, 9 * MOD + E}) {
        check_vector(std::vector<int>(E + 1, 0), T, MOD);       // all-empty at 0
        check_vector(std::vector<int>(E + 1, T), T, MOD);       // all-empty at T
        check_vector(std::vector<int>(E + 1, T + 50), T, MOD);  // all > T
        check_vector(std::vector<int>(E + 1, -7), T, MOD);      // all negative
        std::vector<int> v(E + 1);
        for (int g = 0; g <= E; ++g) v[g] = g;  // single-row groups: the capacity's worst case
        check_vector(v, T, MOD);
        for (int d : {-1, 0, 1}) {              // multiples of MOD, plus or minus 1
          for (int g = 0; g <= E; ++g) v[g] = g * MOD + (g ? d : 0);
          check_vector(v, T, MOD);
          for (int g = 0; g <= E; ++g) v[g] = g * (MOD + d);
          check_vector(v, T, MOD);
        }
        for (int g = 0; g <= E; ++g) v[g] = (E - g) * MOD;  // decreasing
        check_vector(v, T, MOD);
        v.assign(E + 1, 0);
        v[E] = T;  // everything in the last group
        check_vector(v, T, MOD);
        v.assign(E + 1, T);
        v[0] = 0;  // everything in the first group
        check_vector(v, T, MOD);
        v[0] = INT32_MIN;
        v[E] = INT32_MAX;
        check_vector(v, T, MOD);
        // one row in every group but the last, which takes the rest: attains the capacity when
        // the rest is not a multiple of MOD
        for (int g = 0; g <= E; ++g) v[g] = g;
        v[E] = T;
        check_vector(v, T, MOD);
      }
      for (int rep = 0; rep < 160; ++rep) {
        const int T = rnd(0, 6 * MOD);
        std::vector<int> v(E + 1);
        const int kind = rep % 4;
        int run = kind == 1 ? rnd(0, 5) : 0;
        for (int g = 0; g <= E; ++g) {
          if (kind == 0) {            // anything in [-MOD, T + MOD]
            v[g] = rnd(-MOD, T + MOD);
          } else if (kind == 1) {     // monotone, steps of 0 / 1 / multiples of MOD / anything
            v[g] = run;
            const int s = rnd(0, 3);
            run += s == 0 ? 0 : s == 1 ? 1 : s == 2 ? MOD * rnd(0, 2) : rnd(0, 2 * MOD);
          } else if (kind == 2) {     // a partition of [0, T], shuffled a little
            v[g] = (int)((int64_t)T * g / E) + (rnd(0, 4) == 0 ? rnd(-MOD, MOD) : 0);
          } else {                    // sorted random points of [0, T]
            v[g] = rnd(0, T);
          }
        }
        if (kind == 3) {
          for (int i = 0; i <= E; ++i)
            for (int j = i + 1; j <= E; ++j)
              if (v[j] < v[i]) std::swap(v[i], v[j]);
        }
        check_vector(v, T, MOD);
      }
    }
  }
  CHECK(g_attained > 0, "no vector attains the capacity");
  CHECK(kgrouped_capacity(0, 3, 128) == 384 && kgrouped_capacity(1000, 2, 128) == 9 * 128 &&
            kgrouped_capacity(1000, 2, 256) == 5 * 256, "capacity values");
  CHECK(kgrouped_capacity(INT32_MAX, 1024, 128) > 0x7FFFFFFFLL, "64-bit capacity");
  {
    // T close to 2^31: one huge group, the arithmetic stays in range
    int* offs = new int[2]{0, INT32_MAX};
    int64_t k0, kl;
    kgrouped_range(offs, INT32_MAX, 1, 128, 0, k0, kl);
    CHECK(k0 == 0 && kl == ((int64_t)(INT32_MAX / 128) + 1) * 128, "kl at T = 2^31 - 1");
    delete[] offs;
  }
  printf("%ld vectors, %ld tiles, %ld attain the capacity, %d checks failed\n", g_vectors,
         g_tiles, g_attained, g_failed);
  if (g_failed == 0) printf("kgrouped map ok\n");
  fflush(stdout);
  return g_failed != 0 || ferror(stdout) ? 1 : 0;
}
