// Host-only check of the MoE routing sort's index arithmetic (csrc/moe/moe_route_map.h). For a few
// thousand seeded (n = S * k, E, ids) vectors it replays the three launches of moe_route.hip on
// the host, loop for loop (count per chunk, scan per expert column and chunk segment, place per
// chunk / wave / step / lane with the peers of a step found through the id bits), every index
// taken from the header's functions, and asserts that the result is the stable sort of the slots
// by expert with the dropped ids left out, and that every index stays inside its table. Slot
// counts of chunk multiples +- 1, one expert taking everything and every id invalid are among the
// vectors. Built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_moe_route_native_host.py: the workspace and the outputs are heap arrays of their
// exact sizes. The assertions are in this program: it prints "route map ok" and returns 0, or names
// what failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "moe/moe_route_map.h"

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

static long g_vectors = 0, g_slots = 0;

static void check_vector(const std::vector<int64_t>& ids, int k, int E) {
  const int64_t n = (int64_t)ids.size();
  const int chunks = route_chunks(n);
  const int64_t words = route_workspace_words(n, E);
  CHECK(chunks >= 0 && (int64_t)chunks * kRouteChunk >= n && ((int64_t)chunks - 1) * kRouteChunk < n,
        "n=%lld: %d chunks", (long long)n, chunks);
  CHECK(words == ((int64_t)chunks + 1) * E, "workspace words %lld", (long long)words);
  int* ws = new int[words];
  for (int64_t i = 0; i < words; ++i) ws[i] = -12345;  // the launches rely on no initial content
  int* offsets = new int[E + 1];
  int* row_token = new int[n];
  int* slot_row = new int[n];
  for (int i = 0; i <= E; ++i) offsets[i] = -9;
  for (int64_t i = 0; i < n; ++i) row_token[i] = slot_row[i] = -9;
  auto tab = [&](int c, int e) {
    const int64_t i = route_table_index(c, e, E);
    CHECK(c >= 0 && c < chunks && e >= 0 && e < E && i >= 0 && i < (int64_t)chunks * E,
          "table index (%d, %d) -> %lld", c, e, (long long)i);
    return i;
  };
  auto tot = [&](int e) {
    const int64_t i = route_totals_index(chunks, e, E);
    CHECK(e >= 0 && e < E && i >= (int64_t)chunks * E && i < words, "totals index %d -> %lld", e,
          (long long)i);
    return i;
  };
  std::vector<char> seen(n, 0);  // every slot is taken by exactly one (chunk, wave, step, lane)

  // launch 1: count
  for (int c = 0; c < chunks; ++c) {
    std::vector<int> cnt(E, 0);
    for (int w = 0; w < kRouteWaves; ++w)
      for (int st = 0; st < kRouteSteps; ++st)
        for (int l = 0; l < 64; ++l) {
          const int64_t slot = route_slot(c, w, st, l);
          CHECK(slot >= 0, "slot %lld", (long long)slot);
          if (slot >= n) continue;
          ++seen[slot];
          const int e = route_expert(ids[slot], E);
          CHECK(e >= -1 && e < E, "expert %d", e);
          if (e >= 0) ++cnt[e];
        }
    for (int e = 0; e < E; ++e) ws[tab(c, e)] = cnt[e];
  }
  for (int64_t p = 0; p < n; ++p) CHECK(seen[p] == 1, "slot %lld taken %d times", (long long)p, seen[p]);

  // launch 2: scan
  const int col_groups = (E + kRouteScanCols - 1) / kRouteScanCols;
  for (int cg = 0; cg < col_groups; ++cg) {
    std::vector<int> seg_sum(kRouteScanSegs * kRouteScanCols, 0);
    int prev_c1 = 0;
    for (int seg = 0; seg < kRouteScanSegs; ++seg) {
      int c0 = -1, c1 = -1;
      route_scan_segment(chunks, kRouteScanSegs, seg, c0, c1);
      CHECK(c0 == prev_c1 && c1 >= c0 && c1 <= chunks, "segment %d of %d chunks: [%d, %d)", seg,
            chunks, c0, c1);
      prev_c1 = c1;
      for (int l = 0; l < kRouteScanCols; ++l) {
        const int e = cg * kRouteScanCols + l;
        if (e >= E) continue;
        int sum = 0;
        for (int c = c0; c < c1; ++c) sum += ws[tab(c, e)];
        seg_sum[seg * kRouteScanCols + l] = sum;
      }
    }
    CHECK(prev_c1 == chunks, "segments end at %d of %d", prev_c1, chunks);
    for (int seg = 0; seg < kRouteScanSegs; ++seg) {
      int c0, c1;
      route_scan_segment(chunks, kRouteScanSegs, seg, c0, c1);
      for (int l = 0; l < kRouteScanCols; ++l) {
        const int e = cg * kRouteScanCols + l;
        if (e >= E) continue;
        int run = 0, total = 0;
        for (int s = 0; s < kRouteScanSegs; ++s) {
          const int v = seg_sum[s * kRouteScanCols + l];
          run += s < seg ? v : 0;
          total += v;
        }
        for (int c = c0; c < c1; ++c) {
          const int64_t i = tab(c, e);
          const int v = ws[i];
          ws[i] = run;
          run += v;
        }
        if (seg == 0) ws[tot(e)] = total;
      }
    }
  }

  // launch 3: place
  const int bits = route_id_bits(E);
  CHECK(bits >= 0 && bits <= 10 && (1 << bits) >= E && (bits == 0 || (1 << (bits - 1)) < E),
        "E=%d: %d id bits", E, bits);
  for (int c = 0; c < chunks; ++c) {
    std::vector<int> ebase(E);
    int grand = 0;
    for (int e = 0; e < E; ++e) {
      ebase[e] = grand;
      grand += ws[tot(e)];
    }
    std::vector<int> tbl(kRouteWaves * E, 0);
    for (int w = 0; w < kRouteWaves; ++w)
      for (int st = 0; st < kRouteSteps; ++st)
        for (int l = 0; l < 64; ++l) {
          const int64_t slot = route_slot(c, w, st, l);
          const int e = slot < n ? route_expert(ids[slot], E) : -1;
          if (e >= 0) ++tbl[w * E + e];
        }
    for (int e = 0; e < E; ++e) {
      int base = ebase[e] + ws[tab(c, e)];
      for (int w = 0; w < kRouteWaves; ++w) {
        const int cnt = tbl[w * E + e];
        tbl[w * E + e] = base;
        base += cnt;
      }
    }
    for (int w = 0; w < kRouteWaves; ++w)
      for (int st = 0; st < kRouteSteps; ++st) {
        int key[64], base[64], rank[64], cnt[64];
        for (int l = 0; l < 64; ++l) {
          const int64_t slot = route_slot(c, w, st, l);
          key[l] = slot < n ? route_expert(ids[slot], E) : -1;
        }
        uint64_t ballot_valid = 0, ballot_bit[10] = {};  // the ballots: valid, then one per id bit
        for (int m = 0; m < 64; ++m) {
          ballot_valid |= (uint64_t)(key[m] >= 0) << m;
          for (int b = 0; b < bits; ++b) ballot_bit[b] |= (uint64_t)((key[m] >> b) & 1) << m;
        }
        for (int l = 0; l < 64; ++l) {
          uint64_t peers = ballot_valid;
          for (int b = 0; b < bits; ++b)
            peers &= ((key[l] >> b) & 1) ? ballot_bit[b] : ~ballot_bit[b];
          rank[l] = __builtin_popcountll(peers & ((1ull << l) - 1));
          cnt[l] = __builtin_popcountll(peers);
          base[l] = key[l] >= 0 ? tbl[w * E + key[l]] : 0;
          if (key[l] >= 0)
            for (int m = 0; m < 64; ++m)
              CHECK(((peers >> m) & 1) == (uint64_t)(key[m] == key[l]), "peers of lane %d", l);
        }
        for (int l = 0; l < 64; ++l)
          if (key[l] >= 0 && rank[l] == cnt[l] - 1) tbl[w * E + key[l]] = base[l] + cnt[l];
        for (int l = 0; l < 64; ++l) {
          const int64_t slot = route_slot(c, w, st, l);
          if (slot >= n) continue;
          const int row = key[l] >= 0 ? base[l] + rank[l] : -1;
          slot_row[slot] = row;
          if (key[l] >= 0) {
            CHECK(row >= 0 && row < grand && (int64_t)row < n, "row %d of %d", row, grand);
            if ((int64_t)row < n) row_token[row] = (int)(slot / k);
          }
        }
      }
    for (int i = 0; i < kRouteChunk; ++i) {
      const int64_t r = (int64_t)c * kRouteChunk + i;
      if (r >= grand && r < n) row_token[r] = -1;
    }
    if (c == 0) {
      for (int e = 0; e < E; ++e) offsets[e] = ebase[e];
      offsets[E] = grand;
    }
  }

  // the specification: a stable sort of the kept slots by expert
  std::vector<int64_t> kept;
  for (int64_t p = 0; p < n; ++p)
    if (ids[p] >= 0 && ids[p] < E) kept.push_back(p);
  std::stable_sort(kept.begin(), kept.end(), [&](int64_t a, int64_t b) { return ids[a] < ids[b]; });
  std::vector<int> want_off(E + 1, 0);
  for (int64_t p : kept) ++want_off[ids[p] + 1];
  for (int e = 0; e < E; ++e) want_off[e + 1] += want_off[e];
  if (n > 0) {
    for (int e = 0; e <= E; ++e)
      CHECK(offsets[e] == want_off[e], "n=%lld E=%d: offsets[%d] = %d, not %d", (long long)n, E, e,
            offsets[e], want_off[e]);
    std::vector<int> want_slot(n, -1);
    for (size_t r = 0; r < kept.size(); ++r) want_slot[kept[r]] = (int)r;
    for (int64_t r = 0; r < n; ++r) {
      const int want = r < (int64_t)kept.size() ? (int)(kept[r] / k) : -1;
      CHECK(row_token[r] == want, "n=%lld E=%d k=%d: row_token[%lld] = %d, not %d", (long long)n,
            E, k, (long long)r, row_token[r], want);
      CHECK(slot_row[r] == want_slot[r], "n=%lld E=%d: slot_row[%lld] = %d, not %d", (long long)n,
            E, (long long)r, slot_row[r], want_slot[r]);
    }
  }
  delete[] ws;
  delete[] offsets;
  delete[] row_token;
  delete[] slot_row;
  ++g_vectors;
  g_slots += n;
}

int main() {
  std::mt19937 rng(20261021u);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  const int64_t bad[] = {-1, -7, INT32_MAX, INT64_MAX, INT64_MIN, (int64_t)1 << 32};
  auto fill = [&](int64_t n, int E, int kind) {
    std::vector<int64_t> v(n);
    const int one = rnd(0, E - 1);
    for (int64_t p = 0; p < n; ++p) {
      switch (kind) {
        case 0: v[p] = rnd(0, E - 1); break;                        // uniform
        case 1: v[p] = one; break;                                  // one expert takes everything
        case 2: v[p] = p % 2 ? (int64_t)E + rnd(0, 3) : bad[rnd(0, 5)]; break;  // every id invalid
        case 3: v[p] = rnd(0, 9) == 0 ? (rnd(0, 1) ? (int64_t)E : bad[rnd(0, 5)])  // a tenth dropped
                                      : rnd(0, E - 1); break;
        case 4: v[p] = rnd(0, 3) ? one : rnd(0, E - 1); break;      // one heavy expert
        default: v[p] = (E - 1) - (p % E); break;                   // descending cycles
      }
    }
    return v;
  };
  const int C = kRouteChunk;
  const int sizes[] = {1, 2, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1,
                       3 * C + 7};
  for (int E : {1, 2, 3, 5, 63, 64, 65, 257, 1023, 1024})
    for (int64_t n : sizes)
      for (int kind = 0; kind < 6; ++kind)
        for (int k : {1, 2, 8}) check_vector(fill(n, E, kind), k, E);
  // seeded sizes, a few of them past one chunk per scan segment
  for (int rep = 0; rep < 400; ++rep) {
    const int E = rep % 3 == 0 ? rnd(1, 1024) : rnd(1, 40);
    const int64_t n = rep % 40 == 0 ? rnd(16 * C, 40 * C) : rnd(1, 4 * C);
    check_vector(fill(n, E, rep % 6), rnd(1, 9), E);
  }
  check_vector({}, 1, 4);  // no slots: no chunks, nothing indexed
  CHECK(route_chunks(INT32_MAX) == (1 << 21), "chunks of 2^31 - 1 slots");
  CHECK(route_workspace_words(INT32_MAX, 1024) == (((int64_t)1 << 21) + 1) * 1024, "64-bit words");
  CHECK(route_table_index((1 << 21) - 1, 1023, 1024) == ((int64_t)1 << 31) - 1, "64-bit index");
  CHECK(route_slot((1 << 21) - 1, kRouteWaves - 1, kRouteSteps - 1, 63) == ((int64_t)1 << 31) - 1,
        "64-bit slot");
  printf("%ld vectors, %ld slots, %d checks failed\n", g_vectors, g_slots, g_failed);
  if (g_failed == 0) printf("route map ok\n");
  fflush(stdout);
  return g_failed != 0 || ferror(stdout) ? 1 : 0;
}
