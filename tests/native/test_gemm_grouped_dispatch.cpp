// Host-only check of what gemm_launch (csrc/gemm/gemm_mfma.hip) decides for a grouped launch,
// GemmArgs::grp_offs: every accepted form (operands x dense / glu / quantised output / both)
// reaches launch_grouped with its arguments intact, an offered tile and a grid bound that is a
// grid, and one perturbation at a time is refused with hipErrorInvalidValue and no launch at all.
// gemm_mfma.hip holds no device code and calls no HIP API before an entry, so it is included here
// host-only and every entry of gemm_entry.h it calls is a stub that records its call. Built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_gemm_grouped_native_host.py. The
// assertions are in this program: it prints "grouped dispatch ok" and returns 0, or names what
// failed.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "gemm/gemm_mfma.hip"

namespace ddlb {

static const char* const kA = (const char*)0x10000000, * const kB = (const char*)0x20000000;
static char* const kC = (char*)0x30000000;
static const uint8_t* const kAS = (const uint8_t*)0x40000000, * const kBS = (const uint8_t*)0x50000000;
static uint8_t* const kCS = (uint8_t*)0x60000000;
static const uint64_t* const kTab = (const uint64_t*)0x70000000;
static const unsigned* const kFlags = (const unsigned*)0x78000000;
static const int* const kOffs = (const int*)0x7c000000;  // device memory: never read on the host

struct Launch {
  std::string entry;
  int din, dout, tile;
  GemmArgs p;
};
static std::vector<Launch> g_launches;

static hipError_t record(const char* name, int din, int dout, int tile, const GemmArgs& p) {
  g_launches.push_back({name, din, dout, tile, p});
  return hipSuccess;
}

#define FAST(NAME)                                                         \
  hipError_t launch_fast_##NAME(const GemmArgs& p, int tile, hipStream_t) { \
    return record(#NAME, -1, -1, tile, p);                                 \
  }
FAST(bf16_bf16) FAST(bf16_f32) FAST(f16_f16) FAST(f16_f32) FAST(fp8_bf16) FAST(fp8_f16)
FAST(fp8_f32) FAST(f32_f32)
#undef FAST
hipError_t launch_fast_mx(const GemmArgs& p, int dout, int tile, hipStream_t) {
  return record("mx", -1, dout, tile, p);
}
hipError_t launch_fast_mxs(const GemmArgs& p, int dout, int tile, hipStream_t) {
  return record("mxs", -1, dout, tile, p);
}
hipError_t launch_fast_mx4(const GemmArgs& p, int dout, int tile, hipStream_t) {
  return record("mx4", -1, dout, tile, p);
}
hipError_t launch_qout_fp8(const GemmArgs& p, int din, int tile, hipStream_t) {
  return record("qout_fp8", din, -1, tile, p);
}
hipError_t launch_qout_fp4(const GemmArgs& p, int din, int tile, hipStream_t) {
  return record("qout_fp4", din, -1, tile, p);
}
hipError_t launch_generic(const GemmArgs& p, int din, int dout, hipStream_t) {
  return record("generic", din, dout, -1, p);
}
hipError_t launch_grouped(const GemmArgs& p, int din, int dout, int tile, hipStream_t) {
  return record("grouped", din, dout, tile, p);
}

}  // namespace ddlb

using namespace ddlb;

static int g_failed = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      ++g_failed;                                              \
      printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                     \
      printf("\n");                                            \
    }                                                          \
  } while (0)

// The operand / dense-output pairs the grouped kernel is built for; each also runs gated, with a
// quantised output (fp8 / fp4) and with both.
struct Form {
  const char* name;
  int din, dout;
  bool scales;
};
static const Form kForms[] = {
    {"bf16_bf16", DT_BF16, DT_BF16, false}, {"bf16_f32", DT_BF16, DT_F32, false},
    {"f16_f16", DT_F16, DT_F16, false},     {"f16_f32", DT_F16, DT_F32, false},
    {"mxs_bf16", DT_FP8, DT_BF16, true},    {"mxs_f16", DT_FP8, DT_F16, true},
    {"mxs_f32", DT_FP8, DT_F32, true},      {"mx4_bf16", DT_FP4, DT_BF16, true},
    {"mx4_f16", DT_FP4, DT_F16, true},      {"mx4_f32", DT_FP4, DT_F32, true},
};
// epilogues: 0 dense, 1 glu, 2 quantised fp8, 3 quantised fp4, 4 glu + fp8, 5 glu + fp4
static const char* const kEpi[] = {"dense", "glu", "q8", "q4", "glu+q8", "glu+q4"};
static bool epi_glu(int e) { return e == 1 || e >= 4; }
static int epi_dout(int e, int dense) { return e == 2 || e == 4 ? DT_FP8 : e == 3 || e == 5 ? DT_FP4 : dense; }

struct Case {
  GemmArgs p;
  int din, dout, tile, mode;
};

static Case base_case(const Form& f, int epi, int T, int N, int K, int E, int tile) {
  Case c;
  c.din = f.din; c.dout = epi_dout(epi, f.dout); c.tile = tile; c.mode = GEMM_MODE_AUTO;
  GemmArgs& p = c.p;
  const bool glu = epi_glu(epi), quant = c.dout == DT_FP8 || c.dout == DT_FP4;
  const int cols = glu ? N / 2 : N;
  p.a = kA; p.b = kB; p.c = kC;
  p.M = T; p.N = N; p.K = K;
  p.lda = p.ldb = K; p.ldc = cols;
  p.glu = glu;
  p.grp_offs = kOffs; p.ngroups = E;
  p.b_gstride = (int64_t)N * K + 64;  // poison rows between the experts
  if (f.scales) {
    p.a_scale = kAS; p.b_scale = kBS;
    p.a_scale_ld = p.b_scale_ld = K / 32;
    p.b_scale_gstride = (int64_t)N * (K / 32) + 8;
  }
  if (quant) { p.c_scale = kCS; p.c_scale_ld = cols / 32; }
  return c;
}

static hipError_t launch(const Case& c) {
  g_launches.clear();
  return gemm_launch(c.p, c.din, c.dout, c.tile, c.mode, nullptr);
}

static void expect_accepted(const std::string& what, const Case& c) {
  const hipError_t e = launch(c);
  const char* w = what.c_str();
  CHECK(e == hipSuccess, "%s: returned %d", w, (int)e);
  CHECK(g_launches.size() == 1, "%s: %zu launches", w, g_launches.size());
  if (g_launches.size() != 1) return;
  const Launch& l = g_launches[0];
  CHECK(l.entry == "grouped", "%s: reached %s", w, l.entry.c_str());
  CHECK(l.din == c.din && l.dout == c.dout, "%s: dtypes %d -> %d", w, l.din, l.dout);
  CHECK(mxs_offers(l.tile), "%s: tile %d is not offered", w, l.tile);
  CHECK(c.tile == TILE_AUTO || l.tile == c.tile, "%s: tile %d became %d", w, c.tile, l.tile);
  // the arguments arrive as given, in elements
  CHECK(l.p.M == c.p.M && l.p.N == c.p.N && l.p.K == c.p.K && l.p.lda == c.p.lda &&
            l.p.ldb == c.p.ldb && l.p.ldc == c.p.ldc && l.p.a == c.p.a && l.p.b == c.p.b &&
            l.p.c == c.p.c && l.p.a_scale == c.p.a_scale && l.p.b_scale == c.p.b_scale &&
            l.p.c_scale == c.p.c_scale && l.p.c_scale_ld == c.p.c_scale_ld &&
            l.p.act == c.p.act && l.p.glu == c.p.glu && l.p.grp_offs == c.p.grp_offs &&
            l.p.ngroups == c.p.ngroups && l.p.b_gstride == c.p.b_gstride &&
            l.p.b_scale_gstride == c.p.b_scale_gstride && l.p.ksplit == 1 && l.p.tile_order == 0,
        "%s: arguments changed on the way", w);
  CHECK(l.p.a_grp == c.p.M && l.p.c_grp == c.p.M, "%s: rows not plain", w);
  // the grid the launch site will ask for: the bound of tile_map.h for the tile that arrived
  const int bm = tile_rows_of(l.tile), bn = tile_cols_of(l.tile);
  const int tiles_n = (c.p.N + bn - 1) / bn;
  const int64_t grid = grouped_grid_bound(c.p.M, c.p.ngroups, bm, tiles_n);
  const int64_t t1 = (int64_t)(c.p.M / bm) + c.p.ngroups;
  const int64_t t2 = (int64_t)((c.p.M + bm - 1) / bm) * c.p.ngroups;
  CHECK(grid == tiles_n * (t1 < t2 ? t1 : t2) && grid > 0 && grid <= 0x7FFFFFFFLL,
        "%s: grid bound %lld", w, (long long)grid);
}

static void expect_refused(const std::string& what, const Case& c) {
  const hipError_t e = launch(c);
  CHECK(e == hipErrorInvalidValue, "%s: returned %d, not hipErrorInvalidValue", what.c_str(), (int)e);
  CHECK(g_launches.empty(), "%s: %zu launches (%s)", what.c_str(), g_launches.size(),
        g_launches.empty() ? "" : g_launches[0].entry.c_str());
}

struct Perturbation {
  const char* name;
  std::function<bool(Case&)> apply;  // false: does not apply to this form
};

static std::vector<Perturbation> perturbations() {
  std::vector<Perturbation> v;
  auto add = [&](const char* n, std::function<bool(Case&)> f) { v.push_back({n, f}); };
  auto scaled = [](const Case& c) { return c.p.a_scale != nullptr; };
  auto quant = [](const Case& c) { return c.p.c_scale != nullptr; };
  add("flags", [](Case& c) { c.p.flags = kFlags; return true; });
  add("a_table", [](Case& c) { c.p.a_table = kTab; c.p.shard_rows = 256; return true; });
  add("c_table", [](Case& c) { c.p.c_table = kTab; c.p.c_shard_rows = 256; return true; });
  add("a_grp=64", [](Case& c) { c.p.a_grp = c.p.a_gstride = 64; return true; });
  add("c_grp=64", [](Case& c) { c.p.c_grp = c.p.c_gstride = 64; return true; });
  add("ksplit=2", [](Case& c) { c.p.ksplit = 2; c.p.lda = c.p.ldb = 2 * c.p.K; return true; });
  add("tile_order=1", [](Case& c) { c.p.tile_order = 1; return true; });
  add("ag_ctas=8", [](Case& c) { c.p.ag_ctas = 8; return true; });
  add("ag_mode=2", [](Case& c) { c.p.ag_mode = AG_AGENT_ACQUIRE; return true; });
  add("unit_scales", [=](Case& c) {
    if (c.din != DT_FP8) return false; c.p.a_scale = c.p.b_scale = nullptr; return true; });
  add("unit_scales_mode=mx", [=](Case& c) {
    if (c.din != DT_FP8) return false;
    c.p.a_scale = c.p.b_scale = nullptr; c.mode = GEMM_MODE_MX; return true; });
  add("a_scale_only", [=](Case& c) { if (!scaled(c)) return false; c.p.b_scale = nullptr; return true; });
  add("scales_on_16_bit", [=](Case& c) {
    if (scaled(c)) return false;
    c.p.a_scale = kAS; c.p.b_scale = kBS; c.p.a_scale_ld = c.p.b_scale_ld = c.p.K / 32;
    c.p.b_scale_gstride = (int64_t)c.p.N * (c.p.K / 32);
    return true; });
  add("f32_operands", [=](Case& c) {
    if (scaled(c)) return false; c.din = DT_F32; if (!quant(c)) c.dout = DT_F32; return true; });
  add("f64_operands", [=](Case& c) {
    if (scaled(c)) return false; c.din = DT_F64; if (!quant(c)) c.dout = DT_F64; return true; });
  add("dense_output_unpaired", [=](Case& c) {  // bf16 -> f16, f16 -> bf16
    if (scaled(c) || quant(c) || c.dout == DT_F32) return false;
    c.dout = c.dout == DT_BF16 ? DT_F16 : DT_BF16; return true; });
  add("mode=generic", [](Case& c) { c.mode = GEMM_MODE_GENERIC; return true; });
  static const struct { const char* name; int code; } kNotOffered[] = {
      {"tile=pt4", TILE_PT4}, {"tile=t4", TILE_T4}, {"tile=pt8", TILE_PT8}, {"tile=t8", TILE_T8},
      {"tile=256x256", TILE_256x256}, {"tile=256x256w4", TILE_256x256_W4},
      {"tile=i256", TILE_I256}, {"tile=i128", TILE_I128}, {"tile=i256w4", TILE_I256W4},
      {"tile=retired5", 5}, {"tile=unknown99", 99}};
  for (const auto& t : kNotOffered) {
    const int code = t.code;
    add(t.name, [=](Case& c) { c.tile = code; return true; });
  }
  add("ngroups=0", [](Case& c) { c.p.ngroups = 0; return true; });
  add("ngroups=-1", [](Case& c) { c.p.ngroups = -1; return true; });
  add("ngroups=1025", [](Case& c) { c.p.ngroups = 1025; return true; });
  add("grp_offs=null", [](Case& c) { c.p.grp_offs = nullptr; return true; });
  add("b_gstride<N*ldb", [](Case& c) { c.p.b_gstride = (int64_t)c.p.N * c.p.ldb - 64; return true; });
  add("b_gstride=0", [](Case& c) { c.p.b_gstride = 0; return true; });
  add("b_gstride_unaligned", [](Case& c) { c.p.b_gstride += 1; return true; });
  add("b_scale_gstride+2", [=](Case& c) {
    if (!scaled(c)) return false; c.p.b_scale_gstride += 2; return true; });
  add("b_scale_gstride+4_fp4", [=](Case& c) {
    if (c.din != DT_FP4) return false; c.p.b_scale_gstride += 4; return true; });
  add("b_scale_gstride<N*ld", [=](Case& c) {
    if (!scaled(c)) return false; c.p.b_scale_gstride -= 16; return true; });
  add("a_scale_ld+2", [=](Case& c) { if (!scaled(c)) return false; c.p.a_scale_ld += 2; return true; });
  add("c_scale_toggled", [=](Case& c) {
    if (quant(c)) c.p.c_scale = nullptr; else { c.p.c_scale = kCS; c.p.c_scale_ld = c.p.N / 32; }
    return true; });
  add("ldc_short", [](Case& c) { c.p.ldc -= 16; return true; });
  add("N-32", [](Case& c) { if (!c.p.glu && c.p.c_scale == nullptr) return false; c.p.N -= 32; return true; });
  add("lda<K", [](Case& c) { c.p.lda = c.p.K - 16; return true; });
  add("K=0", [](Case& c) { c.p.K = 0; return true; });
  add("M=-1", [](Case& c) { c.p.M = -1; return true; });
  add("a=null", [](Case& c) { c.p.a = nullptr; return true; });
  add("c=null", [](Case& c) { c.p.c = nullptr; return true; });
  return v;
}

int main() {
  static const int tiles[] = {TILE_AUTO, TILE_256x128, TILE_128x256, TILE_128x128,
                              TILE_256x128_W4};
  struct Shape { int T, N, K, E; };
  static const Shape shapes[] = {{649, 1024, 512, 7}, {8192, 4096, 512, 64}, {1, 512, 512, 1},
                                 {300, 1024, 256, 1024}};
  int accepted = 0, refused = 0;
  for (const Form& f : kForms) {
    for (int epi = 0; epi < 6; ++epi) {
      const std::string fe = std::string(f.name) + " " + kEpi[epi];
      for (const Shape& sh : shapes) {
        const int K = f.din == DT_FP4 && sh.K % 256 ? 512 : sh.K;
        for (int t : tiles) {
          char what[96];
          snprintf(what, sizeof what, " %dx%dx%d E=%d tile=%d", sh.T, sh.N, K, sh.E, t);
          expect_accepted(fe + what, base_case(f, epi, sh.T, sh.N, K, sh.E, t));
          ++accepted;
        }
      }
      // an activation, wide pitches, one group with a zero stride
      Case c = base_case(f, epi, 130, 512, 512, 1, TILE_AUTO);
      c.p.ldc += 32;
      if (c.p.c_scale) c.p.c_scale_ld += 8;
      c.p.act = ACT_RELU;
      c.p.b_gstride = 0; c.p.b_scale_gstride = 0;
      expect_accepted(fe + " one group, wide pitches, relu", c);
      ++accepted;
      // empty problems launch nothing and succeed
      for (int which = 0; which < 2; ++which) {
        Case z = base_case(f, epi, 256, 1024, 512, 5, TILE_AUTO);
        (which ? z.p.N : z.p.M) = 0;
        CHECK(launch(z) == hipSuccess && g_launches.empty(), "%s: empty problem", fe.c_str());
      }
      for (const Perturbation& pt : perturbations()) {
        Case r = base_case(f, epi, 256, 1024, 512, 5, TILE_AUTO);
        if (!pt.apply(r)) continue;
        expect_refused(fe + " " + pt.name, r);
        ++refused;
      }
    }
  }
  // a grid bound past 2^31 - 1 is refused: T near 2^31 with 128 x 128 tiles and a wide N
  {
    Case c = base_case(kForms[1], 0, 0x7FFFFF00, 1 << 20, 512, 1024, TILE_128x128);
    c.p.a_scale_ld = 0;
    expect_refused("grid bound past int", c);
    ++refused;
  }
  // without the grouped fields nothing changed: the same arguments reach pt4 as they always have
  {
    Case c = base_case(kForms[0], 0, 8192, 4096, 512, 8, TILE_AUTO);
    c.p.grp_offs = nullptr; c.p.ngroups = 0; c.p.b_gstride = 0;
    CHECK(launch(c) == hipSuccess && g_launches.size() == 1 && g_launches[0].entry == "bf16_bf16" &&
              g_launches[0].tile == TILE_PT4, "the ungrouped path changed");
  }
  printf("%d accepted, %d refused, %d checks failed\n", accepted, refused, g_failed);
  if (g_failed == 0) printf("grouped dispatch ok\n");
  fflush(stdout);
  return g_failed != 0 || ferror(stdout) ? 1 : 0;
}
