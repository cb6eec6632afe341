// Host-only check of what gemm_launch (csrc/gemm/gemm_mfma.hip) decides for a gated (GLU) launch,
// GemmArgs::glu: every accepted form reaches its launch entry with glu = 1 and an offered tile,
// and one perturbation at a time is refused with hipErrorInvalidValue and no launch at all.
// gemm_mfma.hip holds no device code and calls no HIP API before an entry, so it is included here
// host-only and every entry of gemm_entry.h is a stub that records its call. Built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_glu_native_host.py. The assertions
// are in this program: it prints "glu dispatch ok" and returns 0, or names what failed.
#include <cstdint>
#include <cstdio>
#include <cstring>
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

struct Launch {
  std::string entry;
  int dt, tile;
  GemmArgs p;
};
static std::vector<Launch> g_launches;

static hipError_t record(const char* name, int dt, int tile, const GemmArgs& p) {
  g_launches.push_back({name, dt, tile, p});
  return hipSuccess;
}

#define FAST(NAME)                                                         \
  hipError_t launch_fast_##NAME(const GemmArgs& p, int tile, hipStream_t) { \
    return record(#NAME, -1, tile, p);                                     \
  }
FAST(bf16_bf16) FAST(bf16_f32) FAST(f16_f16) FAST(f16_f32) FAST(fp8_bf16) FAST(fp8_f16)
FAST(fp8_f32) FAST(f32_f32)
#undef FAST
hipError_t launch_fast_mx(const GemmArgs& p, int dout, int tile, hipStream_t) {
  return record("mx", dout, tile, p);
}
hipError_t launch_fast_mxs(const GemmArgs& p, int dout, int tile, hipStream_t) {
  return record("mxs", dout, tile, p);
}
hipError_t launch_fast_mx4(const GemmArgs& p, int dout, int tile, hipStream_t) {
  return record("mx4", dout, tile, p);
}
hipError_t launch_qout_fp8(const GemmArgs& p, int din, int tile, hipStream_t) {
  return record("qout_fp8", din, tile, p);
}
hipError_t launch_qout_fp4(const GemmArgs& p, int din, int tile, hipStream_t) {
  return record("qout_fp4", din, tile, p);
}
hipError_t launch_generic(const GemmArgs& p, int din, int dout, hipStream_t) {
  return record("generic", din * 10 + dout, -1, p);
}

}  // namespace ddlb

using namespace ddlb;

static int g_failed = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      ++g_failed;                                 \
      printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
    }                                             \
  } while (0)

// An accepted form: the operands, the output, the entry it reaches and the entry's dtype argument.
struct Form {
  const char* name;
  int din, dout;
  bool scales;
  const char* entry;
  int dt;  // what the entry gets besides the tile: dout, din or -1
};
static const Form kForms[] = {
    {"bf16_bf16", DT_BF16, DT_BF16, false, "bf16_bf16", -1},
    {"bf16_f32", DT_BF16, DT_F32, false, "bf16_f32", -1},
    {"f16_f16", DT_F16, DT_F16, false, "f16_f16", -1},
    {"f16_f32", DT_F16, DT_F32, false, "f16_f32", -1},
    {"mxs_bf16", DT_FP8, DT_BF16, true, "mxs", DT_BF16},
    {"mxs_f16", DT_FP8, DT_F16, true, "mxs", DT_F16},
    {"mxs_f32", DT_FP8, DT_F32, true, "mxs", DT_F32},
    {"mx4_bf16", DT_FP4, DT_BF16, true, "mx4", DT_BF16},
    {"mx4_f16", DT_FP4, DT_F16, true, "mx4", DT_F16},
    {"mx4_f32", DT_FP4, DT_F32, true, "mx4", DT_F32},
    {"bf16_qfp8", DT_BF16, DT_FP8, false, "qout_fp8", DT_BF16},
    {"f16_qfp8", DT_F16, DT_FP8, false, "qout_fp8", DT_F16},
    {"mxs_qfp8", DT_FP8, DT_FP8, true, "qout_fp8", DT_FP8},
    {"mx4_qfp8", DT_FP4, DT_FP8, true, "qout_fp8", DT_FP4},
    {"bf16_qfp4", DT_BF16, DT_FP4, false, "qout_fp4", DT_BF16},
    {"f16_qfp4", DT_F16, DT_FP4, false, "qout_fp4", DT_F16},
    {"mxs_qfp4", DT_FP8, DT_FP4, true, "qout_fp4", DT_FP8},
    {"mx4_qfp4", DT_FP4, DT_FP4, true, "qout_fp4", DT_FP4},
};

struct Case {
  GemmArgs p;
  int din, dout, tile, mode;
};

static bool quantised(int dout) { return dout == DT_FP8 || dout == DT_FP4; }
static int n_modulus(int dout) { return dout == DT_FP4 ? 512 : dout == DT_FP8 ? 256 : 64; }

// N = the rows of b; the output has N / 2 columns, its scales N / 64 per row
static Case base_case(const Form& f, int M, int N, int K, int tile) {
  Case c;
  c.din = f.din; c.dout = f.dout; c.tile = tile; c.mode = GEMM_MODE_AUTO;
  GemmArgs& p = c.p;
  p.a = kA; p.b = kB; p.c = kC;
  p.M = M; p.N = N; p.K = K;
  p.lda = p.ldb = K; p.ldc = N / 2;
  p.glu = 1;
  if (f.scales) {
    p.a_scale = kAS; p.b_scale = kBS;
    p.a_scale_ld = p.b_scale_ld = K / 32;
  }
  if (quantised(f.dout)) { p.c_scale = kCS; p.c_scale_ld = N / 64; }
  return c;
}

static hipError_t launch(const Case& c) {
  g_launches.clear();
  return gemm_launch(c.p, c.din, c.dout, c.tile, c.mode, nullptr);
}

static void expect_accepted(const Form& f, const char* what, const Case& c) {
  const hipError_t e = launch(c);
  CHECK(e == hipSuccess, "%s %s: returned %d", f.name, what, (int)e);
  CHECK(g_launches.size() == 1, "%s %s: %zu launches", f.name, what, g_launches.size());
  if (g_launches.size() != 1) return;
  const Launch& l = g_launches[0];
  CHECK(l.entry == f.entry, "%s %s: reached %s, not %s", f.name, what, l.entry.c_str(), f.entry);
  CHECK(l.dt == f.dt, "%s %s: dtype argument %d, not %d", f.name, what, l.dt, f.dt);
  CHECK(l.p.glu == 1, "%s %s: glu = %d at the entry", f.name, what, l.p.glu);
  CHECK(mxs_offers(l.tile), "%s %s: tile %d is not offered", f.name, what, l.tile);
  CHECK(c.tile == TILE_AUTO || l.tile == c.tile, "%s %s: tile %d became %d", f.name, what, c.tile,
        l.tile);
  // the arguments arrive as given, in elements: N the rows of b, ldc the pitch of N / 2 columns
  CHECK(l.p.M == c.p.M && l.p.N == c.p.N && l.p.K == c.p.K && l.p.lda == c.p.lda &&
            l.p.ldb == c.p.ldb && l.p.ldc == c.p.ldc && l.p.a == c.p.a && l.p.b == c.p.b &&
            l.p.c == c.p.c && l.p.a_scale == c.p.a_scale && l.p.b_scale == c.p.b_scale &&
            l.p.c_scale == c.p.c_scale && l.p.c_scale_ld == c.p.c_scale_ld &&
            l.p.act == c.p.act && l.p.ksplit == 1 && l.p.tile_order == 0,
        "%s %s: arguments changed on the way", f.name, what);
  CHECK(l.p.a_grp == c.p.M && l.p.c_grp == c.p.M, "%s %s: rows not plain", f.name, what);
}

static void expect_refused(const Form& f, const char* what, const Case& c) {
  const hipError_t e = launch(c);
  CHECK(e == hipErrorInvalidValue, "%s %s: returned %d, not hipErrorInvalidValue", f.name, what,
        (int)e);
  CHECK(g_launches.empty(), "%s %s: %zu launches (%s)", f.name, what, g_launches.size(),
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
  // N off the modulus of the output: 64 dense, 256 MX-fp8, 512 MXFP4 (ldc and the pitch follow)
  add("N-32", [](Case& c) { c.p.N -= 32; return true; });
  add("N+modulus/2", [=](Case& c) {
    c.p.N += n_modulus(c.dout) / 2; c.p.ldc = c.p.N / 2;
    if (quant(c)) c.p.c_scale_ld = (c.p.N / 64 + 7) / 8 * 8;
    return true; });
  add("N=modulus/2", [=](Case& c) {
    c.p.N = n_modulus(c.dout) / 2; c.p.ldc = 1024; return true; });
  add("ldc=N/2-1", [](Case& c) { c.p.ldc = c.p.N / 2 - 1; return true; });
  add("ldc=N/2-16", [](Case& c) { c.p.ldc = c.p.N / 2 - 16; return true; });
  add("ksplit=2", [](Case& c) { c.p.ksplit = 2; c.p.lda = c.p.ldb = 2 * c.p.K; return true; });
  add("a_grp=64", [](Case& c) { c.p.a_grp = c.p.a_gstride = 64; return true; });
  add("c_grp=64", [](Case& c) { c.p.c_grp = c.p.c_gstride = 64; return true; });
  add("flags", [](Case& c) { c.p.flags = kFlags; return true; });
  add("a_table", [](Case& c) { c.p.a_table = kTab; c.p.shard_rows = 256; return true; });
  add("c_table", [](Case& c) { c.p.c_table = kTab; c.p.c_shard_rows = 256; return true; });
  add("tile_order=1", [](Case& c) { c.p.tile_order = 1; return true; });
  add("ag_ctas=8", [](Case& c) { c.p.ag_ctas = 8; return true; });
  add("ag_mode=2", [](Case& c) { c.p.ag_mode = AG_AGENT_ACQUIRE; return true; });
  // unit-scale fp8 (one scale or none); scales on 16-bit operands
  add("unit_scales", [=](Case& c) {
    if (c.din != DT_FP8) return false; c.p.a_scale = c.p.b_scale = nullptr; return true; });
  add("unit_scales_mode=mx", [=](Case& c) {
    if (c.din != DT_FP8) return false;
    c.p.a_scale = c.p.b_scale = nullptr; c.mode = GEMM_MODE_MX; return true; });
  add("a_scale_only", [=](Case& c) { if (!scaled(c)) return false; c.p.b_scale = nullptr; return true; });
  add("scales_on_16_bit", [=](Case& c) {
    if (scaled(c)) return false;
    c.p.a_scale = kAS; c.p.b_scale = kBS; c.p.a_scale_ld = c.p.b_scale_ld = c.p.K / 32;
    return true; });
  // other operand and output types
  add("f32_operands", [=](Case& c) {
    if (scaled(c)) return false; c.din = DT_F32; if (!quant(c)) c.dout = DT_F32; return true; });
  add("f64_operands", [=](Case& c) {
    if (scaled(c)) return false; c.din = DT_F64; if (!quant(c)) c.dout = DT_F64; return true; });
  add("dense_output_unpaired", [=](Case& c) {  // bf16 -> f16, f16 -> bf16
    if (scaled(c) || quant(c) || c.dout == DT_F32) return false;
    c.dout = c.dout == DT_BF16 ? DT_F16 : DT_BF16; return true; });
  add("c_scale_toggled", [=](Case& c) {
    if (quant(c)) c.p.c_scale = nullptr; else { c.p.c_scale = kCS; c.p.c_scale_ld = c.p.N / 64; }
    return true; });
  // tiles: the ping-pong codes, the 256x256 and interleaved tiled codes, retired and unknown ones
  static const struct { const char* name; int code; } kNotOffered[] = {
      {"tile=pt4", TILE_PT4}, {"tile=t4", TILE_T4}, {"tile=pt8", TILE_PT8}, {"tile=t8", TILE_T8},
      {"tile=256x256", TILE_256x256}, {"tile=256x256w4", TILE_256x256_W4},
      {"tile=i256", TILE_I256}, {"tile=i128", TILE_I128}, {"tile=i256w4", TILE_I256W4},
      {"tile=retired5", 5}, {"tile=unknown99", 99}};
  for (const auto& t : kNotOffered) {
    const int code = t.code;
    add(t.name, [=](Case& c) { c.tile = code; return true; });
  }
  add("mode=generic", [](Case& c) { c.mode = GEMM_MODE_GENERIC; return true; });
  add("mode=3", [](Case& c) { c.mode = 3; return true; });
  add("mode=mx_on_16_bit", [=](Case& c) {
    if (scaled(c)) return false; c.mode = GEMM_MODE_MX; return true; });
  // the output scales: a short pitch, an unaligned pitch or base
  add("c_scale_ld=N/64-4", [=](Case& c) {
    if (!quant(c)) return false; c.p.c_scale_ld = c.p.N / 64 - 4; return true; });
  add("c_scale_ld=N/64-8", [=](Case& c) {
    if (!quant(c)) return false; c.p.c_scale_ld = c.p.N / 64 - 8; return true; });
  add("c_scale_ld=N/64+2", [=](Case& c) {
    if (!quant(c)) return false; c.p.c_scale_ld = c.p.N / 64 + 2; return true; });
  add("c_scale+2", [=](Case& c) { if (!quant(c)) return false; c.p.c_scale = kCS + 2; return true; });
  add("c+8_quantised", [=](Case& c) { if (!quant(c)) return false; c.p.c = kC + 8; return true; });
  add("c+4", [](Case& c) { c.p.c = kC + 4; return true; });
  add("lda<K", [](Case& c) { c.p.lda = c.p.K - 16; return true; });
  add("K=0", [](Case& c) { c.p.K = 0; return true; });
  add("M=-1", [](Case& c) { c.p.M = -1; return true; });
  add("a=null", [](Case& c) { c.p.a = nullptr; return true; });
  add("c=null", [](Case& c) { c.p.c = nullptr; return true; });
  return v;
}

// An empty problem (M == 0 or N == 0) with one malformed shape argument is refused: the rules on the
// shape come before the empty problem's hipSuccess.
struct EmptyFault {
  const char* name;
  std::function<bool(Case&)> apply;  // false: does not apply to this form
};
static const EmptyFault kEmptyFaults[] = {
    {"fp4 K % 256", [](Case& c) {
       if (c.din != DT_FP4) return false; c.p.K = c.p.lda = c.p.ldb = 384; return true; }},
    {"fp4 odd lda", [](Case& c) { if (c.din != DT_FP4) return false; c.p.lda += 1; return true; }},
    {"lda < K", [](Case& c) { c.p.lda = c.p.K - 16; return true; }},
    {"ldb < K", [](Case& c) { c.p.ldb = c.p.K - 16; return true; }},
};

int main() {
  static const int tiles[] = {TILE_AUTO, TILE_256x128, TILE_128x256, TILE_128x128,
                              TILE_256x128_W4};
  struct Shape { int M, N, K; };
  // whole 256x256 tiles (where an ungated `auto` is pt4), many of them, and a ragged M
  static const Shape shapes[] = {{256, 1024, 512}, {8192, 4096, 512}, {300, 1024, 256}, {1, 512, 512}};
  int accepted = 0, refused = 0;
  for (const Form& f : kForms) {
    for (const Shape& sh : shapes) {
      const int K = f.din == DT_FP4 && sh.K % 256 ? 512 : sh.K;
      for (int t : tiles) {
        char what[64];
        snprintf(what, sizeof what, "%dx%dx%d tile=%d", sh.M, sh.N, K, t);
        expect_accepted(f, what, base_case(f, sh.M, sh.N, K, t));
        ++accepted;
      }
    }
    // the smallest N of the form, a wider ldc and scale pitch, an activation
    Case c = base_case(f, 130, n_modulus(f.dout), 512, TILE_AUTO);
    c.p.ldc = c.p.N / 2 + 32;
    if (c.p.c_scale) c.p.c_scale_ld = c.p.N / 64 + 8;
    c.p.act = ACT_SILU;
    expect_accepted(f, "smallest N, wide pitches, silu", c);
    ++accepted;
    // empty problems launch nothing and succeed
    for (int which = 0; which < 2; ++which) {
      Case z = base_case(f, 256, 1024, 512, TILE_AUTO);
      (which ? z.p.N : z.p.M) = 0;
      CHECK(launch(z) == hipSuccess && g_launches.empty(), "%s: empty problem", f.name);
      for (const EmptyFault& ef : kEmptyFaults) {
        Case y = z;
        if (!ef.apply(y)) continue;
        const hipError_t e = launch(y);
        CHECK(e == hipErrorInvalidValue && g_launches.empty(), "%s: empty problem (%s = 0) with %s: %d",
              f.name, which ? "N" : "M", ef.name, (int)e);
      }
    }
  }
  const std::vector<Perturbation> perts = perturbations();
  for (const Form& f : kForms) {
    for (const Perturbation& pt : perts) {
      Case c = base_case(f, 256, 1024, 512, TILE_AUTO);
      if (!pt.apply(c)) continue;
      expect_refused(f, pt.name, c);
      ++refused;
    }
  }
  // glu = 0 is the old path: the same arguments reach pt4 (bf16) as they always have
  {
    Case c = base_case(kForms[0], 8192, 4096, 512, TILE_AUTO);
    c.p.glu = 0; c.p.ldc = c.p.N;
    CHECK(launch(c) == hipSuccess && g_launches.size() == 1 && g_launches[0].tile == TILE_PT4 &&
              g_launches[0].p.glu == 0, "glu = 0 changed the ungated path");
  }
  printf("%d accepted, %d refused, %d checks failed\n", accepted, refused, g_failed);
  if (g_failed == 0) printf("glu dispatch ok\n");
  fflush(stdout);
  return g_failed != 0 || ferror(stdout) ? 1 : 0;
}
