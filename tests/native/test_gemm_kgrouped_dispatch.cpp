// Host-only check of what gemm_launch (csrc/gemm/gemm_mfma.hip) decides for a K-grouped launch,
// GemmArgs::kgrouped: every accepted form (block-scaled fp8 / fp4 operands x f32 / bf16 / f16
// output x offered tile) reaches launch_kgrouped with its arguments intact, an offered tile and
// a grid E * tiles_m * tiles_n that is a grid, and one perturbation at a time is refused with
// hipErrorInvalidValue and no launch at all. gemm_mfma.hip holds no device code and calls no HIP
// API before an entry, so it is included here host-only and every entry of gemm_entry.h it calls
// is a stub that records its call. Built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_gemm_kgrouped_native_host.py. The assertions are in this program: it prints
// "kgrouped dispatch ok" and returns 0, or names what failed.
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
hipError_t launch_kgrouped(const GemmArgs& p, int din, int dout, int tile, hipStream_t) {
  return record("kgrouped", din, dout, tile, p);
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

struct Form {
  const char* name;
  int din, dout;
};
static const Form kForms[] = {
    {"mxs_bf16", DT_FP8, DT_BF16}, {"mxs_f16", DT_FP8, DT_F16}, {"mxs_f32", DT_FP8, DT_F32},
    {"mx4_bf16", DT_FP4, DT_BF16}, {"mx4_f16", DT_FP4, DT_F16}, {"mx4_f32", DT_FP4, DT_F32},
};

struct Case {
  GemmArgs p;
  int din, dout, tile, mode;
};

// M x N outputs for E groups over T rows; the operands have exactly the capacity plus `spare`
// columns (a multiple of MOD)
static Case base_case(const Form& f, int M, int N, int T, int E, int tile, int spare = 0) {
  Case c;
  c.din = f.din; c.dout = f.dout; c.tile = tile; c.mode = GEMM_MODE_AUTO;
  const int MOD = f.din == DT_FP4 ? 256 : 128;
  GemmArgs& p = c.p;
  p.a = kA; p.b = kB; p.c = kC;
  p.M = M; p.N = N; p.K = (int)kgrouped_capacity(T, E, MOD) + spare * MOD;
  p.lda = p.ldb = p.K; p.ldc = N;
  p.grp_offs = kOffs; p.ngroups = E;
  p.kgrouped = 1; p.kgrp_rows = T;
  p.c_kgstride = (int64_t)M * N + 64;  // a sentinel gap between the groups' outputs
  p.a_scale = kAS; p.b_scale = kBS;
  p.a_scale_ld = p.b_scale_ld = p.K / 32;
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
  CHECK(l.entry == "kgrouped", "%s: reached %s", w, l.entry.c_str());
  CHECK(l.din == c.din && l.dout == c.dout, "%s: dtypes %d -> %d", w, l.din, l.dout);
  CHECK(mxs_offers(l.tile), "%s: tile %d is not offered", w, l.tile);
  CHECK(c.tile == TILE_AUTO || l.tile == c.tile, "%s: tile %d became %d", w, c.tile, l.tile);
  CHECK(l.p.M == c.p.M && l.p.N == c.p.N && l.p.K == c.p.K && l.p.lda == c.p.lda &&
            l.p.ldb == c.p.ldb && l.p.ldc == c.p.ldc && l.p.a == c.p.a && l.p.b == c.p.b &&
            l.p.c == c.p.c && l.p.a_scale == c.p.a_scale && l.p.b_scale == c.p.b_scale &&
            l.p.a_scale_ld == c.p.a_scale_ld && l.p.b_scale_ld == c.p.b_scale_ld &&
            l.p.c_scale == nullptr && l.p.act == ACT_NONE && l.p.glu == 0 &&
            l.p.grp_offs == c.p.grp_offs && l.p.ngroups == c.p.ngroups && l.p.kgrouped == 1 &&
            l.p.kgrp_rows == c.p.kgrp_rows && l.p.c_kgstride == c.p.c_kgstride &&
            l.p.ksplit == 1 && l.p.tile_order == 0,
        "%s: arguments changed on the way", w);
  CHECK(l.p.a_grp == c.p.M && l.p.c_grp == c.p.M, "%s: rows not plain", w);
  const int bm = tile_rows_of(l.tile), bn = tile_cols_of(l.tile);
  const int64_t grid = (int64_t)((c.p.M + bm - 1) / bm) * ((c.p.N + bn - 1) / bn) * c.p.ngroups;
  CHECK(grid > 0 && grid <= 0x7FFFFFFFLL, "%s: grid %lld", w, (long long)grid);
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
  // what the M-grouped form refuses about flags, tables, grouped rows, K-split, all-gather
  add("flags", [](Case& c) { c.p.flags = kFlags; return true; });
  add("a_table", [](Case& c) { c.p.a_table = kTab; c.p.shard_rows = 256; return true; });
  add("c_table", [](Case& c) { c.p.c_table = kTab; c.p.c_shard_rows = 256; return true; });
  add("a_grp=64", [](Case& c) { c.p.a_grp = c.p.a_gstride = 64; return true; });
  add("c_grp=64", [](Case& c) { c.p.c_grp = c.p.c_gstride = 64; return true; });
  add("ksplit=2", [](Case& c) { c.p.ksplit = 2; return true; });
  add("tile_order=1", [](Case& c) { c.p.tile_order = 1; return true; });
  add("ag_ctas=8", [](Case& c) { c.p.ag_ctas = 8; return true; });
  add("ag_mode=2", [](Case& c) { c.p.ag_mode = AG_AGENT_ACQUIRE; return true; });
  add("mode=generic", [](Case& c) { c.mode = GEMM_MODE_GENERIC; return true; });
  add("mode=7", [](Case& c) { c.mode = 7; return true; });
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
  add("b_gstride=64", [](Case& c) { c.p.b_gstride = 64; return true; });
  add("b_scale_gstride=8", [](Case& c) { c.p.b_scale_gstride = 8; return true; });
  // an activation, a gate, a quantised output
  add("act=relu", [](Case& c) { c.p.act = ACT_RELU; return true; });
  add("glu", [](Case& c) { c.p.glu = 1; return true; });
  add("c_scale", [](Case& c) { c.p.c_scale = kCS; c.p.c_scale_ld = c.p.N / 32; return true; });
  add("dout=fp8", [](Case& c) { c.dout = DT_FP8; return true; });
  add("dout=fp8+c_scale", [](Case& c) {
    c.dout = DT_FP8; c.p.c_scale = kCS; c.p.c_scale_ld = c.p.N / 32; return true; });
  add("dout=fp4+c_scale", [](Case& c) {
    c.dout = DT_FP4; c.p.c_scale = kCS; c.p.c_scale_ld = c.p.N / 32; return true; });
  add("dout=f64", [](Case& c) { c.dout = DT_F64; return true; });
  // unscaled operands, other operands
  add("unit_scales", [](Case& c) { c.p.a_scale = c.p.b_scale = nullptr; return true; });
  add("a_scale_only", [](Case& c) { c.p.b_scale = nullptr; return true; });
  add("b_scale_only", [](Case& c) { c.p.a_scale = nullptr; return true; });
  add("bf16_operands", [](Case& c) { c.din = DT_BF16; c.dout = DT_BF16; return true; });
  add("f16_operands_with_scales", [](Case& c) { c.din = DT_F16; c.dout = DT_F16; return true; });
  add("f32_operands", [](Case& c) { c.din = DT_F32; c.dout = DT_F32; return true; });
  // the column extent against the capacity
  add("K=capacity-MOD", [](Case& c) {
    c.p.K -= c.din == DT_FP4 ? 256 : 128; return true; });
  add("K+32", [](Case& c) { c.p.K += 32; c.p.lda += 32; c.p.ldb += 32; return true; });
  add("K=0", [](Case& c) { c.p.K = 0; return true; });
  add("rows+MOD", [](Case& c) { c.p.kgrp_rows += c.din == DT_FP4 ? 256 : 128; return true; });
  add("rows=-1", [](Case& c) { c.p.kgrp_rows = -1; return true; });
  add("ngroups+1", [](Case& c) { c.p.ngroups += 1; return true; });
  add("lda<K", [](Case& c) { c.p.lda = c.p.K - 16; return true; });
  add("ldb<K", [](Case& c) { c.p.ldb = c.p.K - 16; return true; });
  add("lda_odd_fp4", [](Case& c) { if (c.din != DT_FP4) return false; c.p.lda += 1; return true; });
  add("a_scale_ld_short", [](Case& c) { c.p.a_scale_ld -= 8; return true; });
  add("a_scale_ld+2", [](Case& c) { c.p.a_scale_ld += 2; return true; });
  add("b_scale_ld+4_fp4", [](Case& c) {
    if (c.din != DT_FP4) return false; c.p.b_scale_ld += 4; return true; });
  add("a_scale+4_fp4", [](Case& c) {
    if (c.din != DT_FP4) return false; c.p.a_scale += 4; return true; });
  add("a+8", [](Case& c) { c.p.a = kA + 8; return true; });
  // the groups' outputs
  add("c_kgstride<M*ldc", [](Case& c) { c.p.c_kgstride = (int64_t)c.p.M * c.p.ldc - 64; return true; });
  add("c_kgstride=0", [](Case& c) { c.p.c_kgstride = 0; return true; });
  add("c_kgstride=-8", [](Case& c) { c.p.c_kgstride = -8; return true; });
  add("c_kgstride_off_8_bytes", [](Case& c) {
    c.p.c_kgstride += c.dout == DT_F32 ? 1 : 2; return true; });
  add("ldc_short", [](Case& c) { c.p.ldc -= 16; return true; });
  add("M=-1", [](Case& c) { c.p.M = -1; return true; });
  add("N=-1", [](Case& c) { c.p.N = -1; return true; });
  add("a=null", [](Case& c) { c.p.a = nullptr; return true; });
  add("b=null", [](Case& c) { c.p.b = nullptr; return true; });
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
    {"fp4 K % 256", [](Case& c) {  // still at least the capacity
       if (c.din != DT_FP4) return false; c.p.K += 128; c.p.lda = c.p.ldb = c.p.K; return true; }},
    {"fp4 odd lda", [](Case& c) { if (c.din != DT_FP4) return false; c.p.lda += 1; return true; }},
    {"lda < K", [](Case& c) { c.p.lda = c.p.K - 16; return true; }},
    {"ldb < K", [](Case& c) { c.p.ldb = c.p.K - 16; return true; }},
};

int main() {
  static const int tiles[] = {TILE_AUTO, TILE_256x128, TILE_128x256, TILE_128x128,
                              TILE_256x128_W4};
  struct Shape { int M, N, T, E; };
  static const Shape shapes[] = {{192, 320, 644, 7}, {4096, 1024, 8192, 64}, {8, 8, 1, 1},
                                 {512, 512, 300, 1024}, {128, 256, 0, 3}};
  int accepted = 0, refused = 0;
  for (const Form& f : kForms) {
    for (const Shape& sh : shapes) {
      for (int t : tiles) {
        char what[96];
        snprintf(what, sizeof what, " %dx%d T=%d E=%d tile=%d", sh.M, sh.N, sh.T, sh.E, t);
        expect_accepted(f.name + std::string(what), base_case(f, sh.M, sh.N, sh.T, sh.E, t));
        ++accepted;
      }
    }
    // spare columns, wide pitches, one group with a zero output stride
    Case c = base_case(f, 130, 72, 500, 1, TILE_AUTO, 2);
    c.p.lda += 256; c.p.ldb += 512; c.p.ldc += 32;
    c.p.a_scale_ld += 8; c.p.b_scale_ld += 16;
    c.p.c_kgstride = 0;
    expect_accepted(std::string(f.name) + " one group, wide pitches", c);
    ++accepted;
    c.mode = GEMM_MODE_MX;
    expect_accepted(std::string(f.name) + " mode mx", c);
    ++accepted;
    // empty problems launch nothing and succeed
    for (int which = 0; which < 2; ++which) {
      Case z = base_case(f, 256, 1024, 600, 5, TILE_AUTO);
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
    for (const Perturbation& pt : perturbations()) {
      Case r = base_case(f, 256, 1024, 600, 5, TILE_AUTO);
      if (!pt.apply(r)) continue;
      expect_refused(std::string(f.name) + " " + pt.name, r);
      ++refused;
    }
  }
  // a grid past 2^31 - 1 is refused: 2^11 x 2^11 tiles of 128 x 128 in 1024 groups (everything
  // else about the launch is in order: the same launch with 2^7 x 2^7 tiles is accepted)
  {
    Case c = base_case(kForms[2], 1 << 18, 1 << 18, 0, 1024, TILE_128x128);
    expect_refused("grid past int", c);
    ++refused;
    Case d = base_case(kForms[2], 1 << 14, 1 << 14, 0, 1024, TILE_128x128);
    expect_accepted("2^24 workgroups", d);
    ++accepted;
  }
  // without the switch nothing changed: the M-grouped and ungrouped paths take what they took
  {
    Case c = base_case(kForms[0], 256, 1024, 600, 5, TILE_AUTO);
    c.p.kgrouped = 0; c.p.kgrp_rows = 0; c.p.c_kgstride = 0;
    c.p.b_gstride = (int64_t)c.p.N * c.p.K; c.p.b_scale_gstride = (int64_t)c.p.N * (c.p.K / 32);
    CHECK(launch(c) == hipSuccess && g_launches.size() == 1 && g_launches[0].entry == "grouped",
          "the M-grouped path changed");
    c.p.grp_offs = nullptr; c.p.ngroups = 0; c.p.b_gstride = c.p.b_scale_gstride = 0;
    CHECK(launch(c) == hipSuccess && g_launches.size() == 1 && g_launches[0].entry == "mxs",
          "the ungrouped path changed");
  }
  printf("%d accepted, %d refused, %d checks failed\n", accepted, refused, g_failed);
  if (g_failed == 0) printf("kgrouped dispatch ok\n");
  fflush(stdout);
  return g_failed != 0 || ferror(stdout) ? 1 : 0;
}
