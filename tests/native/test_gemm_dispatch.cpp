// Host-only table of everything gemm_launch (csrc/gemm/gemm_mfma.hip) decides before a kernel
// runs: which launch entry it calls, with which tile and which GemmArgs, what it refuses and with
// which code, how the K-split fallback slices, when it clears tile_order or maps `auto` onto an
// offered tile. gemm_mfma.hip holds no device code and calls no HIP API before an entry, so it is
// included here host-only and every entry of gemm_entry.h is a stub that records its call.
// Built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_native_host.py, which
// compares stdout with tests/native/gemm_dispatch_expected.txt byte for byte.
//
// One line per case:  <family> <shape> <tile> <perturbation> -> <return code> {launch}*
//   launch = entry[dtype arg]/tile M N K lda ldb ldc a_grp a_gstride c_grp c_gstride ksplit
//            tile_order nsub ag_ctas a_scale_ld b_scale_ld c_scale_ld a+off b+off c+off
// (offsets in bytes from the pointers the case passed in; pointers are fake aligned constants).
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

static std::string g_log;          // the launches of the current case
static const void* g_a, *g_b, *g_c;  // the pointers the current case passed in
static bool g_pt4_refuses_ksplit;  // the pt4 entry answers hipErrorNotSupported to a K-split

static hipError_t record(const char* name, int dt, int tile, const GemmArgs& p) {
  char buf[512];
  snprintf(buf, sizeof buf,
           " {%s[%d]/%d %d %d %d %lld %lld %lld %lld %lld %lld %lld %d %d %d %d %lld %lld %lld "
           "a+%lld b+%lld c+%lld}",
           name, dt, tile, p.M, p.N, p.K, (long long)p.lda, (long long)p.ldb, (long long)p.ldc,
           (long long)p.a_grp, (long long)p.a_gstride, (long long)p.c_grp, (long long)p.c_gstride,
           p.ksplit, p.tile_order, p.nsub, p.ag_ctas, (long long)p.a_scale_ld,
           (long long)p.b_scale_ld, (long long)p.c_scale_ld,
           (long long)((const char*)p.a - (const char*)g_a),
           (long long)((const char*)p.b - (const char*)g_b),
           (long long)((const char*)p.c - (const char*)g_c));
  g_log += buf;
  if (g_pt4_refuses_ksplit && tile == TILE_PT4 && p.ksplit > 1) return hipErrorNotSupported;
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

struct Family {
  const char* name;
  int din, dout, mode;
  bool scales, c_scale;
};
static const Family kFamilies[] = {
    {"bf16_bf16", DT_BF16, DT_BF16, GEMM_MODE_AUTO, false, false},
    {"fp8_bf16", DT_FP8, DT_BF16, GEMM_MODE_AUTO, false, false},
    {"f32_f32", DT_F32, DT_F32, GEMM_MODE_AUTO, false, false},
    {"fp8mx_bf16", DT_FP8, DT_BF16, GEMM_MODE_MX, false, false},
    {"mxs_bf16", DT_FP8, DT_BF16, GEMM_MODE_AUTO, true, false},
    {"mxs_f32", DT_FP8, DT_F32, GEMM_MODE_AUTO, true, false},
    {"mx4_bf16", DT_FP4, DT_BF16, GEMM_MODE_AUTO, true, false},
    {"mx4_f32", DT_FP4, DT_F32, GEMM_MODE_AUTO, true, false},
    {"bf16_qfp8", DT_BF16, DT_FP8, GEMM_MODE_AUTO, false, true},
    {"mxs_qfp8", DT_FP8, DT_FP8, GEMM_MODE_AUTO, true, true},
    {"mx4_qfp8", DT_FP4, DT_FP8, GEMM_MODE_AUTO, true, true},
    {"bf16_qfp4", DT_BF16, DT_FP4, GEMM_MODE_AUTO, false, true},
    {"mxs_qfp4", DT_FP8, DT_FP4, GEMM_MODE_AUTO, true, true},
    {"mx4_qfp4", DT_FP4, DT_FP4, GEMM_MODE_AUTO, true, true},
    {"f64_f64", DT_F64, DT_F64, GEMM_MODE_AUTO, false, false},
    {"bf16_bf16_generic", DT_BF16, DT_BF16, GEMM_MODE_GENERIC, false, false},
    // (the families below run the shape x tile grid only)
    {"f16_qfp8", DT_F16, DT_FP8, GEMM_MODE_AUTO, false, true},
    {"f16_qfp4", DT_F16, DT_FP4, GEMM_MODE_AUTO, false, true},
    {"bf16_f32", DT_BF16, DT_F32, GEMM_MODE_AUTO, false, false},
    {"f16_f16", DT_F16, DT_F16, GEMM_MODE_AUTO, false, false},
    {"f16_f32", DT_F16, DT_F32, GEMM_MODE_AUTO, false, false},
    {"fp8_f16", DT_FP8, DT_F16, GEMM_MODE_AUTO, false, false},
    {"fp8_f32", DT_FP8, DT_F32, GEMM_MODE_AUTO, false, false},
    {"fp8mx_f32", DT_FP8, DT_F32, GEMM_MODE_MX, false, false},
    {"mxs_f16", DT_FP8, DT_F16, GEMM_MODE_AUTO, true, false},
    {"mx4_f16", DT_FP4, DT_F16, GEMM_MODE_AUTO, true, false},
    {"bf16_f16_nopair", DT_BF16, DT_F16, GEMM_MODE_AUTO, false, false},
    {"f32_bf16_nopair", DT_F32, DT_BF16, GEMM_MODE_AUTO, false, false},
};
constexpr int kPerturbedFamilies = 16;

struct Case {
  GemmArgs p;
  int din, dout, tile, mode;
  bool pt4_refuses_ksplit = false;
};

static int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

static Case base_case(const Family& f, int M, int N, int K, int tile) {
  Case c;
  c.din = f.din; c.dout = f.dout; c.tile = tile; c.mode = f.mode;
  GemmArgs& p = c.p;
  p.a = kA; p.b = kB; p.c = kC;
  p.M = M; p.N = N; p.K = K;
  p.lda = p.ldb = K; p.ldc = N;
  if (f.scales) {
    p.a_scale = kAS; p.b_scale = kBS;
    p.a_scale_ld = p.b_scale_ld = round_up(K / 32, 8);
  }
  if (f.c_scale) { p.c_scale = kCS; p.c_scale_ld = round_up(N / 32, 8); }
  return c;
}

static void run(const char* family, const char* shape, const char* tile, const char* what,
                const Case& c) {
  g_log.clear();
  g_a = c.p.a; g_b = c.p.b; g_c = c.p.c;
  g_pt4_refuses_ksplit = c.pt4_refuses_ksplit;
  const hipError_t e = gemm_launch(c.p, c.din, c.dout, c.tile, c.mode, nullptr);
  printf("%s %s %s %s -> %d%s\n", family, shape, tile, what, (int)e, g_log.c_str());
}

struct Perturbation {
  const char* name;
  std::function<bool(Case&)> apply;  // false: does not apply to this family (no line)
};

static void set_ksplit(Case& c, int n) {  // K stays the slice length; rows hold every slice
  c.p.ksplit = n;
  c.p.lda = c.p.ldb = (int64_t)c.p.K * n;
}
static void set_ag(Case& c) {  // everything the in-kernel all-gather asks for
  c.p.flags = kFlags; c.p.ag_ctas = 8; c.p.ag_tab = kTab; c.p.ag_parts = 1;
  c.p.nshards = 1; c.p.nsub = 1; c.p.flag_rows = 256;
}

static std::vector<Perturbation> perturbations() {
  std::vector<Perturbation> v;
  auto add = [&](const char* n, std::function<bool(Case&)> f) { v.push_back({n, f}); };
  auto scaled = [](const Case& c) { return c.p.a_scale != nullptr; };
  auto quant = [](const Case& c) { return c.p.c_scale != nullptr; };
  // scale operands
  add("a_scale_toggled", [=](Case& c) {
    if (scaled(c)) c.p.a_scale = nullptr; else { c.p.a_scale = kAS; c.p.a_scale_ld = 16; }
    return true; });
  add("b_scale_toggled", [=](Case& c) {
    if (scaled(c)) c.p.b_scale = nullptr; else { c.p.b_scale = kBS; c.p.b_scale_ld = 16; }
    return true; });
  add("both_scales_toggled", [=](Case& c) {
    if (scaled(c)) { c.p.a_scale = c.p.b_scale = nullptr; }
    else { c.p.a_scale = kAS; c.p.b_scale = kBS; c.p.a_scale_ld = c.p.b_scale_ld = 16; }
    return true; });
  add("a_scale+1", [=](Case& c) { if (!scaled(c)) return false; c.p.a_scale = kAS + 1; return true; });
  add("a_scale+4", [=](Case& c) { if (!scaled(c)) return false; c.p.a_scale = kAS + 4; return true; });
  add("b_scale+1", [=](Case& c) { if (!scaled(c)) return false; c.p.b_scale = kBS + 1; return true; });
  add("b_scale+4", [=](Case& c) { if (!scaled(c)) return false; c.p.b_scale = kBS + 4; return true; });
  add("a_scale_ld=8", [=](Case& c) { if (!scaled(c)) return false; c.p.a_scale_ld = 8; return true; });
  add("b_scale_ld=8", [=](Case& c) { if (!scaled(c)) return false; c.p.b_scale_ld = 8; return true; });
  add("a_scale_ld=18", [=](Case& c) { if (!scaled(c)) return false; c.p.a_scale_ld = 18; return true; });
  add("a_scale_ld=20", [=](Case& c) { if (!scaled(c)) return false; c.p.a_scale_ld = 20; return true; });
  add("b_scale_ld=20", [=](Case& c) { if (!scaled(c)) return false; c.p.b_scale_ld = 20; return true; });
  add("a_scale_ld=24", [=](Case& c) { if (!scaled(c)) return false; c.p.a_scale_ld = 24; return true; });
  add("a_scale_rows=2^31", [=](Case& c) {
    if (!scaled(c)) return false; c.p.a_scale_ld = int64_t(1) << 23; return true; });
  add("a_scale_rows=2^31-2048", [=](Case& c) {
    if (!scaled(c)) return false; c.p.a_scale_ld = (int64_t(1) << 23) - 8; return true; });
  add("b_scale_rows=2^31", [=](Case& c) {
    if (!scaled(c)) return false; c.p.b_scale_ld = int64_t(1) << 23; return true; });
  // K and the operand rows
  add("K=384", [](Case& c) { c.p.K = c.p.lda = c.p.ldb = 384; return true; });
  add("K=100", [](Case& c) { c.p.K = c.p.lda = c.p.ldb = 100; return true; });
  add("K=0", [](Case& c) { c.p.K = 0; return true; });
  add("lda<K", [](Case& c) { c.p.lda = c.p.K - 16; return true; });
  add("ldb<K", [](Case& c) { c.p.ldb = c.p.K - 16; return true; });
  add("lda=K+1", [](Case& c) { c.p.lda = c.p.K + 1; return true; });
  add("ldb=K+1", [](Case& c) { c.p.ldb = c.p.K + 1; return true; });
  add("lda=K+2", [](Case& c) { c.p.lda = c.p.K + 2; return true; });
  add("lda=K+32", [](Case& c) { c.p.lda = c.p.K + 32; return true; });
  add("a+8", [](Case& c) { c.p.a = kA + 8; return true; });
  // the output
  add("c+8", [](Case& c) { c.p.c = kC + 8; return true; });
  add("c+4", [](Case& c) { c.p.c = kC + 4; return true; });
  add("ldc<N", [](Case& c) { c.p.ldc = c.p.N - 16; return true; });
  add("ldc=N+1", [](Case& c) { c.p.ldc = c.p.N + 1; return true; });
  add("ldc=N+8", [](Case& c) { c.p.ldc = c.p.N + 8; return true; });
  add("ldc=N+32", [](Case& c) { c.p.ldc = c.p.N + 32; return true; });
  add("N=128", [](Case& c) { c.p.N = c.p.ldc = 128; return true; });
  add("N=192", [](Case& c) { c.p.N = c.p.ldc = 192; return true; });
  add("c_scale_toggled", [=](Case& c) {
    if (quant(c)) c.p.c_scale = nullptr; else { c.p.c_scale = kCS; c.p.c_scale_ld = 8; }
    return true; });
  add("c_scale+4", [=](Case& c) { if (!quant(c)) return false; c.p.c_scale = kCS + 4; return true; });
  add("c_scale+1", [=](Case& c) { if (!quant(c)) return false; c.p.c_scale = kCS + 1; return true; });
  add("c_scale_ld=4", [=](Case& c) { if (!quant(c)) return false; c.p.c_scale_ld = 4; return true; });
  add("c_scale_ld=12", [=](Case& c) { if (!quant(c)) return false; c.p.c_scale_ld = 12; return true; });
  add("c_scale_ld=10", [=](Case& c) { if (!quant(c)) return false; c.p.c_scale_ld = 10; return true; });
  add("c_scale_rows=2^31", [=](Case& c) {
    if (!quant(c)) return false; c.p.c_scale_ld = int64_t(1) << 23; return true; });
  // K-split
  add("ksplit=2", [](Case& c) { set_ksplit(c, 2); return true; });
  add("ksplit=2_128x128", [](Case& c) { set_ksplit(c, 2); c.tile = TILE_128x128; return true; });
  add("ksplit=3_pt4", [](Case& c) { set_ksplit(c, 3); c.tile = TILE_PT4; return true; });
  add("ksplit=2_pt4_refuses", [](Case& c) {
    set_ksplit(c, 2); c.pt4_refuses_ksplit = true; return true; });
  add("ksplit=2_tile_order=1", [](Case& c) { set_ksplit(c, 2); c.p.tile_order = 1; return true; });
  add("ksplit=65", [](Case& c) { set_ksplit(c, 65); return true; });
  add("ksplit=2_act", [](Case& c) { set_ksplit(c, 2); c.p.act = ACT_GELU; return true; });
  add("ksplit=2_c_grp=64", [](Case& c) {
    set_ksplit(c, 2); c.p.c_grp = c.p.c_gstride = 64; return true; });
  add("act", [](Case& c) { c.p.act = ACT_GELU; return true; });
  // grouped rows, flags, tables, the in-kernel all-gather
  add("a_grp=64", [](Case& c) { c.p.a_grp = c.p.a_gstride = 64; return true; });
  add("c_grp=64", [](Case& c) { c.p.c_grp = c.p.c_gstride = 64; return true; });
  add("flags", [](Case& c) { c.p.flags = kFlags; return true; });
  add("a_table_shard_rows=0", [](Case& c) { c.p.a_table = kTab; return true; });
  add("a_table_shard_rows=256", [](Case& c) { c.p.a_table = kTab; c.p.shard_rows = 256; return true; });
  add("a_table_shard_rows=320", [](Case& c) { c.p.a_table = kTab; c.p.shard_rows = 320; return true; });
  add("a_table_shard_rows=256_flags", [](Case& c) {
    c.p.a_table = kTab; c.p.shard_rows = 256; c.p.flags = kFlags; return true; });
  add("a_table_shard_rows=320_flags", [](Case& c) {
    c.p.a_table = kTab; c.p.shard_rows = 320; c.p.flags = kFlags; return true; });
  add("a_table_shard_rows=256_t4", [](Case& c) {
    c.p.a_table = kTab; c.p.shard_rows = 256; c.tile = TILE_T4; return true; });
  add("c_table", [](Case& c) { c.p.c_table = kTab; c.p.c_shard_rows = 256; return true; });
  add("c_table_c_shard_rows=0", [](Case& c) { c.p.c_table = kTab; return true; });
  add("c_table_flags", [](Case& c) {
    c.p.c_table = kTab; c.p.c_shard_rows = 256; c.p.flags = kFlags; return true; });
  add("ag_ctas=8", [](Case& c) { c.p.ag_ctas = 8; return true; });
  add("ag_ctas=8_complete", [](Case& c) { set_ag(c); return true; });
  add("ag_ctas=8_complete_act", [](Case& c) { set_ag(c); c.p.act = ACT_RELU; return true; });
  add("ag_mode=2", [](Case& c) { c.p.ag_mode = AG_AGENT_ACQUIRE; return true; });
  // tile order
  auto order = [](Case& c, int o, int nshards) { c.p.tile_order = o; c.p.nshards = nshards; };
  add("tile_order=1", [=](Case& c) { order(c, 1, 1); return true; });
  add("tile_order=2_nshards=2", [=](Case& c) { order(c, 2, 2); return true; });
  add("tile_order=2_nshards=3", [=](Case& c) { order(c, 2, 3); return true; });
  add("tile_order=2_nshards=0", [=](Case& c) { order(c, 2, 0); return true; });
  add("tile_order=3_nshards=2", [=](Case& c) { order(c, 3, 2); return true; });
  add("tile_order=3_nshards=3", [=](Case& c) { order(c, 3, 3); return true; });
  add("tile_order=2_nshards=2_256x128", [=](Case& c) {
    order(c, 2, 2); c.tile = TILE_256x128; return true; });
  add("tile_order=3_nshards=2_256x128", [=](Case& c) {
    order(c, 3, 2); c.tile = TILE_256x128; return true; });
  add("tile_order=2_nshards=2_N=192", [=](Case& c) {
    order(c, 2, 2); c.p.N = c.p.ldc = 192; return true; });
  add("tile_order=1_nshards=2_nsub=0", [=](Case& c) { order(c, 1, 2); c.p.nsub = 0; return true; });
  add("tile_order=1_nshards=2_nsub=4", [=](Case& c) { order(c, 1, 2); c.p.nsub = 4; return true; });
  // modes, empty problems, null operands
  add("mode=-1", [](Case& c) { c.mode = -1; return true; });
  add("mode=auto", [](Case& c) { c.mode = GEMM_MODE_AUTO; return true; });
  add("mode=generic", [](Case& c) { c.mode = GEMM_MODE_GENERIC; return true; });
  add("mode=mx", [](Case& c) { c.mode = GEMM_MODE_MX; return true; });
  add("mode=3", [](Case& c) { c.mode = 3; return true; });
  add("M=0", [](Case& c) { c.p.M = 0; return true; });
  add("N=0", [](Case& c) { c.p.N = 0; return true; });
  add("M=-1", [](Case& c) { c.p.M = -1; return true; });
  add("M=0_a_scale_toggled", [=](Case& c) {
    c.p.M = 0;
    if (scaled(c)) c.p.a_scale = nullptr; else { c.p.a_scale = kAS; c.p.a_scale_ld = 16; }
    return true; });
  add("M=0_ksplit=2", [](Case& c) { c.p.M = 0; c.p.ksplit = 2; return true; });
  add("a=null", [](Case& c) { c.p.a = nullptr; return true; });
  add("b=null", [](Case& c) { c.p.b = nullptr; return true; });
  add("c=null", [](Case& c) { c.p.c = nullptr; return true; });
  return v;
}

int main() {
  struct Shape { int M, N, K; };
  struct TileName { const char* name; int code; };
  static const TileName tiles[] = {{"auto", TILE_AUTO}, {"128x128", TILE_128x128},
                                   {"256x128", TILE_256x128}, {"256x256", TILE_256x256},
                                   {"i256", TILE_I256}, {"t8", TILE_T8}, {"pt4", TILE_PT4},
                                   {"retired5", 5}, {"unknown99", 99}};
  char shape[64];
  for (const Family& f : kFamilies) {
    // fp4 operands: K % 256, so the ragged shape keeps K = 512
    const Shape shapes[] = {{256, 256, 512}, {8192, 1024, 512},
                            {300, 202, f.din == DT_FP4 ? 512 : 256}};
    for (const Shape& sh : shapes) {
      snprintf(shape, sizeof shape, "%dx%dx%d", sh.M, sh.N, sh.K);
      for (const TileName& t : tiles)
        run(f.name, shape, t.name, "base", base_case(f, sh.M, sh.N, sh.K, t.code));
    }
  }
  const std::vector<Perturbation> perts = perturbations();
  for (int i = 0; i < kPerturbedFamilies; ++i) {
    const Family& f = kFamilies[i];
    for (const Perturbation& pt : perts) {
      Case c = base_case(f, 256, 256, 512, TILE_AUTO);
      if (pt.apply(c)) run(f.name, "256x256x512", "auto", pt.name, c);
    }
  }
  // where choose_tile answers pt4: the K-split and the orders that depend on the tile's rows
  for (const Family& f : kFamilies) {
    const std::string fam = f.name;
    if (fam != "bf16_bf16" && fam != "fp8mx_bf16" && fam != "mxs_bf16" && fam != "mx4_bf16" &&
        fam != "bf16_qfp8" && fam != "f64_f64")
      continue;
    for (const Perturbation& pt : perts) {
      const std::string n = pt.name;
      if (n.rfind("ksplit", 0) != 0 && n.rfind("tile_order", 0) != 0 && n.rfind("a_table", 0) != 0)
        continue;
      Case c = base_case(f, 8192, 1024, 512, TILE_AUTO);
      if (pt.apply(c)) run(f.name, "8192x1024x512", "auto", pt.name, c);
    }
  }
  // an empty problem with one malformed shape argument, for fp4 operands and quantised outputs
  for (const Family& f : kFamilies) {
    const bool in4 = f.din == DT_FP4;
    if (!in4 && !f.c_scale) continue;
    for (const char* empty : {"M=0", "N=0"}) {
      for (const char* fault : {"K=384", "lda=K+1", "lda<K", "ldb<K"}) {
        const std::string what = std::string(empty) + "_" + fault;
        if (!in4 && (what.find("K=384") != std::string::npos || what.find("K+1") != std::string::npos))
          continue;  // rules of fp4 operands: K % 256, even leading dimensions
        Case c = base_case(f, 256, 256, 512, TILE_AUTO);
        (empty[0] == 'M' ? c.p.M : c.p.N) = 0;
        for (const Perturbation& pt : perts)
          if (fault == std::string(pt.name)) pt.apply(c);
        run(f.name, "256x256x512", "auto", what.c_str(), c);
      }
    }
  }
  fflush(stdout);
  return ferror(stdout) ? 1 : 0;
}
