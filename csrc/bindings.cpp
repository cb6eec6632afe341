// Python bindings of the native runtime (module ddlb_amd._C).
//
// Tensors cross the boundary as raw device pointers + the caller's HIP stream handle
// (torch.cuda.current_stream().cuda_stream): no dependency on torch's C++ ABI, and every call is a
// single C++ entry. Python-side wrappers (ddlb_amd/ops, ddlb_amd/parallel) validate shapes, dtypes,
// devices and alignment BEFORE anything is launched. Symmetric buffers are exported to torch via
// DLPack (kDLROCM) so they can be used as ordinary tensors.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <ATen/dlpack.h>

#include <memory>
#include <tuple>

#include "comm/comm.h"
#include "gemm/gemm.h"
#include "gemm/glu_act.h"
#include "moe/moe.h"
#include "moe/moe_route_map.h"
#include "runtime/kernels.h"
#include "runtime/plan.h"

namespace py = pybind11;
using namespace ddlb;

namespace {

void check(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    (void)hipGetLastError();  // keep torch's next error check clean
    throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
  }
}

struct DLCtx {
  std::shared_ptr<void> owner;  // keeps the allocation (symmetric buffer / RCCL memory) alive
  int64_t shape[1];
};

void dl_deleter(DLManagedTensor* t) {
  delete static_cast<DLCtx*>(t->manager_ctx);
  delete t;
}

void capsule_destructor(PyObject* cap) {
  if (PyCapsule_IsValid(cap, "dltensor")) {  // never consumed
    auto* t = static_cast<DLManagedTensor*>(PyCapsule_GetPointer(cap, "dltensor"));
    if (t && t->deleter) t->deleter(t);
  }
}

py::object raw_dlpack(std::shared_ptr<void> owner, uintptr_t ptr, size_t bytes, int device) {
  auto* ctx = new DLCtx{std::move(owner), {(int64_t)bytes}};
  auto* t = new DLManagedTensor();
  t->dl_tensor.data = (void*)ptr;
  t->dl_tensor.device = DLDevice{kDLROCM, device};
  t->dl_tensor.ndim = 1;
  t->dl_tensor.dtype = DLDataType{kDLUInt, 8, 1};
  t->dl_tensor.shape = ctx->shape;
  t->dl_tensor.strides = nullptr;
  t->dl_tensor.byte_offset = 0;
  t->manager_ctx = ctx;
  t->deleter = dl_deleter;
  return py::reinterpret_steal<py::object>(PyCapsule_New(t, "dltensor", capsule_destructor));
}

py::object buffer_dlpack(std::shared_ptr<SymmetricBuffer> buf, int device) {
  return raw_dlpack(buf, buf->local(), buf->bytes(), device);
}

// CU holder of the rccl_cap preflight phase (ddlb_amd/parallel/preflight.py): holds n CUs with
// hold_cus_kernel while a capped RCCL collective must finish beside them. The counters live in
// host-coherent pinned memory, so the host sees residency and releases the holders without any
// stream ordering (the collective is queued on another stream).
class CuHolder {
 public:
  explicit CuHolder(int device) : device_(device) {
    check(hipSetDevice(device), "hipSetDevice");
    check(hipHostMalloc((void**)&host_, 512, hipHostMallocCoherent | hipHostMallocMapped),
          "hipHostMalloc");
    check(hipHostGetDevicePointer((void**)&dev_, host_, 0), "hipHostGetDevicePointer");
    reset();
  }
  ~CuHolder() {
    if (host_) {
      release();
      hipSetDevice(device_);
      hipDeviceSynchronize();
      hipHostFree(host_);
    }
  }
  void start(int nwg, uintptr_t stream, double max_s) {
    reset();
    HoldArgs a;
    a.arrived = dev_;
    a.go = dev_ + 32;
    a.timeout_word = dev_ + 64;
    a.max_ticks = (uint64_t)(max_s * 1e8);  // s_memrealtime: 100 MHz
    check(hipSetDevice(device_), "hipSetDevice");
    check(hold_cus_launch(a, nwg, (hipStream_t)stream), "hold_cus_launch");
  }
  unsigned arrived() const { return __atomic_load_n(host_, __ATOMIC_ACQUIRE); }
  unsigned timeout_bits() const { return __atomic_load_n(host_ + 64, __ATOMIC_ACQUIRE); }
  void release() { __atomic_store_n(host_ + 32, 1u, __ATOMIC_RELEASE); }

 private:
  void reset() {
    __atomic_store_n(host_, 0u, __ATOMIC_RELEASE);
    __atomic_store_n(host_ + 32, 0u, __ATOMIC_RELEASE);
    __atomic_store_n(host_ + 64, 0u, __ATOMIC_RELEASE);
  }
  int device_;
  unsigned* host_ = nullptr;  // [0] arrived, [32] go, [64] timeout bits (separate 128-B lines)
  unsigned* dev_ = nullptr;
};

GemmArgs make_args(uintptr_t a, uintptr_t b, uintptr_t c, int64_t lda, int64_t ldb, int64_t ldc,
                   int M, int N, int K, int64_t a_grp, int64_t a_gstride, int64_t c_grp,
                   int64_t c_gstride) {
  GemmArgs g;
  g.a = (const void*)a; g.b = (const void*)b; g.c = (void*)c;
  g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.M = M; g.N = N; g.K = K;
  g.a_grp = a_grp; g.a_gstride = a_gstride; g.c_grp = c_grp; g.c_gstride = c_gstride;
  return g;
}

// The block scales of the operands and the epilogue of the three GEMM bindings (an absent scale
// pointer is 0).
void set_scales_epilogue(GemmArgs& g, uintptr_t a_scale, uintptr_t b_scale, int64_t a_scale_ld,
                         int64_t b_scale_ld, uintptr_t c_scale = 0, int64_t c_scale_ld = 0,
                         int act = ACT_NONE, int glu = 0) {
  g.a_scale = (const uint8_t*)a_scale; g.b_scale = (const uint8_t*)b_scale;
  g.a_scale_ld = a_scale_ld; g.b_scale_ld = b_scale_ld;
  g.c_scale = (uint8_t*)c_scale; g.c_scale_ld = c_scale_ld;
  g.act = act; g.glu = glu != 0;
}

// The two row-wise MX quantiser bindings: one signature, one argument block, two launchers.
void def_row_quantizer(py::module_& m, const char* name,
                       hipError_t (*launch)(const MxQuantArgs&, int, hipStream_t)) {
  m.def(name,
        [name, launch](uintptr_t x, uintptr_t q, uintptr_t sc, int64_t ldx, int64_t ldq,
                       int64_t lds, int R, int K, int din, uintptr_t stream) {
          MxQuantArgs a;
          a.x = (const void*)x; a.q = (void*)q; a.s = (uint8_t*)sc;
          a.ldx = ldx; a.ldq = ldq; a.lds = lds;
          a.R = R; a.K = K;
          check(launch(a, din, (hipStream_t)stream), name);
        },
        py::arg("x"), py::arg("q"), py::arg("s"), py::arg("ldx"), py::arg("ldq"),
        py::arg("lds"), py::arg("R"), py::arg("K"), py::arg("din"), py::arg("stream") = 0);
}

// Tile codes a flavour of the tiled kernel is built for (gemm.h mxs_offers / mx4_offers).
std::vector<int> offered_tiles(bool (*offers)(int)) {
  std::vector<int> v;
  for (int i = 0; i < kNumTileCfgs; ++i)
    if (offers(kTileCfgs[i].code)) v.push_back(kTileCfgs[i].code);
  return v;
}

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "ddlb_amd native runtime: CDNA4 MFMA GEMM, RCCL/IPC data plane, plan executor";
  m.attr("OP_WORDS") = kOpWords;
  m.attr("MAX_REDUCE_SRC") = kMaxReduceSrc;
  m.attr("MAX_COPY_SEG") = kMaxCopySeg;
  m.attr("MAX_SIGNAL") = kMaxSignal;

  m.def("gemm",
        [](uintptr_t a, uintptr_t b, uintptr_t c, int64_t lda, int64_t ldb, int64_t ldc, int M,
           int N, int K, int din, int dout, int tile, int mode, int64_t a_grp, int64_t a_gstride,
           int64_t c_grp, int64_t c_gstride, uintptr_t stream, int act, int ksplit,
           uintptr_t a_scale, uintptr_t b_scale, int64_t a_scale_ld, int64_t b_scale_ld,
           uintptr_t c_scale, int64_t c_scale_ld, int glu) {
          GemmArgs g = make_args(a, b, c, lda, ldb, ldc, M, N, K, a_grp, a_gstride, c_grp,
                                 c_gstride);
          g.ksplit = ksplit > 1 ? ksplit : 1;
          set_scales_epilogue(g, a_scale, b_scale, a_scale_ld, b_scale_ld, c_scale, c_scale_ld,
                              act, glu);
          check(gemm_launch(g, din, dout, tile, mode, (hipStream_t)stream), "gemm_launch");
        },
        py::arg("a"), py::arg("b"), py::arg("c"), py::arg("lda"), py::arg("ldb"), py::arg("ldc"),
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("din"), py::arg("dout"),
        py::arg("tile") = 0, py::arg("mode") = 0, py::arg("a_grp") = 0, py::arg("a_gstride") = 0,
        py::arg("c_grp") = 0, py::arg("c_gstride") = 0, py::arg("stream") = 0,
        py::arg("act") = 0, py::arg("ksplit") = 1, py::arg("a_scale") = 0,
        py::arg("b_scale") = 0, py::arg("a_scale_ld") = 0, py::arg("b_scale_ld") = 0,
        py::arg("c_scale") = 0, py::arg("c_scale_ld") = 0, py::arg("glu") = 0);
  // Grouped GEMM (GemmArgs::grp_offs): group g = rows [offs[g], offs[g + 1]) of a / c (M rows in
  // all) times the weight at b + g * b_gstride elements; offs is device memory, never read here.
  m.def("gemm_grouped",
        [](uintptr_t a, uintptr_t b, uintptr_t c, uintptr_t offs, int ngroups, int64_t lda,
           int64_t ldb, int64_t ldc, int64_t b_gstride, int M, int N, int K, int din, int dout,
           int tile, uintptr_t stream, int act, uintptr_t a_scale, uintptr_t b_scale,
           int64_t a_scale_ld, int64_t b_scale_ld, int64_t b_scale_gstride, uintptr_t c_scale,
           int64_t c_scale_ld, int glu) {
          GemmArgs g = make_args(a, b, c, lda, ldb, ldc, M, N, K, 0, 0, 0, 0);
          g.grp_offs = (const int*)offs;
          g.ngroups = ngroups;
          g.b_gstride = b_gstride;
          g.b_scale_gstride = b_scale_gstride;
          set_scales_epilogue(g, a_scale, b_scale, a_scale_ld, b_scale_ld, c_scale, c_scale_ld,
                              act, glu);
          // a null offsets pointer or ngroups = 0 must be refused, not run ungrouped
          if (offs == 0 || ngroups <= 0) check(hipErrorInvalidValue, "gemm_grouped");
          check(gemm_launch(g, din, dout, tile, GEMM_MODE_AUTO, (hipStream_t)stream),
                "gemm_grouped");
        },
        py::arg("a"), py::arg("b"), py::arg("c"), py::arg("offs"), py::arg("ngroups"),
        py::arg("lda"), py::arg("ldb"), py::arg("ldc"), py::arg("b_gstride"), py::arg("M"),
        py::arg("N"), py::arg("K"), py::arg("din"), py::arg("dout"), py::arg("tile") = 0,
        py::arg("stream") = 0, py::arg("act") = 0, py::arg("a_scale") = 0,
        py::arg("b_scale") = 0, py::arg("a_scale_ld") = 0, py::arg("b_scale_ld") = 0,
        py::arg("b_scale_gstride") = 0, py::arg("c_scale") = 0, py::arg("c_scale_ld") = 0,
        py::arg("glu") = 0);
  // K-grouped GEMM (GemmArgs::kgrouped): c[g] = a[:, cols g] b[:, cols g]^T under the scales of
  // the same columns, the groups' column ranges derived from offs (clamped to rows) on the device;
  // K is the operands' column extent, c_gstride the elements between the groups' outputs.
  m.def("gemm_kgrouped",
        [](uintptr_t a, uintptr_t b, uintptr_t c, uintptr_t offs, int ngroups, int rows,
           int64_t lda, int64_t ldb, int64_t ldc, int64_t c_gstride, int M, int N, int K, int din,
           int dout, int tile, uintptr_t stream, uintptr_t a_scale, uintptr_t b_scale,
           int64_t a_scale_ld, int64_t b_scale_ld) {
          GemmArgs g = make_args(a, b, c, lda, ldb, ldc, M, N, K, 0, 0, 0, 0);
          g.grp_offs = (const int*)offs;
          g.ngroups = ngroups;
          g.kgrouped = 1;
          g.kgrp_rows = rows;
          g.c_kgstride = c_gstride;
          set_scales_epilogue(g, a_scale, b_scale, a_scale_ld, b_scale_ld);
          check(gemm_launch(g, din, dout, tile, GEMM_MODE_AUTO, (hipStream_t)stream),
                "gemm_kgrouped");
        },
        py::arg("a"), py::arg("b"), py::arg("c"), py::arg("offs"), py::arg("ngroups"),
        py::arg("rows"), py::arg("lda"), py::arg("ldb"), py::arg("ldc"), py::arg("c_gstride"),
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("din"), py::arg("dout"),
        py::arg("tile") = 0, py::arg("stream") = 0, py::arg("a_scale") = 0,
        py::arg("b_scale") = 0, py::arg("a_scale_ld") = 0, py::arg("b_scale_ld") = 0);
  m.def("mx_quantize_t_grouped",  // x[T, C], rows grouped by offs -> qt / st in the padded K
        // layout of gemm_kgrouped, or (stacked_rows > 0) one [C, R] slab per group
        [](uintptr_t x, uintptr_t qt, uintptr_t st, uintptr_t offs, int ngroups, int64_t ldx,
           int64_t ldqt, int64_t ldst, int T, int C, int din, bool fp4, int stacked_rows,
           int64_t qt_gstride, int64_t st_gstride, uintptr_t stream) {
          MxQuantTGroupedArgs a;
          a.x = (const void*)x; a.qt = (void*)qt; a.st = (uint8_t*)st;
          a.offs = (const int*)offs;
          a.ngroups = ngroups;
          a.ldx = ldx; a.ldqt = ldqt; a.ldst = ldst;
          a.T = T; a.C = C;
          a.stacked_rows = stacked_rows;
          a.qt_gstride = qt_gstride; a.st_gstride = st_gstride;
          check(mx_quantize_t_grouped_launch(a, din, fp4, (hipStream_t)stream),
                "mx_quantize_t_grouped");
        },
        py::arg("x"), py::arg("qt"), py::arg("st"), py::arg("offs"), py::arg("ngroups"),
        py::arg("ldx"), py::arg("ldqt"), py::arg("ldst"), py::arg("T"), py::arg("C"),
        py::arg("din"), py::arg("fp4") = false, py::arg("stacked_rows") = 0,
        py::arg("qt_gstride") = 0, py::arg("st_gstride") = 0, py::arg("stream") = 0);
  // x[R, K] f32 / f16 / bf16 -> q[R, K] e4m3 + s[R, K / 32] E8M0 bytes; mxfp4_quantize: the same
  // -> q[R, K / 2] E2M1 nibble pairs (ldq in bytes) + s
  def_row_quantizer(m, "mx_quantize", mx_quantize_launch);
  def_row_quantizer(m, "mxfp4_quantize", mxfp4_quantize_launch);
  m.def("mx_quantize_gather",  // q / s row r = the row quantiser's output for x[src[r]]; an index
        // outside [0, X) gives a zero row. src is device memory, never read here.
        [](uintptr_t x, uintptr_t src, uintptr_t q, uintptr_t sc, int64_t ldx, int64_t ldq,
           int64_t lds, int R, int K, int X, int din, bool fp4, uintptr_t stream) {
          MxQuantGatherArgs a;
          a.x = (const void*)x; a.q = (void*)q; a.s = (uint8_t*)sc;
          a.src = (const int*)src;
          a.ldx = ldx; a.ldq = ldq; a.lds = lds;
          a.R = R; a.K = K; a.X = X;
          check(mx_quantize_gather_launch(a, din, fp4, (hipStream_t)stream),
                "mx_quantize_gather");
        },
        py::arg("x"), py::arg("src"), py::arg("q"), py::arg("s"), py::arg("ldx"), py::arg("ldq"),
        py::arg("lds"), py::arg("R"), py::arg("K"), py::arg("X"), py::arg("din"),
        py::arg("fp4") = false, py::arg("stream") = 0);
  // MoE dispatch (csrc/moe): the routing sort and the weighted un-permute. Every array is device
  // memory that only the kernels read or write.
  m.attr("ROUTE_CHUNK") = kRouteChunk;
  m.def("moe_route",
        [](uintptr_t ids, uintptr_t offsets, uintptr_t row_token, uintptr_t slot_row,
           uintptr_t ws, int64_t n, int k, int E, bool ids64, uintptr_t stream) {
          MoeRouteArgs a;
          a.ids = (const void*)ids;
          a.offsets = (int*)offsets; a.row_token = (int*)row_token; a.slot_row = (int*)slot_row;
          a.ws = (int*)ws;
          a.n = n; a.k = k; a.E = E;
          a.ids64 = ids64 ? 1 : 0;
          check(moe_route_launch(a, (hipStream_t)stream), "moe_route");
        },
        py::arg("ids"), py::arg("offsets"), py::arg("row_token"), py::arg("slot_row"),
        py::arg("ws"), py::arg("n"), py::arg("k"), py::arg("E"), py::arg("ids64"),
        py::arg("stream") = 0);
  m.def("moe_combine",
        [](uintptr_t y, uintptr_t slot_row, uintptr_t gate, uintptr_t out, int64_t ldy,
           int64_t ldo, int S, int k, int T, int H, int din, int dout, uintptr_t stream) {
          MoeCombineArgs a;
          a.y = (const void*)y; a.slot_row = (const int*)slot_row;
          a.gate = (const float*)gate; a.out = (void*)out;
          a.ldy = ldy; a.ldo = ldo;
          a.S = S; a.k = k; a.T = T; a.H = H;
          check(moe_combine_launch(a, din, dout, (hipStream_t)stream), "moe_combine");
        },
        py::arg("y"), py::arg("slot_row"), py::arg("gate"), py::arg("out"), py::arg("ldy"),
        py::arg("ldo"), py::arg("S"), py::arg("k"), py::arg("T"), py::arg("H"), py::arg("din"),
        py::arg("dout"), py::arg("stream") = 0);
  m.def("moe_gather",
        [](uintptr_t x, uintptr_t row_token, uintptr_t out, int64_t ldx, int64_t ldo, int S,
           int T, int H, int dt, uintptr_t stream) {
          MoeGatherArgs a;
          a.x = (const void*)x; a.row_token = (const int*)row_token; a.out = (void*)out;
          a.ldx = ldx; a.ldo = ldo;
          a.S = S; a.T = T; a.H = H;
          check(moe_gather_launch(a, dt, (hipStream_t)stream), "moe_gather");
        },
        py::arg("x"), py::arg("row_token"), py::arg("out"), py::arg("ldx"), py::arg("ldo"),
        py::arg("S"), py::arg("T"), py::arg("H"), py::arg("dt"), py::arg("stream") = 0);
  m.def("moe_combine_bwd",
        [](uintptr_t dout, uintptr_t slot_row, uintptr_t gate, uintptr_t row_token, uintptr_t y,
           uintptr_t dy, uintptr_t dgate, int64_t lddo, int64_t ldy, int64_t lddy, int S, int k,
           int T, int H, int din, int dout_dt, uintptr_t stream) {
          MoeCombineBwdArgs a;
          a.dout = (const void*)dout; a.slot_row = (const int*)slot_row;
          a.gate = (const float*)gate; a.row_token = (const int*)row_token;
          a.y = (const void*)y; a.dy = (void*)dy; a.dgate = (float*)dgate;
          a.lddo = lddo; a.ldy = ldy; a.lddy = lddy;
          a.S = S; a.k = k; a.T = T; a.H = H;
          check(moe_combine_bwd_launch(a, din, dout_dt, (hipStream_t)stream), "moe_combine_bwd");
        },
        py::arg("dout"), py::arg("slot_row"), py::arg("gate"), py::arg("row_token"),
        py::arg("y"), py::arg("dy"), py::arg("dgate"), py::arg("lddo"), py::arg("ldy"),
        py::arg("lddy"), py::arg("S"), py::arg("k"), py::arg("T"), py::arg("H"), py::arg("din"),
        py::arg("dout_dt"), py::arg("stream") = 0);
  m.def("glu_fwd",
        [](uintptr_t c, uintptr_t out, int64_t ldc, int64_t ldo, int T, int F, int act, int din,
           int dout, uintptr_t stream) {
          GluArgs a;
          a.c = (const void*)c; a.out = (void*)out;
          a.ldc = ldc; a.ldo = ldo;
          a.T = T; a.F = F; a.act = act;
          check(glu_fwd_launch(a, din, dout, (hipStream_t)stream), "glu_fwd");
        },
        py::arg("c"), py::arg("out"), py::arg("ldc"), py::arg("ldo"), py::arg("T"), py::arg("F"),
        py::arg("act"), py::arg("din"), py::arg("dout"), py::arg("stream") = 0);
  m.def("glu_bwd",
        [](uintptr_t dh, uintptr_t c, uintptr_t out, int64_t ldh, int64_t ldc, int64_t ldo, int T,
           int F, int act, int din, uintptr_t stream) {
          GluArgs a;
          a.dh = (const void*)dh; a.c = (const void*)c; a.out = (void*)out;
          a.ldh = ldh; a.ldc = ldc; a.ldo = ldo;
          a.T = T; a.F = F; a.act = act;
          check(glu_bwd_launch(a, din, (hipStream_t)stream), "glu_bwd");
        },
        py::arg("dh"), py::arg("c"), py::arg("out"), py::arg("ldh"), py::arg("ldc"),
        py::arg("ldo"), py::arg("T"), py::arg("F"), py::arg("act"), py::arg("din"),
        py::arg("stream") = 0);
  m.def("mx_quantize_t",  // x[R, C] -> qt[C, R] (fp4: [C, R / 2]) + st[C, R / 32], blocks down
        // the columns of x; two: also the row-wise q[R, C] (fp4: [R, C / 2]) + s[R, C / 32]
        [](uintptr_t x, uintptr_t qt, uintptr_t st, int64_t ldx, int64_t ldqt, int64_t ldst,
           int R, int C, int din, bool fp4, uintptr_t stream, bool two, uintptr_t q,
           uintptr_t sc, int64_t ldq, int64_t lds) {
          MxQuantTArgs a;
          a.x = (const void*)x; a.qt = (void*)qt; a.st = (uint8_t*)st;
          a.q = (void*)q; a.s = (uint8_t*)sc;
          a.ldx = ldx; a.ldqt = ldqt; a.ldst = ldst; a.ldq = ldq; a.lds = lds;
          a.R = R; a.C = C;
          check(mx_quantize_t_launch(a, din, fp4, two, (hipStream_t)stream), "mx_quantize_t");
        },
        py::arg("x"), py::arg("qt"), py::arg("st"), py::arg("ldx"), py::arg("ldqt"),
        py::arg("ldst"), py::arg("R"), py::arg("C"), py::arg("din"), py::arg("fp4") = false,
        py::arg("stream") = 0, py::arg("two") = false, py::arg("q") = 0, py::arg("s") = 0,
        py::arg("ldq") = 0, py::arg("lds") = 0);
  m.attr("MX4_TILES") = offered_tiles(mx4_offers);  // the block-scaled fp4 GEMM is built for
  m.attr("MXS_TILES") = offered_tiles(mxs_offers);  // the block-scaled fp8 GEMM is built for
  m.def("gemm_fast_path_ok",
        [](uintptr_t a, uintptr_t b, uintptr_t c, int64_t lda, int64_t ldb, int64_t ldc, int M,
           int N, int K, int din, int dout) {
          GemmArgs g = make_args(a, b, c, lda, ldb, ldc, M, N, K, M, M, M, M);
          return gemm_fast_path_ok(g, din, dout);
        });
  m.def("choose_tile", &choose_tile);
  m.def("tile_rows", &tile_rows);
  m.def("tile_cols", &tile_cols);

  m.def("reduce_sum",
        [](uintptr_t dst, std::vector<uintptr_t> srcs, int64_t count, int dtype, uintptr_t s,
           int src_dtype) {
          ReduceArgs a;
          a.dst = (void*)dst;
          a.count = count;
          a.nsrc = (int)srcs.size();
          if (a.nsrc < 1 || a.nsrc > kMaxReduceSrc) throw std::runtime_error("1..16 sources");
          for (int i = 0; i < a.nsrc; ++i) a.src[i] = (const void*)srcs[(size_t)i];
          check(reduce_sum_launch(a, dtype, (hipStream_t)s, src_dtype), "reduce_sum");
        },
        py::arg("dst"), py::arg("srcs"), py::arg("count"), py::arg("dtype"), py::arg("stream"),
        py::arg("src_dtype") = -1);
  m.def("copy",
        [](uintptr_t dst, uintptr_t src, int64_t bytes, int max_blocks, uintptr_t s) {
          CopyArgs a;
          a.nseg = 1;
          a.dst[0] = (void*)dst;
          a.src[0] = (const void*)src;
          a.bytes[0] = bytes;
          check(copy_launch(a, max_blocks, (hipStream_t)s), "copy");
        });
  m.def("memcpy_async",  // one copy-engine copy (diagnostics: the xGMI probe's SDMA pulls)
        [](uintptr_t dst, uintptr_t src, int64_t bytes, uintptr_t s) {
          check(hipMemcpyAsync((void*)dst, (const void*)src, (size_t)bytes,
                               hipMemcpyDeviceToDevice, (hipStream_t)s),
                "hipMemcpyAsync");
        });
  m.def("copy_multi",  // segments (dst, src, bytes) copied concurrently by one CU kernel
        [](std::vector<std::tuple<uintptr_t, uintptr_t, int64_t>> segs, int max_blocks,
           uintptr_t s) {
          CopyArgs a;
          a.nseg = (int)segs.size();
          if (a.nseg < 1 || a.nseg > kMaxCopySeg) throw std::runtime_error("1..8 segments");
          for (int i = 0; i < a.nseg; ++i) {
            a.dst[i] = (void*)std::get<0>(segs[(size_t)i]);
            a.src[i] = (const void*)std::get<1>(segs[(size_t)i]);
            a.bytes[i] = std::get<2>(segs[(size_t)i]);
          }
          check(copy_launch(a, max_blocks, (hipStream_t)s), "copy_multi");
        });
  m.def("copy_batch_api_available", &copy_batch_api_available);
  m.def("copy_batch_status", &copy_batch_status);
  m.def("copy_batch",  // copy-engine copies (dst, src, bytes) submitted as one batch
        [](std::vector<std::tuple<uintptr_t, uintptr_t, int64_t>> segs, uintptr_t s) {
          std::vector<void*> d, sr;
          std::vector<size_t> b;
          for (auto& t : segs) {
            d.push_back((void*)std::get<0>(t));
            sr.push_back((void*)std::get<1>(t));
            b.push_back((size_t)std::get<2>(t));
          }
          if (d.empty()) return;
          check(copy_batch(d.data(), sr.data(), b.data(), d.size(), (hipStream_t)s), "copy_batch");
        });
  m.def("install_crash_handler", &install_crash_handler);
  m.def("device_synchronize", []() { check(hipDeviceSynchronize(), "hipDeviceSynchronize"); });
  m.def("get_last_error", []() { return std::string(hipGetErrorString(hipGetLastError())); });

  py::class_<RcclComm, std::shared_ptr<RcclComm>>(m, "RcclComm")
      .def_static("unique_id", []() { return py::bytes(RcclComm::unique_id()); })
      // (the id arrives as std::string: converted from bytes before the GIL is released)
      .def(py::init([](const std::string& uid, int nranks, int rank, int device, int max_ctas) {
             return std::make_shared<RcclComm>(uid, nranks, rank, device, max_ctas);
           }),
           py::arg("uid"), py::arg("nranks"), py::arg("rank"), py::arg("device"),
           py::arg("max_ctas") = 0, py::call_guard<py::gil_scoped_release>())
      .def("destroy", &RcclComm::destroy)
      // collectives on the caller's stream (preflight / diagnostics: the plans go through the
      // executor); count in elements of dtype (DT_* codes)
      .def("all_gather",
           [](RcclComm& c, uintptr_t send, uintptr_t recv, size_t count, int dtype, uintptr_t s) {
             DDLB_NCCL(ncclAllGather((const void*)send, (void*)recv, count, nccl_dtype(dtype),
                                     c.get(), (hipStream_t)s));
           })
      .def("reduce_scatter",
           [](RcclComm& c, uintptr_t send, uintptr_t recv, size_t count, int dtype, uintptr_t s) {
             DDLB_NCCL(ncclReduceScatter((const void*)send, (void*)recv, count, nccl_dtype(dtype),
                                         ncclSum, c.get(), (hipStream_t)s));
           })
      .def("async_error", &RcclComm::async_error)
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("nranks", &RcclComm::nranks)
      .def_property_readonly("max_ctas", &RcclComm::max_ctas);
  py::class_<CuHolder>(m, "CuHolder")
      .def(py::init<int>(), py::arg("device"))
      .def("start", &CuHolder::start, py::arg("nwg"), py::arg("stream"),
           py::arg("max_s") = 10.0)
      .def("arrived", &CuHolder::arrived)
      .def("timeout_bits", &CuHolder::timeout_bits)
      .def("release", &CuHolder::release);

  py::class_<RcclMem, std::shared_ptr<RcclMem>>(m, "RcclMem")
      .def(py::init<std::shared_ptr<RcclComm>, size_t, int>(), py::arg("comm"), py::arg("bytes"),
           py::arg("device"))
      .def("release", &RcclMem::release)
      .def("local", &RcclMem::local)
      .def_property_readonly("registered", &RcclMem::registered)
      .def_property_readonly("bytes", &RcclMem::bytes);
  m.def("rccl_mem_dlpack", [](std::shared_ptr<RcclMem> b, int device) {
    return raw_dlpack(b, b->local(), b->bytes(), device);
  });

  py::class_<SymmetricBuffer, std::shared_ptr<SymmetricBuffer>>(m, "SymmetricBuffer")
      .def(py::init<size_t, int, bool>(), py::arg("bytes"), py::arg("device"),
           py::arg("uncached") = false)
      .def_property_readonly("uncached", &SymmetricBuffer::uncached)
      .def("ipc_handle", [](const SymmetricBuffer& b) { return py::bytes(b.ipc_handle()); })
      .def("open_peers",
           [](SymmetricBuffer& b, std::vector<py::bytes> hs, int my_rank) {
             std::vector<std::string> v;
             for (auto& h : hs) v.emplace_back(std::string(h));
             b.open_peers(v, my_rank);
           })
      .def("close_peers", &SymmetricBuffer::close_peers)
      .def("release", &SymmetricBuffer::release)
      .def("local", &SymmetricBuffer::local)
      .def("peer", &SymmetricBuffer::peer)
      .def("npeers", &SymmetricBuffer::npeers)
      .def_property_readonly("bytes", &SymmetricBuffer::bytes);
  m.def("buffer_dlpack", &buffer_dlpack);

  py::class_<PlanExecutor, std::shared_ptr<PlanExecutor>>(m, "PlanExecutor")
      .def(py::init<int, int, int, const std::vector<int>&>())
      .def("load", &PlanExecutor::load)
      .def("set_comm", [](PlanExecutor& p, std::shared_ptr<RcclComm> c) { p.set_comm(c.get()); },
           py::keep_alive<1, 2>())
      .def("run", &PlanExecutor::run)
      .def("epoch", &PlanExecutor::epoch)
      .def("nops", &PlanExecutor::nops)
      .def("stream", &PlanExecutor::stream)
      .def("timeout_word", &PlanExecutor::timeout_word)
      .def("read_timeout", &PlanExecutor::read_timeout)
      .def("enable_graph", &PlanExecutor::enable_graph)
      .def("graph_enabled", &PlanExecutor::graph_enabled)
      .def("graph_capturable", &PlanExecutor::graph_capturable)
      .def("set_timeline", &PlanExecutor::set_timeline)
      .def("timeline", &PlanExecutor::timeline)
      .def("host_times", &PlanExecutor::host_times)
      .def("set_cu_split", &PlanExecutor::set_cu_split)
      .def("cu_split", &PlanExecutor::cu_split)
      .def("stream_info", &PlanExecutor::stream_info)
      .def("set_trace", &PlanExecutor::set_trace);
}
