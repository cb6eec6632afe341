// What the skinny-M GEMM kernels share behind their K-loops (gemm_skinny.hip: block-scaled
// activations; gemm_skinny_a16.hip: bf16 / f16 activations): the epilogue tail a lane ends in with
// four consecutive output columns of one row, and the two kernels that sum the K-slices of a
// split launch. Device code, header-only, one copy per translation unit (as gemm_kernels.h).
#pragma once
#include "gemm_skinny.h"

#include "gemm_kernels.h"
#include "row_io.h"

namespace ddlb {
namespace {

// ---------------------------------------------------------------- the epilogue tail
// The output kind is one compile-time pair: OUT (bf16 / f16 / f32 dense, DT_FP8 / DT_FP4 quantised
// by the rule of mx_cvt.h) and GLU. A lane holds four consecutive output columns of one row.
template <int OUT> constexpr bool skinny_qout() { return OUT == DT_FP8 || OUT == DT_FP4; }
template <int OUT> constexpr int skinny_bytes4() {  // bytes of four output columns
  return OUT == DT_F32 ? 16 : OUT == DT_FP8 ? 4 : OUT == DT_FP4 ? 2 : 8;
}

// act(gate) * up: one f32 multiply, materialised before any conversion (row_io.h row_keep_f32)
__device__ __forceinline__ f32x4 skinny_gate(const f32x4 g, const f32x4 u, int act) {
  const f32x4 a = act4(g, act);
  return f32x4{row_keep_f32(a.x * u.x), row_keep_f32(a.y * u.y), row_keep_f32(a.z * u.z),
               row_keep_f32(a.w * u.w)};
}

// the four values' contribution to their block's amax word (dense outputs carry none)
template <int OUT>
__device__ __forceinline__ unsigned skinny_amax4(unsigned m, const f32x4 v) {
  if constexpr (skinny_qout<OUT>()) {
    constexpr bool Q4 = OUT == DT_FP4;
    m = mx_amax_join<Q4>(m, mx_amax_bits<Q4>(v.x));
    m = mx_amax_join<Q4>(m, mx_amax_bits<Q4>(v.y));
    m = mx_amax_join<Q4>(m, mx_amax_bits<Q4>(v.z));
    m = mx_amax_join<Q4>(m, mx_amax_bits<Q4>(v.w));
  }
  return m;
}
template <int OUT>
__device__ __forceinline__ unsigned skinny_amax_xor(unsigned m, int d) {
  if constexpr (skinny_qout<OUT>())
    m = mx_amax_join<OUT == DT_FP4>(m, (unsigned)__shfl_xor((int)m, d));
  return m;
}

// Four f32 values and their block's amax word -> one dword of e4m3, two bytes of E2M1, or a dense
// Store4 at dst; the block's scale byte at sdst from the one lane that is given it.
template <int OUT>
__device__ __forceinline__ void skinny_tail(char* dst, uint8_t* sdst, const f32x4 v, unsigned m) {
  if constexpr (skinny_qout<OUT>()) {
    constexpr bool Q4 = OUT == DT_FP4;
    const int e = mx_scale_exp<Q4>(m);
    if constexpr (Q4) {
      const float sc = mx_fp4_scale(e);
      unsigned w = mx_cvt2_e2m1<0>(0u, v.x, v.y, sc);
      w = mx_cvt2_e2m1<1>(w, v.z, v.w, sc);
      *(unsigned short*)dst = (unsigned short)w;
    } else {
      *(unsigned*)dst = mx_cvt4_e4m3(v.x, v.y, v.z, v.w, e);
    }
    if (sdst != nullptr) *sdst = (uint8_t)mx_scale_byte<Q4>(m, e);
  } else {
    Store4<OUT>::st(dst, v);
  }
}

// Columns col .. col + 3 of the row at crow, of ncols: the tail, or (dense rows that are ragged
// or not aligned for the vector store) element by element. A quantised row holds whole blocks.
template <int OUT>
__device__ __forceinline__ void skinny_store4(char* crow, int64_t col, int64_t ncols, bool vec,
                                              uint8_t* sdst, const f32x4 v4, unsigned m) {
  constexpr int B4 = skinny_bytes4<OUT>();
  if (col + 3 < ncols && (skinny_qout<OUT>() || vec)) {
    skinny_tail<OUT>(crow + (col >> 2) * B4, sdst, v4, m);
  } else if constexpr (!skinny_qout<OUT>()) {
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
    for (int r = 0; r < 4; ++r)
      if (col + r < ncols) Store4<OUT>::st1(crow + (col + r) * (B4 / 4), v[r]);
  }
}
// whether a dense output's rows take the vector store
template <int OUT>
__device__ __forceinline__ bool skinny_vec(const SkinnyArgs& p) {
  constexpr int B4 = skinny_bytes4<OUT>();
  return ((((uintptr_t)p.c | (uint64_t)(p.ldc * (B4 / 4))) & (B4 - 1)) == 0);
}

// ---------------------------------------------------------------- the sum of the K-slices
// C[row, col] = round(act(sum over s = 0 .. S - 1, in that order, of ws[s][row][col])): one
// workgroup per (row, 256 columns). Grouped: rows [o'[0], o'[E]) only, read from the offsets here.
template <int OUT>
__global__ __launch_bounds__(256) void skinny_reduce_kernel(const SkinnyArgs p, const int S) {
  int r0 = 0, r1 = p.M;
  if (p.offs != nullptr) skinny_group_rows(p.offs, p.M, -1, p.ngroups, r0, r1);
  const int64_t row = (int64_t)r0 + blockIdx.x;
  const int64_t col = (int64_t)blockIdx.y * 256 + threadIdx.x;
  if (row >= r1 || col >= p.N) return;
  const GLB_AS float* src = (const GLB_AS float*)p.ws + row * p.N + col;
  const int64_t step = (int64_t)p.M * p.N;
  float acc = src[0];
#pragma unroll 4
  for (int s = 1; s < S; ++s) acc += src[s * step];
  constexpr int OSZ = out_size<OUT>();
  Store4<OUT>::st1((char*)p.c + (row * p.ldc + col) * OSZ, act1(acc, p.act));
}

// The gated and / or quantising form of the reduce: a lane sums four consecutive columns of the
// S slices in the same order (gated: the gate quad at 64 g + 4 t and the up quad at
// 64 g + 32 + 4 t of output columns 32 g + 4 t ..), eight adjacent lanes are one 32-column block
// (three cross-lane steps join its amax word), each lane stores its own quad and lane t = 0 the
// scale byte. Rows of whole blocks (N % 64 == 0 at least), so a row is ncols / 4 quads, a
// multiple of 8, and a block never straddles rows or the range's end. Grouped: as above.
template <int OUT, bool GLU>
__global__ __launch_bounds__(256) void skinny_epilogue_kernel(const SkinnyArgs p, const int S) {
  int r0 = 0, r1 = p.M;
  if (p.offs != nullptr) skinny_group_rows(p.offs, p.M, -1, p.ngroups, r0, r1);
  const int64_t ncols = GLU ? p.N / 2 : p.N;
  const int qpr = (int)(ncols / 4);
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = (int64_t)r0 + q / qpr;
  const int t4 = (int)(q % qpr);
  const bool ok = row < r1;  // the same for the eight lanes of a block
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (ok) {
    const GLB_AS float* src = (const GLB_AS float*)p.ws + row * p.N +
                              (GLU ? 64 * (t4 >> 3) + 4 * (t4 & 7) : 4 * t4);
    const int64_t step = (int64_t)p.M * p.N;
    f32x4 g = *(const GLB_AS f32x4*)src;
#pragma unroll 4
    for (int s = 1; s < S; ++s) g += *(const GLB_AS f32x4*)(src + s * step);
    if constexpr (GLU) {
      f32x4 u = *(const GLB_AS f32x4*)(src + 32);
#pragma unroll 4
      for (int s = 1; s < S; ++s) u += *(const GLB_AS f32x4*)(src + 32 + s * step);
      v = skinny_gate(g, u, p.act);
    } else {
      v = act4(g, p.act);
    }
  }
  unsigned m = skinny_amax4<OUT>(0u, v);
#pragma unroll
  for (int d = 1; d <= 4; d *= 2) m = skinny_amax_xor<OUT>(m, d);
  if (!ok) return;
  uint8_t* sdst = nullptr;
  if constexpr (skinny_qout<OUT>())
    if ((t4 & 7) == 0) sdst = p.c_scale + row * p.c_scale_ld + (t4 >> 3);
  skinny_store4<OUT>((char*)p.c + row * p.ldc * skinny_bytes4<OUT>() / 4, 4 * (int64_t)t4, ncols,
                     skinny_vec<OUT>(p), sdst, v, m);
}

// The kernels behind the partial kernel of a split launch (S > 1): the plain reduce, or the
// gated / quantising epilogue.
template <int OUT>
hipError_t skinny_launch_reduce(const SkinnyArgs& p, int S, hipStream_t s) {
  const dim3 rgrid((unsigned)p.M, (unsigned)((p.N + 255) / 256));
  hipLaunchKernelGGL((skinny_reduce_kernel<OUT>), rgrid, dim3(256), 0, s, p, S);
  return hipGetLastError();
}
template <int OUT, bool GLU>
hipError_t skinny_launch_epilogue(const SkinnyArgs& p, int S, hipStream_t s) {
  const int64_t quads = (int64_t)p.M * ((GLU ? p.N / 2 : p.N) / 4);
  const dim3 egrid((unsigned)((quads + 255) / 256));
  hipLaunchKernelGGL((skinny_epilogue_kernel<OUT, GLU>), egrid, dim3(256), 0, s, p, S);
  return hipGetLastError();
}

}  // namespace
}  // namespace ddlb
