// MoE routing for gfx950: a stable counting sort of the n = S * k (token, choice) slots by expert
// id, on the device, in three launches in stream order (moe.h MoeRouteArgs has the contract).
//
//   count  every chunk of kRouteChunk slots histograms its ids in LDS (integer atomics: a count
//          does not depend on the order of its increments) and stores its E counts
//   scan   per expert, an exclusive scan down the chunk axis of that table, and the E totals
//   place  every chunk re-reads its ids and ranks each slot among the slots of its expert: experts
//          before it (a scan of the totals), chunks before it (the table), waves before it in the
//          chunk (per-wave LDS counts), steps before it in the wave (a running LDS count) and
//          lanes before it in the step (ballots over the bits of the id)
//
// Nothing here waits: no workgroup reads what another workgroup of the same launch writes, there
// are no flags, tickets or cooperative launches, and no global atomics, so the result is a function
// of the ids alone and the three kernels cannot hang. Ids outside [0, E) are dropped at the first
// read (moe_route_map.h route_expert) and never index anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moe.h"
#include "moe_route_map.h"

namespace ddlb {
namespace {

template <typename IdT>
__global__ __launch_bounds__(kRouteThreads) void moe_route_count_kernel(const MoeRouteArgs a) {
  __shared__ int cnt[kRouteMaxExperts];
  const int tid = threadIdx.x, chunk = blockIdx.x, E = a.E;
  const IdT* ids = (const IdT*)a.ids;
  for (int e = tid; e < E; e += kRouteThreads) cnt[e] = 0;
  __syncthreads();
#pragma unroll
  for (int st = 0; st < kRouteSteps; ++st) {
    const int64_t slot = route_slot(chunk, tid >> 6, st, tid & 63);
    const int e = slot < a.n ? route_expert((int64_t)ids[slot], E) : -1;
    if (e >= 0) atomicAdd(&cnt[e], 1);
  }
  __syncthreads();
  for (int e = tid; e < E; e += kRouteThreads) a.ws[route_table_index(chunk, e, E)] = cnt[e];
}

// One workgroup per kRouteScanCols experts, one wave per segment of the chunk axis: lane l owns
// expert e0 + l, sums its segment, takes the sums of the segments before it from LDS and walks the
// segment again storing the running count. 64 consecutive int32 per row: one 256-byte line.
__global__ __launch_bounds__(kRouteScanCols* kRouteScanSegs) void moe_route_scan_kernel(
    const MoeRouteArgs a, int chunks) {
  __shared__ int seg_sum[kRouteScanSegs][kRouteScanCols];
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6, E = a.E;
  const int e = blockIdx.x * kRouteScanCols + lane;
  const bool on = e < E;
  int c0, c1;
  route_scan_segment(chunks, kRouteScanSegs, seg, c0, c1);
  int sum = 0;
  if (on) {
#pragma unroll 4
    for (int c = c0; c < c1; ++c) sum += a.ws[route_table_index(c, e, E)];
  }
  seg_sum[seg][lane] = sum;
  __syncthreads();
  if (!on) return;
  int run = 0, total = 0;
#pragma unroll
  for (int s = 0; s < kRouteScanSegs; ++s) {
    const int v = seg_sum[s][lane];
    run += s < seg ? v : 0;
    total += v;
  }
#pragma unroll 4
  for (int c = c0; c < c1; ++c) {
    const int64_t i = route_table_index(c, e, E);
    const int v = a.ws[i];
    a.ws[i] = run;
    run += v;
  }
  if (seg == 0) a.ws[route_totals_index(chunks, e, E)] = total;
}

template <typename IdT>
__global__ __launch_bounds__(kRouteThreads) void moe_route_place_kernel(const MoeRouteArgs a,
                                                                        int chunks, int bits) {
  __shared__ int tbl[kRouteWaves][kRouteMaxExperts];  // per wave: counts, then next free rows
  __shared__ int ebase[kRouteMaxExperts];             // the experts' first rows (= offsets)
  __shared__ int wsum[kRouteWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x, E = a.E;
  const IdT* ids = (const IdT*)a.ids;

  // the exclusive scan of the E totals: PER consecutive experts per thread
  constexpr int PER = kRouteMaxExperts / kRouteThreads;
  int tot[PER], mine = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = tid * PER + i;
    tot[i] = e < E ? a.ws[route_totals_index(chunks, e, E)] : 0;
    mine += tot[i];
  }
  int inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d *= 2) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  for (int e = tid; e < E; e += kRouteThreads) {
#pragma unroll
    for (int w = 0; w < kRouteWaves; ++w) tbl[w][e] = 0;
  }
  __syncthreads();
  int before = 0, grand = 0;  // grand = offsets[E]: the slots that were not dropped
#pragma unroll
  for (int w = 0; w < kRouteWaves; ++w) {
    const int t = wsum[w];
    before += w < wave ? t : 0;
    grand += t;
  }
  int run = before + inc - mine;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = tid * PER + i;
    if (e < E) ebase[e] = run;
    run += tot[i];
  }

  // every wave counts the kRouteRun consecutive slots it will place
  int key[kRouteSteps];
#pragma unroll
  for (int st = 0; st < kRouteSteps; ++st) {
    const int64_t slot = route_slot(chunk, wave, st, lane);
    key[st] = slot < a.n ? route_expert((int64_t)ids[slot], E) : -1;
    if (key[st] >= 0) atomicAdd(&tbl[wave][key[st]], 1);
  }
  __syncthreads();
  // counts -> the first row of (expert, this chunk, wave)
  for (int e = tid; e < E; e += kRouteThreads) {
    int base = ebase[e] + a.ws[route_table_index(chunk, e, E)];
#pragma unroll
    for (int w = 0; w < kRouteWaves; ++w) {
      const int c = tbl[w][e];
      tbl[w][e] = base;
      base += c;
    }
  }
  __syncthreads();
  // 64 slots per step: peers = the lanes of this step with my expert, found bit by bit
#pragma unroll
  for (int st = 0; st < kRouteSteps; ++st) {
    const int e = key[st];
    const bool valid = e >= 0;
    uint64_t peers = __builtin_amdgcn_ballot_w64(valid);
    for (int b = 0; b < bits; ++b) {
      const bool bit = (e >> b) & 1;
      const uint64_t m = __builtin_amdgcn_ballot_w64(bit);
      peers &= bit ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1));
    const int cnt = __popcll(peers);
    const int base = valid ? tbl[wave][e] : 0;
    __syncthreads();  // (only this wave touches tbl[wave]; the trip count is uniform)
    if (valid && rank == cnt - 1) tbl[wave][e] = base + cnt;
    __syncthreads();
    const int64_t slot = route_slot(chunk, wave, st, lane);
    if (slot < a.n) {
      const int row = valid ? base + rank : -1;
      a.slot_row[slot] = row;
      // row < grand <= n by construction; the compare keeps the store inside row_token even if the
      // ids were overwritten between the launches
      if (valid && (int64_t)row < a.n) a.row_token[row] = (int)(slot / a.k);
    }
  }
  // the rows behind the sorted ones, and the offsets
  for (int i = tid; i < kRouteChunk; i += kRouteThreads) {
    const int64_t r = (int64_t)chunk * kRouteChunk + i;
    if (r >= grand && r < a.n) a.row_token[r] = -1;
  }
  if (chunk == 0) {
    for (int e = tid; e < E; e += kRouteThreads) a.offsets[e] = ebase[e];
    if (tid == 0) a.offsets[E] = grand;
  }
}

template <typename IdT>
hipError_t route_go(const MoeRouteArgs& a, hipStream_t s) {
  const int chunks = route_chunks(a.n);
  hipLaunchKernelGGL(moe_route_count_kernel<IdT>, dim3((unsigned)chunks), dim3(kRouteThreads), 0,
                     s, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int col_groups = (a.E + kRouteScanCols - 1) / kRouteScanCols;
  hipLaunchKernelGGL(moe_route_scan_kernel, dim3((unsigned)col_groups),
                     dim3(kRouteScanCols * kRouteScanSegs), 0, s, a, chunks);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(moe_route_place_kernel<IdT>, dim3((unsigned)chunks), dim3(kRouteThreads), 0,
                     s, a, chunks, route_id_bits(a.E));
  return hipGetLastError();
}

}  // namespace

hipError_t moe_route_launch(const MoeRouteArgs& a, hipStream_t s) {
  if (a.E < 1 || a.E > kRouteMaxExperts || a.k < 1 || a.n < 0 || a.n > 0x7FFFFFFFLL ||
      a.n % a.k)
    return hipErrorInvalidValue;
  if (a.n == 0) return hipSuccess;
  if (a.ids == nullptr || a.offsets == nullptr || a.row_token == nullptr ||
      a.slot_row == nullptr || a.ws == nullptr)
    return hipErrorInvalidValue;
  return a.ids64 ? route_go<int64_t>(a, s) : route_go<int32_t>(a, s);
}

}  // namespace ddlb
