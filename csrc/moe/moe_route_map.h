// The index arithmetic of the MoE routing sort (moe_route.hip), shared with its host-side test
// (tests/native/test_moe_route_map.cpp): how n = S * k slots are cut into chunks and wave runs,
// where a chunk's counts live in the int32 workspace, and how the scan cuts the chunk axis.
//
// Workspace (int32 words): table[chunks][E], then totals[E].
//   after the count launch  table[c][e] = slots of chunk c whose id is e
//   after the scan launch   table[c][e] = slots of chunks < c whose id is e, totals[e] = all of them
// The place launch adds the exclusive scan of totals (the experts' first rows, = offsets).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddlb {

constexpr int kRouteChunk = 1024;    // slots per workgroup of the count and place launches
constexpr int kRouteThreads = 256;   // their workgroup: 4 waves
constexpr int kRouteWaves = kRouteThreads / 64;
constexpr int kRouteRun = kRouteChunk / kRouteWaves;  // consecutive slots one wave places
constexpr int kRouteSteps = kRouteRun / 64;           // 64 slots per step
constexpr int kRouteScanCols = 64;   // experts per workgroup of the scan launch
constexpr int kRouteScanSegs = 16;   // its waves: each sums one segment of the chunk axis
constexpr int kRouteMaxExperts = 1024;

// chunks of n slots (n >= 0)
__host__ __device__ inline int route_chunks(int64_t n) {
  return (int)((n + kRouteChunk - 1) / kRouteChunk);
}

// the slot lane `lane` of wave `wave` takes in step `step` of chunk `chunk` (>= n: none)
__host__ __device__ inline int64_t route_slot(int chunk, int wave, int step, int lane) {
  return (int64_t)chunk * kRouteChunk + wave * kRouteRun + step * 64 + lane;
}

// word of table[chunk][e]
__host__ __device__ inline int64_t route_table_index(int chunk, int e, int E) {
  return (int64_t)chunk * E + e;
}

// word of totals[e]
__host__ __device__ inline int64_t route_totals_index(int chunks, int e, int E) {
  return (int64_t)chunks * E + e;
}

// words of the workspace for n slots and E experts
__host__ __device__ inline int64_t route_workspace_words(int64_t n, int E) {
  return ((int64_t)route_chunks(n) + 1) * E;
}

// the chunks [c0, c1) that segment seg of nseg takes in the scan: contiguous, in order, covering
// [0, chunks) exactly once
__host__ __device__ inline void route_scan_segment(int chunks, int nseg, int seg, int& c0,
                                                   int& c1) {
  c0 = (int)((int64_t)chunks * seg / nseg);
  c1 = (int)((int64_t)chunks * (seg + 1) / nseg);
}

// an id as the sort sees it: e in [0, E), or -1 (dropped)
__host__ __device__ inline int route_expert(int64_t id, int E) {
  return id >= 0 && id < E ? (int)id : -1;
}

// bits of the ids that tell experts apart: the smallest b with 2^b >= E (E = 1: 0)
__host__ __device__ inline int route_id_bits(int E) {
  int b = 0;
  while ((1 << b) < E) ++b;
  return b;
}

}  // namespace ddlb
