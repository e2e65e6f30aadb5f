// kernels_maps.hip — per-vertex registration maps of many meshes and the maps a chain's samples imply (icp_registration_maps_many,
// icp_distance_summaries_many).
//
// The searches are the metrics' launches (kernels_metrics.hip): this file holds what comes behind them.  Both kernels are plain
// per-vertex work — thread = vertex, record = blockIdx.y, neighbouring vertices read and write neighbouring words — with the
// distance taken in the expression k_dist_stats / k_met_stats reduce: sqrt of the search's squared distance.  No atomics.
#include "icp_kernels.hpp"

namespace icp {

namespace {

constexpr int kMapBlock = 256;

// the rows of one direction at vertex i; bad: the item's mesh is not finite
__device__ __forceinline__ void map_side_row(const MapSide& s, int i, bool bad) {
  if (i >= s.K) return;
  if (bad) {
    const double nan = __builtin_nan("");
    if (s.cp) { s.cp[3 * i] = nan; s.cp[3 * i + 1] = nan; s.cp[3 * i + 2] = nan; }
    if (s.tri) s.tri[i] = -1;
    if (s.dist) s.dist[i] = nan;
    return;
  }
  if (s.dist) s.dist[i] = sqrt(s.d2[i]);
}

// P1: the map epilogue, item = blockIdx.y.  The points and triangles stay where the searches wrote them (the staging rows)
__global__ void __launch_bounds__(kMapBlock) k_map_rows(const MapItem* __restrict__ items) {
  const MapItem& it = items[blockIdx.y];
  const int i = blockIdx.x * kMapBlock + threadIdx.x;
  const bool bad = it.nonfinite[0] != 0;
  map_side_row(it.m2t, i, bad);
  map_side_row(it.t2m, i, bad);
  if (it.flag && i < it.m2t.K) {
    unsigned char f = 0;
    if (!bad && it.nnv) {
      const int v = it.nnv[i];
      f = (v >= 0 && v < it.n_flags && it.boundary[v] != 0) ? 1 : 0;  // (k_met_stats' test)
    }
    it.flag[i] = f;
  }
}

// P2: Σ d in sample order and max d of a segment's samples, segment = blockIdx.y; the set's last segment divides once
__global__ void __launch_bounds__(kMapBlock) k_map_summaries(const MapSumSeg* __restrict__ segs) {
  const MapSumSeg& g = segs[blockIdx.y];
  const int i = blockIdx.x * kMapBlock + threadIdx.x;
  if (i >= g.K) return;
  int bad = g.first ? 0 : g.bad[0];
  for (int s = 0; s < g.n; ++s) bad |= g.nonfinite[s];
  double sum = 0.0, mx = -__builtin_inf();
  if (!g.first) { sum = g.acc_in[i]; mx = g.acc_in[g.K + i]; }
  const double* d2 = g.d2 + i;
  for (int s = 0; s < g.n; ++s) {
    const double d = sqrt(d2[(size_t)s * g.K]);
    sum += d;
    mx = fmax(mx, d);
  }
  if (!g.last) {
    g.acc_out[i] = sum; g.acc_out[g.K + i] = mx;
    if (i == 0 && bad) g.bad[0] = 1;
    return;
  }
  if (i == 0 && bad) g.bad[0] = 1;
  const double nan = __builtin_nan("");
  if (g.mean) g.mean[i] = bad ? nan : sum / (double)g.S;
  if (g.max) g.max[i] = bad ? nan : mx;
}

}  // namespace

void launch_map_rows(hipStream_t st, int n_items, int kmax, const MapItem* items) {
  if (n_items <= 0 || kmax <= 0) return;
  hipLaunchKernelGGL(k_map_rows, dim3(cdiv(kmax, kMapBlock), n_items), dim3(kMapBlock), 0, st, items);
}

void launch_map_summaries(hipStream_t st, int n_segs, int kmax, const MapSumSeg* segs) {
  if (n_segs <= 0 || kmax <= 0) return;
  ProfScope _ps(st, KID_REDUCE);
  hipLaunchKernelGGL(k_map_summaries, dim3(cdiv(kmax, kMapBlock), n_segs), dim3(kMapBlock), 0, st, segs);
}

}  // namespace icp
