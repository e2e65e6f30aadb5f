// kernels_metrics.hip — registration metrics of many meshes side by side (icp_mesh_metrics_many; apps/femur/
// StdIcpVsChainICPrandomInitComparisonAll.scala:43-64, MeshMetrics.avgDistance / hausdorffDistance / diceCoefficient).
//
// Every launch carries all items of a chunk (item or search = blockIdx.y, stats job = blockIdx.x) and reads its record from a device
// table made once per call.  The stages are the one-item path's device bodies: tri_sphere, vertex_normal, icp_search.hpp's init /
// filter / resolve, k_dist_stats' loop and block reductions at the one-item path's block size.  A search's winner is the exact
// lexicographic (d², index) minimum whatever its hint and however its queries are split, so no result depends on the other items.
#include <algorithm>

#include "icp_kernels.hpp"
#include "icp_search.hpp"
#include "icp_dense.hpp"

namespace icp {

namespace {

// orc_rng_uniform (oracle/icp_oracle.c): splitmix64 over (seed, step, lane) -> (0, 1), exact in double
__device__ __forceinline__ unsigned long long met_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ double met_uniform(unsigned long long seed, unsigned long long step, unsigned long long lane) {
  const unsigned long long h = met_splitmix64(met_splitmix64(met_splitmix64(seed) ^ (step * 0xD1342543DE82EF95ull)) ^ (lane * 0x2545F4914F6CDD1Dull));
  return ((double)(h >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// M1: the item's model triangle spheres in the sphere-list order of the model (k_tri_spheres with tri_order), item = blockIdx.y
__global__ void __launch_bounds__(kSearchBlock) k_met_spheres(int T, const int* __restrict__ tris,
                                                             const int* __restrict__ order, const MetItem* __restrict__ items) {
  const MetItem& it = items[blockIdx.y];
  const int pos = blockIdx.x * kSearchBlock + threadIdx.x;
  if (pos >= T) return;
  const int t = order[pos];
  it.spheres[pos] = tri_sphere(it.x, tris, t);
  sphere_triangles(it.spheres, T)[pos] = t;
}

// M2: the item's vertex normals (k_vertex_normals), item = blockIdx.y
__global__ void __launch_bounds__(kSearchBlock) k_met_normals(int N, const int* __restrict__ tris, const int* __restrict__ adj_off,
                                                             const int* __restrict__ adj, const MetItem* __restrict__ items) {
  const MetItem& it = items[blockIdx.y];
  const int v = blockIdx.x * kSearchBlock + threadIdx.x;
  if (v >= N) return;
  const d3 n = vertex_normal(it.x, tris, adj_off, adj, v);
  it.normals[3 * v] = n.x; it.normals[3 * v + 1] = n.y; it.normals[3 * v + 2] = n.z;
}

// M3: axis-aligned box of a vertex set (min / max are exact: any order), united with `with` if given; counts non-finite
// coordinates into *nonfinite.  One workgroup per job.
constexpr int kBoxBlock = 256;
__global__ void __launch_bounds__(kBoxBlock) k_met_box(const MetBoxJob* __restrict__ jobs) {
  __shared__ double s_lo[3][kBoxBlock / 64], s_hi[3][kBoxBlock / 64];
  __shared__ int s_bad[kBoxBlock / 64];
  const MetBoxJob& j = jobs[blockIdx.x];
  double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
  int bad = 0;
  for (int v = threadIdx.x; v < j.n; v += kBoxBlock)
    for (int d = 0; d < 3; ++d) {
      const double c = j.verts[3 * v + d];
      if (!(fabs(c) <= 1.7976931348623157e308)) { ++bad; continue; }
      lo[d] = fmin(lo[d], c); hi[d] = fmax(hi[d], c);
    }
  for (int o = 32; o > 0; o >>= 1) {
    for (int d = 0; d < 3; ++d) { lo[d] = fmin(lo[d], __shfl_xor(lo[d], o, 64)); hi[d] = fmax(hi[d], __shfl_xor(hi[d], o, 64)); }
    bad += __shfl_xor(bad, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    for (int d = 0; d < 3; ++d) { s_lo[d][w] = lo[d]; s_hi[d][w] = hi[d]; }
    s_bad[w] = bad;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int nb = 0;
  for (int d = 0; d < 3; ++d) {
    double l = s_lo[d][0], h = s_hi[d][0];
    for (int k = 1; k < kBoxBlock / 64; ++k) { l = fmin(l, s_lo[d][k]); h = fmax(h, s_hi[d][k]); }
    if (j.with) { l = fmin(l, j.with[d]); h = fmax(h, j.with[3 + d]); }
    j.out[d] = l; j.out[3 + d] = h;
  }
  for (int k = 0; k < kBoxBlock / 64; ++k) nb += s_bad[k];
  if (j.nonfinite) j.nonfinite[0] = nb;
}

// M4: the searches' initialisation.  A query's hint — an upper bound only: any element gives the exact winner — is the nearest of
// a strided subset of the searched set (every hint_step-th sphere centre / vertex), or, hint_step == 0, the first corner of the
// triangle hint_tri[k] of hint_tris (the nearest target vertex of a surface point: a corner of the triangle it lies on)
__global__ void __launch_bounds__(kSearchBlock) k_met_search_init(const MetSearch* __restrict__ jobs) {
  const MetSearch& j = jobs[blockIdx.y];
  const int k = blockIdx.x * kSearchBlock + threadIdx.x;
  if (j.kind == 0) {
    const SurfaceTask& q = j.s;
    if (k >= q.Kpad) return;
    d3 p = {0.0, 0.0, 0.0};
    if (k < q.K) {
      p = ld3(q.P + 3 * k);
      int best_pos = -1;
      double best = __builtin_inf();
      for (int pos = 0; pos < q.T; pos += j.hint_step) {
        const float4 s = q.spheres[pos];
        const double dx = p.x - (double)s.x, dy = p.y - (double)s.y, dz = p.z - (double)s.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best) { best = d2; best_pos = pos; }
      }
      q.hint[k] = best_pos >= 0 ? sphere_triangles(q.spheres, q.T)[best_pos] : -1;
    }
    surface_init_at(q, k, p);
  } else {
    const VertexTask& q = j.v;
    if (k >= q.Kpad) return;
    if (k < q.K) {
      int h = -1;
      if (j.hint_step > 0) {
        const d3 p = ld3(q.P + 3 * k);
        double best = __builtin_inf();
        for (int v = 0; v < q.V; v += j.hint_step) {
          const d3 d = sub(p, ld3(q.verts + 3 * v));
          const double d2 = dot(d, d);
          if (d2 < best) { best = d2; h = v; }
        }
      } else {
        const int t = j.hint_tri[k];
        h = t >= 0 ? j.hint_tris[3 * t] : -1;
      }
      q.hint[k] = h;
    }
    vertex_init(q, k);
  }
}

// M5: the filter of every search (grid layout of k_fit_filter: see filter_grid_blocks), search = blockIdx.y
__global__ void __launch_bounds__(kSearchBlock, 8) k_met_filter(const MetSearch* __restrict__ jobs) {
  const MetSearch& j = jobs[blockIdx.y];
  const int l = blockIdx.x;
  if (l >= j.fblocks) return;
  if (j.kind == 0) {
    const SurfaceTask& q = j.s;
    const int bx = l / (8 * q.ksplit) * 8 + (l & 7), by = (l % (8 * q.ksplit)) >> 3;
    if (bx < q.tblocks) surface_filter<true>(q, bx, by);
  } else {
    const VertexTask& q = j.v;
    const int bx = l / (8 * q.ksplit) * 8 + (l & 7), by = (l % (8 * q.ksplit)) >> 3;
    if (bx < q.vblocks) vertex_filter(q, bx, by);
  }
}

// M6: one wave per query: the exact winner (the task's outputs are written by surface_resolve / vertex_resolve)
__global__ void __launch_bounds__(64) k_met_resolve(const MetSearch* __restrict__ jobs) {
  const MetSearch& j = jobs[blockIdx.y];
  const int k = blockIdx.x;
  if (j.kind == 0) {
    if (k >= j.s.K) return;
    double best; int tri; d3 cp;
    surface_resolve(j.s, k, &best, &tri, &cp);
  } else {
    if (k >= j.v.K) return;
    double best; int idx;
    vertex_resolve(j.v, k, &best, &idx);
  }
}

// M7: Σ kept distances, their maximum and count — k_dist_stats' loop and reductions at the one-item path's block size
// (launch_dist_stats: 1024 threads above 4,096 distances, else kSearchBlock), one workgroup per job
template <int kThreads>
__global__ void __launch_bounds__(kThreads) k_met_stats(const MetStats* __restrict__ jobs) {
  __shared__ double s_red[16];
  const MetStats& j = jobs[blockIdx.x];
  const int K = j.K;
  double sum = 0.0, mx = -__builtin_inf(), cnt = 0.0;
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    bool drop = false;
    if (j.flags) {
      int i = j.idx ? j.idx[k] : k;
      drop = (i >= 0 && i < j.n_flags) ? j.flags[i] != 0 : false;
    }
    if (!drop) {
      double d = sqrt(j.d2[k]);
      sum += d;
      mx = fmax(mx, d);
      cnt += 1.0;
    }
  }
  sum = block_sum(sum, s_red);
  cnt = block_sum(cnt, s_red);
  mx = block_max(mx, s_red);
  if (threadIdx.x == 0) { j.out[0] = sum; j.out[1] = mx; j.out[2] = cnt; }
}

// M8: Dice's sample points, p_k = lo_k + u(s, k)·(hi_k − lo_k) in the item's evaluation box (subtract, multiply, add: each rounded)
constexpr int kDiceBlock = 256;
__global__ void __launch_bounds__(kDiceBlock) k_met_samples(unsigned long long seed, const MetDice* __restrict__ jobs) {
  const MetDice& j = jobs[blockIdx.y];
  const int k = blockIdx.x * kDiceBlock + threadIdx.x;
  if (k >= j.n) return;
  const unsigned long long s = (unsigned long long)(j.s0 + k);
  for (int d = 0; d < 3; ++d) {
    const double lo = j.box[d], w = j.box[3 + d] - lo;
    const double t = met_uniform(seed, s, (unsigned long long)d) * w;
    j.P[3 * k + d] = lo + t;
  }
}

// (n.x·(v.x − p.x) + n.y·(v.y − p.y)) + n.z·(v.z − p.z) > 0 with v the nearest vertex, n its vertex normal
__device__ __forceinline__ bool met_inside(d3 p, const double* __restrict__ x, const double* __restrict__ nrm, int nv, int v) {
  if (v < 0 || v >= nv) return false;
  const d3 q = ld3(x + 3 * v), n = ld3(nrm + 3 * v);
  return (n.x * (q.x - p.x) + n.y * (q.y - p.y)) + n.z * (q.z - p.z) > 0.0;
}

// M9: classify and count — per workgroup sums, then one integer atomicAdd per workgroup and counter (order-free: exact)
__global__ void __launch_bounds__(kDiceBlock) k_met_dice_count(const MetDice* __restrict__ jobs) {
  __shared__ unsigned s_c[3][kDiceBlock / 64];
  const MetDice& j = jobs[blockIdx.y];
  const int k = blockIdx.x * kDiceBlock + threadIdx.x;
  bool a = false, b = false;
  if (k < j.n) {
    const d3 p = ld3(j.P + 3 * k);
    a = met_inside(p, j.xA, j.nA, j.NA, j.idxA[k]);
    b = met_inside(p, j.xB, j.nB, j.NB, j.idxB[k]);
  }
  const unsigned ca = (unsigned)__popcll(__ballot(a)), cb = (unsigned)__popcll(__ballot(b)), cab = (unsigned)__popcll(__ballot(a && b));
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_c[0][w] = ca; s_c[1][w] = cb; s_c[2][w] = cab; }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned t = 0;
    for (int i = 0; i < kDiceBlock / 64; ++i) t += s_c[threadIdx.x][i];
    if (t) atomicAdd(j.counts + threadIdx.x, t);
  }
}

}  // namespace

void launch_met_items(hipStream_t st, int B, int N, int T, const int* tris, const int* tri_order, const int* adj_off, const int* adj,
                      bool normals, const MetItem* items) {
  if (B <= 0) return;
  { ProfScope _ps(st, KID_TRI_SPHERES);
    hipLaunchKernelGGL(k_met_spheres, dim3(cdiv(T, kSearchBlock), B), dim3(kSearchBlock), 0, st, T, tris, tri_order, items); }
  if (normals) hipLaunchKernelGGL(k_met_normals, dim3(cdiv(N, kSearchBlock), B), dim3(kSearchBlock), 0, st, N, tris, adj_off, adj, items);
}

void launch_met_box(hipStream_t st, int n, const MetBoxJob* jobs) {
  if (n <= 0) return;
  ProfScope _ps(st, KID_REDUCE);
  hipLaunchKernelGGL(k_met_box, dim3(n), dim3(kBoxBlock), 0, st, jobs);
}

void launch_met_searches(hipStream_t st, int n, int kpad_max, int filter_max, int kmax, const MetSearch* jobs) {
  if (n <= 0) return;
  { ProfScope _ps(st, KID_SURFACE_INIT);
    hipLaunchKernelGGL(k_met_search_init, dim3(cdiv(kpad_max, kSearchBlock), n), dim3(kSearchBlock), 0, st, jobs); }
  if (filter_max > 0) {
    ProfScope _ps(st, KID_SURFACE_FILTER);
    hipLaunchKernelGGL(k_met_filter, dim3(filter_max, n), dim3(kSearchBlock), 0, st, jobs);
  }
  { ProfScope _ps(st, KID_SURFACE_RESOLVE);
    hipLaunchKernelGGL(k_met_resolve, dim3(kmax, n), dim3(64), 0, st, jobs); }
}

void launch_met_stats(hipStream_t st, int n, bool big, const MetStats* jobs) {
  if (n <= 0) return;
  ProfScope _ps(st, KID_REDUCE);
  if (big) hipLaunchKernelGGL(k_met_stats<1024>, dim3(n), dim3(1024), 0, st, jobs);
  else hipLaunchKernelGGL(k_met_stats<kSearchBlock>, dim3(n), dim3(kSearchBlock), 0, st, jobs);
}

void launch_met_samples(hipStream_t st, int n, int nmax, uint64_t seed, const MetDice* jobs) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_met_samples, dim3(cdiv(nmax, kDiceBlock), n), dim3(kDiceBlock), 0, st, (unsigned long long)seed, jobs);
}

void launch_met_dice_count(hipStream_t st, int n, int nmax, const MetDice* jobs) {
  if (n <= 0) return;
  ProfScope _ps(st, KID_REDUCE);
  hipLaunchKernelGGL(k_met_dice_count, dim3(cdiv(nmax, kDiceBlock), n), dim3(kDiceBlock), 0, st, jobs);
}

}  // namespace icp
