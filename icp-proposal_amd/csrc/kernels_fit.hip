// kernels_fit.hip — many deterministic ICP fits side by side (icp_fit_deterministic_many; api/other/IcpBasedSurfaceFitting.scala:46-126).
//
// Every fit of a call advances recursion by recursion in lockstep on one stream; each launch below carries all fits (fit = blockIdx.y,
// or .z for the regression) and reads the fit's record — pointers, pose, search tasks, sample counts — from a device table made once per
// call.  The recursion's direction is read from the fit's row of the schedule (block-uniform: one fit per workgroup), so ModelSampling
// and TargetSampling fits share every launch.  The stages are the one-fit path's own device bodies (instance_point's sums,
// icp_search.hpp's init / filter / resolve, regression_tile, block_matvec), with the one-fit path's decomposition of every fit's work
// (split counts are functions of that fit's K alone): a fit's bits depend neither on the other fits of the call nor on their order.
#include <algorithm>

#include "icp_kernels.hpp"
#include "icp_search.hpp"
#include "icp_dense.hpp"

namespace icp {

namespace {

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ bool fit_model_side(const FitItem& f, int rec) { return f.dirs[rec] == 0; }

// F1: instances of up to kFitInstGroup fits from one pass over the basis (thread = model point).  The sums are instance_point's: the
// mean, then the basis columns in order with separately rounded multiply and add, then instance_pose — every fit's points are the bits
// of its own k_instance launch.  The coefficients are wave-uniform loads from the fit's device vector (no rank limit from LDS).
constexpr int kFitInstBlock = 64;
constexpr int kFitInstU = 8;  // basis columns (× 3 rows) in flight per batch of loads
__global__ void __launch_bounds__(kFitInstBlock) k_fit_instance(int B, int N, int r, const double* __restrict__ Qp, const double* __restrict__ ref,
                                                                const double* __restrict__ mean, const FitItem* __restrict__ items) {
  constexpr int G = kFitInstGroup;
  const int g0 = blockIdx.y * G, ng = min(G, B - g0);
  const int i = blockIdx.x * kFitInstBlock + threadIdx.x;
  if (i >= N) return;
  const double* cf[G];
#pragma unroll
  for (int g = 0; g < G; ++g) cf[g] = items[g0 + (g < ng ? g : 0)].coeffs;
  double a0[G], a1[G], a2[G];
  const double m0 = mean[3 * i], m1 = mean[3 * i + 1], m2 = mean[3 * i + 2];
#pragma unroll
  for (int g = 0; g < G; ++g) { a0[g] = m0; a1[g] = m1; a2[g] = m2; }
  const double* q = Qp + i;
  int j = 0;
  for (; j + kFitInstU <= r; j += kFitInstU) {
    double v[3 * kFitInstU];
#pragma unroll
    for (int u = 0; u < 3 * kFitInstU; ++u) v[u] = q[(size_t)(3 * j + u) * N];
    __builtin_amdgcn_sched_barrier(0);  // (all loads requested before the first multiply)
#pragma unroll
    for (int u = 0; u < kFitInstU; ++u)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const double c = cf[g][j + u];
        a0[g] = a0[g] + v[3 * u] * c;
        a1[g] = a1[g] + v[3 * u + 1] * c;
        a2[g] = a2[g] + v[3 * u + 2] * c;
      }
  }
  for (; j < r; ++j) {
    const double v0 = q[(size_t)(3 * j) * N], v1 = q[(size_t)(3 * j + 1) * N], v2 = q[(size_t)(3 * j + 2) * N];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const double c = cf[g][j];
      a0[g] = a0[g] + v0 * c;
      a1[g] = a1[g] + v1 * c;
      a2[g] = a2[g] + v2 * c;
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g >= ng) continue;
    const FitItem& f = items[g0 + g];
    const d3 p = instance_pose(i, ref, f.pose, a0[g], a1[g], a2[g]);  // ModelFittingParameters.scala:108-110
    f.x[3 * i] = p.x; f.x[3 * i + 1] = p.y; f.x[3 * i + 2] = p.z;
  }
}

// F2: the searches' initialisation.  Model side: gather the sample ids' points of the new instance (:72) and take each query's bound
// from its previous winner; target side: the nearest-vertex queries' bounds against the new instance.
__global__ void __launch_bounds__(kSearchBlock) k_fit_search_init(const FitItem* __restrict__ items, int rec) {
  const FitItem& f = items[blockIdx.y];
  const int k = blockIdx.x * kSearchBlock + threadIdx.x;
  if (fit_model_side(f, rec)) {
    if (k >= f.surf.Kpad) return;
    d3 p = {0.0, 0.0, 0.0};
    if (k < f.surf.K) {
      const int id = f.ids[k];
      p = ld3(f.x + 3 * id);
      f.P[3 * k] = p.x; f.P[3 * k + 1] = p.y; f.P[3 * k + 2] = p.z;
    }
    surface_init_at(f.surf, k, p);  // (k >= K: a sentinel slot)
  } else {
    vertex_init(f.vert, k);
  }
}

// F3: the filter of the fit's search this recursion (grid layout of k_wide_filter: see filter_grid_blocks)
__global__ void __launch_bounds__(kSearchBlock, 8) k_fit_filter(const FitItem* __restrict__ items, int rec) {
  const FitItem& f = items[blockIdx.y];
  const int l = blockIdx.x;
  if (fit_model_side(f, rec)) {
    const SurfaceTask& q = f.surf;
    if (l >= f.fblocks_m) return;
    const int bx = l / (8 * q.ksplit) * 8 + (l & 7), by = (l % (8 * q.ksplit)) >> 3;
    if (bx < q.tblocks) surface_filter<true>(q, bx, by);
  } else {
    const VertexTask& q = f.vert;
    if (l >= f.fblocks_t) return;
    const int bx = l / (8 * q.ksplit) * 8 + (l & 7), by = (l % (8 * q.ksplit)) >> 3;
    if (bx < q.vblocks) vertex_filter(q, bx, by);
  }
}

// correspondence row k with isotropic noise (k_correspond_plain): e = pt − x̄_id − μ_id in world space (:81), keep = 1, n̂ = 0
__device__ __forceinline__ void fit_write_corr(const CorrBuffers& cb, int k, int id, d3 p, const double* __restrict__ ref,
                                               const double* __restrict__ mean) {
  cb.id[k] = id; cb.aux[k] = -1; cb.keep[k] = 1;
  const double pv[3] = {p.x, p.y, p.z};
  for (int d = 0; d < 3; ++d) {
    cb.pt[3 * k + d] = pv[d];
    cb.nhat[3 * k + d] = 0.0;
    cb.e[3 * k + d] = (pv[d] - ref[3 * id + d]) - mean[3 * id + d];
  }
}

// F4: one wave per query — the exact winner, then the fit's correspondence row (model side :72-74, target side :76-78)
__global__ void __launch_bounds__(64) k_fit_resolve(const FitItem* __restrict__ items, int rec, int N, const double* __restrict__ ref,
                                                    const double* __restrict__ mean) {
  const FitItem& f = items[blockIdx.y];
  const int k = blockIdx.x;
  if (fit_model_side(f, rec)) {
    if (k >= f.surf.K) return;
    double best; int tri; d3 cp;
    surface_resolve(f.surf, k, &best, &tri, &cp);
    if (lane_id() == 0) fit_write_corr(f.cb, k, f.ids[k], cp, ref, mean);
  } else {
    if (k >= f.vert.K) return;
    double best; int idx;
    vertex_resolve(f.vert, k, &best, &idx);
    // (no winner only for a non-finite instance: that fit's coefficients are non-finite already; the row stays in bounds)
    const int id = idx >= 0 && idx < N ? idx : 0;
    if (lane_id() == 0) fit_write_corr(f.cb, k, id, ld3(f.tpts + 3 * k), ref, mean);
  }
}

// F5: split-K partial sums of every fit's normal equations (k_regression_mfma: blockIdx.x = split, .y = tile), fit = blockIdx.z
__global__ void __launch_bounds__(64) k_fit_regression(const FitItem* __restrict__ items, int rec, int r, const double* __restrict__ Q,
                                                       double wt) {
  const FitItem& f = items[blockIdx.z];
  const bool ms = fit_model_side(f, rec);
  const int K = ms ? f.surf.K : f.vert.K, S = ms ? f.splits_m : f.splits_t;
  if ((int)blockIdx.x >= S) return;
  regression_tile(blockIdx.y, blockIdx.x, K, cdiv(K, S), r, Q, f.cb, wt, 0.0, f.Mpart);
}

// F6: the mean step of every fit (k_mean_step; one workgroup per fit), and the fit's sticky status: a factorisation that failed in
// any recursion fails the fit
__global__ void __launch_bounds__(256) k_fit_mean_step(const FitItem* __restrict__ items, int r, const double* __restrict__ P, double sigma2,
                                                       int tpr_log2) {
  __shared__ double s_a[512], s_y[512];
  const FitItem& f = items[blockIdx.x];
  if (threadIdx.x == 0 && f.factor_status[0] != 0) f.status[0] = 1;
  for (int i = threadIdx.x; i < r; i += blockDim.x) s_a[i] = f.alpha[i];
  __syncthreads();
  block_matvec(r, P, r, s_a, s_y, tpr_log2);
  double* c = f.coeffs;
  for (int i = threadIdx.x; i < r; i += blockDim.x) {
    const double cnew = fma(-sigma2, s_y[i], s_a[i]);   // model.coefficients(posterior.mean) (:84)
    c[i] = c[i] + (cnew - c[i]) * f.step;               // :85
  }
}

}  // namespace

int query_kpad(int K) { return (K + kQU - 1) / kQU * kQU; }

void launch_fit_instance(hipStream_t st, int B, int N, int r, const double* Qp, const double* ref, const double* mean, const FitItem* items) {
  ProfScope _ps(st, KID_INSTANCE);
  hipLaunchKernelGGL(k_fit_instance, dim3(cdiv(N, kFitInstBlock), cdiv(B, kFitInstGroup)), dim3(kFitInstBlock), 0, st, B, N, r, Qp, ref, mean, items);
}

void launch_fit_searches(hipStream_t st, int B, int rec, const FitGrid& g, int N, const double* ref, const double* mean, const FitItem* items) {
  { ProfScope _ps(st, KID_SURFACE_INIT);
    hipLaunchKernelGGL(k_fit_search_init, dim3(cdiv(g.kpad, kSearchBlock), B), dim3(kSearchBlock), 0, st, items, rec); }
  { ProfScope _ps(st, KID_SURFACE_FILTER);
    hipLaunchKernelGGL(k_fit_filter, dim3(g.filter, B), dim3(kSearchBlock), 0, st, items, rec); }
  { ProfScope _ps(st, KID_SURFACE_RESOLVE);
    hipLaunchKernelGGL(k_fit_resolve, dim3(g.kmax, B), dim3(64), 0, st, items, rec, N, ref, mean); }
}

void launch_fit_regression(hipStream_t st, int B, int rec, const FitGrid& g, int r, const double* Q, double wt, const FitItem* items) {
  ProfScope _ps(st, KID_REGRESSION);
  hipLaunchKernelGGL(k_fit_regression, dim3(g.splits, regression_tiles(r), B), dim3(64), 0, st, items, rec, r, Q, wt);
}

void launch_fit_mean_step(hipStream_t st, int B, int r, const double* P, double sigma2, const FitItem* items) {
  ProfScope _ps(st, KID_TAIL);
  hipLaunchKernelGGL(k_fit_mean_step, dim3(B), dim3(256), 0, st, items, r, P, sigma2, matvec_tpr_log2(r, 256));
}

}  // namespace icp
