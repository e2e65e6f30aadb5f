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

__device__ __forceinline__ bool fit_model_side(const FitItem& f, int rec) { return f.dirs[rec] == 0; }

// F1: the fits' instances are one launch_instance_many (kernels_geometry.hip) over the call's instance records.

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
