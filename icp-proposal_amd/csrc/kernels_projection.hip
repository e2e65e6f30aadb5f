// kernels_projection.hip — model projection of many meshes side by side (icp_model_coefficients_many; Scalismo's
// DiscreteLowRankGaussianProcess.coefficients / project as apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:53-55,
// api/other/IcpBasedSurfaceFitting.scala:84 and NonRigidIcpProposal.scala:59 call them): c = (QᵀQ + σ²I)⁻¹ Qᵀ(x − x̄ − μ).
//
// The meshes of a call pass through one chunk buffer, chunk by chunk; every launch of a chunk carries all its items:
//   P1 k_proj_residual  thread = vertex, blockIdx.y = item: the inverse rigid pose where one is given (write_corr's expression), minus
//                       x̄ and μ, non-finite vertices counted; writes D[group][row][16]: the 16 items of a group side by side
//   P2 k_proj_gemm      b = Qᵀ·D on the f64 matrix cores: a wave owns up to kProjTiles 16 × 16 output tiles (basis columns × items of one
//                       group) over one slab of rows, so the basis is read once per group of 16 items
//   P3 k_proj_solve     one workgroup per item: the slabs' partial sums folded in slab order, then c = P·b in column order
// The meshes of items given as states, and the projections asked for, are instanced by k_instance_many (kernels_geometry.hip).
//
// An item's bits depend on nothing but the item: its residuals are its own; a column of the matrix instruction never sees another
// column's data (D[i][j] = Σ_k A[i][k]·B[k][j]: item j's sums read item j's operands only) and the padding columns of a group are
// zeros; the slabs are cut by proj_slab_rows(N) whatever the batch; a slab's sum runs over its rows in order, four per instruction
// (fused inside the matrix instruction, not separately rounded), and the slabs' sums are added in slab order from 0.0.  No floating-point atomics.
#include "icp_kernels.hpp"
#include "icp_search.hpp"
#include "icp_dense.hpp"

#include <algorithm>

namespace icp {

namespace {

constexpr int kProjResBlock = 128;
constexpr int kProjTiles = 4;     // 16-column tiles of the basis a wave owns (64 columns: 512 contiguous bytes of a basis row)
constexpr int kProjSteps = 4;     // matrix instructions' worth of rows (4 each) whose loads are in flight together
constexpr int kProjSolveBlock = 256;

// P1.  Items past n (the padding of the chunk's last group) get zeros.
__global__ void __launch_bounds__(kProjResBlock) k_proj_residual(const ProjItem* __restrict__ items, int n, int N,
                                                                 const double* __restrict__ ref, const double* __restrict__ mean,
                                                                 double* __restrict__ D, int* __restrict__ nonfinite) {
  const int slot = blockIdx.y;
  const int i = blockIdx.x * kProjResBlock + threadIdx.x;
  if (i >= N) return;
  const global_ptr<double> d = as_global(D) + ((size_t)(slot >> 4) * 3 * N + (size_t)3 * i) * kProjGroup + (slot & 15);
  if (slot >= n) {
    d[0] = 0.0; d[kProjGroup] = 0.0; d[2 * kProjGroup] = 0.0;
    return;
  }
  const ProjItem& it = items[slot];
  const global_ptr<const double> x = as_global(it.x) + (size_t)3 * i;
  double b0 = x[0], b1 = x[1], b2 = x[2];
  if (!(isfinite(b0) && isfinite(b1) && isfinite(b2))) atomicAdd(nonfinite + slot, 1);
  if (it.has_pose) {  // inverse RIGID pose (write_corr, icp_dense.hpp): Rᵀ((p − t) − ctr) + ctr
    const Pose& pose = it.pose;
    const double v0 = (b0 - pose.t[0]) - pose.ctr[0], v1 = (b1 - pose.t[1]) - pose.ctr[1], v2 = (b2 - pose.t[2]) - pose.ctr[2];
    b0 = ((pose.R[0] * v0 + pose.R[3] * v1) + pose.R[6] * v2) + pose.ctr[0];
    b1 = ((pose.R[1] * v0 + pose.R[4] * v1) + pose.R[7] * v2) + pose.ctr[1];
    b2 = ((pose.R[2] * v0 + pose.R[5] * v1) + pose.R[8] * v2) + pose.ctr[2];
  }
  d[0] = (b0 - ref[3 * i]) - mean[3 * i];
  d[kProjGroup] = (b1 - ref[3 * i + 1]) - mean[3 * i + 1];
  d[2 * kProjGroup] = (b2 - ref[3 * i + 2]) - mean[3 * i + 2];
}

// P2.  One wave; blockIdx = (block of kProjTiles tiles, slab, group).  v_mfma_f64_16x16x4_f64, operand maps as regression_tile
// (icp_dense.hpp) and cdna_hip_programming.md §3: lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15], result register g of
// lane l is D[row = (l>>4) + 4g][col = l&15].  Here i = basis column, k = row of the basis (3·vertex + coordinate), j = item:
// A = Q[row][column] from the row-major basis (a quarter wave reads 128 contiguous bytes of one row), B = D[group][row][item] (the
// wave reads 512 contiguous bytes).  Rows past the slab and columns past the rank supply zeros.
__global__ void __launch_bounds__(64) k_proj_gemm(const double* __restrict__ Q, int R, int r, int slab_rows, int rpad,
                                                  const double* __restrict__ D, double* __restrict__ part) {
  const int l = threadIdx.x, c16 = l & 15, kk = l >> 4;
  const int j0 = blockIdx.x * 16 * kProjTiles, slab = blockIdx.y, grp = blockIdx.z, n_slabs = gridDim.y;
  const int tn = min(kProjTiles, (r - j0 + 15) >> 4);  // (uniform) tiles of this block that hold a basis column
  int col[kProjTiles];
  bool on[kProjTiles];
#pragma unroll
  for (int t = 0; t < kProjTiles; ++t) {
    const int c = j0 + 16 * t + c16;
    on[t] = c < r;
    col[t] = on[t] ? c : 0;
  }
  const global_ptr<const double> q = as_global(Q);
  const global_ptr<const double> dg = as_global(D) + (size_t)grp * R * kProjGroup + c16;
  const int k0 = slab * slab_rows, k1 = min(R, k0 + slab_rows);
  d4_t acc[kProjTiles];
#pragma unroll
  for (int t = 0; t < kProjTiles; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int k = k0; k < k1; k += 4 * kProjSteps) {
    double a[kProjSteps][kProjTiles], b[kProjSteps];
    bool ok[kProjSteps];
#pragma unroll
    for (int u = 0; u < kProjSteps; ++u) {
      const int row = k + 4 * u + kk;
      ok[u] = row < k1;
      const size_t rc = ok[u] ? row : k1 - 1;  // (past the slab: a repeated load, its value replaced by zero)
      b[u] = dg[rc * kProjGroup];
#pragma unroll
      for (int t = 0; t < kProjTiles; ++t) a[u][t] = q[rc * r + col[t]];
    }
    __builtin_amdgcn_sched_barrier(0);  // (all loads requested before the first product)
#pragma unroll
    for (int u = 0; u < kProjSteps; ++u) {
      if (k + 4 * u < k1) {
        const double bu = ok[u] ? b[u] : 0.0;
#pragma unroll
        for (int t = 0; t < kProjTiles; ++t)
          if (t < tn) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ok[u] && on[t] ? a[u][t] : 0.0, bu, acc[t], 0, 0, 0);
      }
    }
  }
  const global_ptr<double> out = as_global(part) + ((size_t)grp * n_slabs + slab) * rpad * kProjGroup + c16;
#pragma unroll
  for (int t = 0; t < kProjTiles; ++t) {
    if (t >= tn) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = j0 + 16 * t + kk + 4 * g;  // (< rpad: tile t holds a column below the rank)
      out[(size_t)j * kProjGroup] = acc[t][g];
    }
  }
}

// P3.  blockIdx.x = item of the chunk.  b_j = Σ_slabs in slab order from 0.0; c_i = Σ_j P[i][j]·b_j in column order from 0.0, every
// product and sum rounded separately.  c goes to the call's coefficient rows: what the host copies out and what the instance pass of
// `project` reads.
__global__ void __launch_bounds__(kProjSolveBlock) k_proj_solve(int r, int rpad, int n_slabs, const double* __restrict__ part,
                                                                const double* __restrict__ P, double* __restrict__ coeffs) {
  __shared__ double s_b[512];
  const int slot = blockIdx.x, tid = threadIdx.x;
  const global_ptr<const double> pt = as_global(part) + (size_t)(slot >> 4) * n_slabs * rpad * kProjGroup + (slot & 15);
  for (int j = tid; j < r; j += kProjSolveBlock) {
    double s = 0.0;
    for (int sl = 0; sl < n_slabs; ++sl) s = s + pt[((size_t)sl * rpad + j) * kProjGroup];
    s_b[j] = s;
  }
  __syncthreads();
  const global_ptr<const double> p = as_global(P);
  const global_ptr<double> c = as_global(coeffs) + (size_t)slot * r;
  for (int i = tid; i < r; i += kProjSolveBlock) {
    const global_ptr<const double> row = p + (size_t)i * r;
    double acc = 0.0;
    int j = 0;
    for (; j + 8 <= r; j += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = row[j + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = acc + v[u] * s_b[j + u];
    }
    for (; j < r; ++j) acc = acc + row[j] * s_b[j];
    c[i] = acc;
  }
}

}  // namespace

int proj_slab_rows(int N) {
  const int rows = 3 * (N > 0 ? N : 1);
  const int s = std::max(kProjMinSlabRows, cdiv(rows, kProjMaxSlabs));
  return cdiv(s, 16) * 16;
}
int proj_slabs(int N) { return cdiv(3 * (N > 0 ? N : 1), proj_slab_rows(N)); }

void launch_proj_residual(hipStream_t st, int n, int N, const double* ref, const double* mean, const ProjItem* items, double* D,
                          int* nonfinite) {
  if (n <= 0) return;
  const int padded = cdiv(n, kProjGroup) * kProjGroup;
  hipLaunchKernelGGL(k_proj_residual, dim3(cdiv(N, kProjResBlock), padded), dim3(kProjResBlock), 0, st, items, n, N, ref, mean, D, nonfinite);
}
void launch_proj_gemm(hipStream_t st, int n, int N, int r, const double* Q, const double* D, double* part) {
  if (n <= 0) return;
  const int rpad = cdiv(r, 16) * 16;
  hipLaunchKernelGGL(k_proj_gemm, dim3(cdiv(r, 16 * kProjTiles), proj_slabs(N), cdiv(n, kProjGroup)), dim3(64), 0, st, Q, 3 * N, r,
                     proj_slab_rows(N), rpad, D, part);
}
void launch_proj_solve(hipStream_t st, int n, int N, int r, const double* part, const double* P, double* coeffs) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_proj_solve, dim3(n), dim3(kProjSolveBlock), 0, st, r, cdiv(r, 16) * 16, proj_slabs(N), part, P, coeffs);
}

}  // namespace icp
