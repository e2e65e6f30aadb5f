// kernels_pca_model.hip — PCA shape models from meshes in correspondence, many side by side (icp_pca_models_many): generalised
// Procrustes alignment, the centring, and the rank rule of a Gram matrix that is singular by construction.  What Scalismo's
// DataCollection.gpa and StatisticalMeshModel.createUsingPCA make; the alignment rules are this project's restatement.
// The centred columns ARE the factor L ([n][3N], one mesh per column) of the m-space half of kernels_gp_model.hip, which makes the model.
//
//   PC0 k_pca_init       working copies X[j] = the pool's mesh j; the first mean shape Σ_j X[j] / n (j = 0, 1, … in order); identity
//                        transforms
//   one round, for every item that has not stopped (blockIdx.z = item; a stopped item returns from every launch):
//   PC1 k_pca_centroids  every workgroup reduces the previous round's displacement partials itself and decides whether the item has
//                        stopped; otherwise its 256 vertices' coordinate sums, of every mesh and of the mean shape
//   PC2 k_pca_cross      every workgroup reduces the centroid partials of its mesh and of the mean shape itself, then its 256 vertices'
//                        part of Σ (x − c_x)(y − c_y)ᵀ: two passes, not Σ x yᵀ − N c_x c_yᵀ
//   PC3 k_pca_apply      every workgroup reduces centroids and cross-covariance itself, ONE thread solves Horn's 4 × 4 eigenproblem by
//                        cyclic Jacobi (the same bits in every workgroup), and the 256 vertices become R·(x − c_x) + c_y; workgroup 0
//                        composes the mesh's transform
//   PC4 k_pca_mean       the new mean shape, and its 256 rows' part of Σ (new − old)²
//   PC5 k_pca_centre     X[j] ← (X[j] − mean) / √(n−1) in place; partials of Σ column² = trace(G) and of Σ x²; rounds run and the last RMS
//   PC6 k_pca_rank       between the refinement and the operand of the m-space half: re = min(rank, #{θ_j > τ})
//
// An item's bits depend on nothing but the item: a workgroup owns kPcaBlock vertices (or rows) whatever shares the launch, its partial
// is a fixed tree over its threads, partials are reduced as k_gpm_pivot_step reduces them (thread t over partials t, t + 256, … in
// order, then the same tree), a mean is summed over the meshes in order.  No floating-point atomics, no device-side waits, no launch
// per reduction.  Loads are coalesced 8-byte ones through LDS: a column of X starts at 8·3N·j bytes, which is 16-byte aligned for
// every j only when N is even, so 16-byte loads would need a second code path and bits would still have to agree.
#include "icp_kernels.hpp"
#include "icp_dense.hpp"

#include <algorithm>

namespace icp {

namespace {

// the workgroup's sums of its 256 threads' K values, in every thread; a fixed tree.  s: [K][kPcaBlock] LDS
template <int K>
__device__ __forceinline__ void pca_block_sum(double (&v)[K], double* s) {
  const int t = threadIdx.x;
  __syncthreads();  // (the array may still be read from an earlier reduction)
#pragma unroll
  for (int k = 0; k < K; ++k) s[k * kPcaBlock + t] = v[k];
  __syncthreads();
  for (int o = kPcaBlock / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int k = 0; k < K; ++k) s[k * kPcaBlock + t] = s[k * kPcaBlock + t] + s[k * kPcaBlock + t + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = s[k * kPcaBlock];
}

// the sums of K rows of partials, part[k][0 .. cnt-1], in every thread: thread t over partials t, t + 256, … in order, then the tree
template <int K>
__device__ __forceinline__ void pca_reduce_partials(const double* part, int cnt, double (&v)[K], double* s) {
  const global_ptr<const double> p = as_global(part);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double a = 0.0;
    for (int b = threadIdx.x; b < cnt; b += kPcaBlock) a = a + p[(size_t)k * cnt + b];
    v[k] = a;
  }
  pca_block_sum<K>(v, s);
}

// the workgroup's 3·cnt doubles from `src` (the rows of vertices v0 .. v0+cnt-1) into LDS, a wave's loads next to each other
__device__ __forceinline__ void pca_stage(const double* src, int cnt, double* sx) {
  const global_ptr<const double> p = as_global(src);
  for (int k = threadIdx.x; k < 3 * cnt; k += kPcaBlock) sx[k] = p[k];
}

// RMS displacement of the mean shape in the last round run, from its partials
__device__ __forceinline__ double pca_rms(const PcaItem& it, double* s) {
  double d[1];
  pca_reduce_partials<1>(it.dpart, it.nblkR, d, s);
  return sqrt(d[0] / (double)it.N);
}

// Horn's unit quaternion (J. Opt. Soc. Am. A 4, 1987): the rotation that takes the centred x onto the centred y in the least-squares
// sense, from S[3a + b] = Σ x_a·y_b.  The eigenvector of the largest eigenvalue of the symmetric 4 × 4 matrix below, by cyclic Jacobi
// sweeps in plain f64; a rotation is skipped once its off-diagonal entry is below 2⁻⁶⁴ of the matrix.  Always a proper rotation; q and
// −q give the same R.  S = 0 (one vertex, or all vertices equal) gives the identity.  Every index is a constant after unrolling.
__device__ void pca_horn(const double* S, double* Rm) {
  double A[4][4], V[4][4];
  A[0][0] = (S[0] + S[4]) + S[8];
  A[0][1] = S[5] - S[7]; A[0][2] = S[6] - S[2]; A[0][3] = S[1] - S[3];
  A[1][1] = (S[0] - S[4]) - S[8];
  A[1][2] = S[1] + S[3]; A[1][3] = S[6] + S[2];
  A[2][2] = (S[4] - S[0]) - S[8];
  A[2][3] = S[5] + S[7];
  A[3][3] = (S[8] - S[0]) - S[4];
  double norm = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < i) A[i][j] = A[j][i];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) norm = norm + fabs(A[i][j]);
  const double small = 0x1p-64 * norm;
  for (int sweep = 0; sweep < 32; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (fabs(apq) > small) {
          rotated = true;
          const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
          const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // columns p, q
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = c * akp - s * akq;
            A[k][q] = s * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // rows p, q
            const double apk = A[p][k], aqk = A[q][k];
            A[p][k] = c * apk - s * aqk;
            A[q][k] = s * apk + c * aqk;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - s * vkq;
            V[k][q] = s * vkp + c * vkq;
          }
        }
      }
    if (!rotated) break;
  }
  double best = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (A[j][j] > best) { best = A[j][j]; q0 = V[0][j]; q1 = V[1][j]; q2 = V[2][j]; q3 = V[3][j]; }
  const double nrm = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
  q0 = q0 / nrm; q1 = q1 / nrm; q2 = q2 / nrm; q3 = q3 / nrm;
  Rm[0] = ((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3;
  Rm[1] = 2.0 * (q1 * q2 - q0 * q3);
  Rm[2] = 2.0 * (q1 * q3 + q0 * q2);
  Rm[3] = 2.0 * (q1 * q2 + q0 * q3);
  Rm[4] = ((q0 * q0 - q1 * q1) + q2 * q2) - q3 * q3;
  Rm[5] = 2.0 * (q2 * q3 - q0 * q1);
  Rm[6] = 2.0 * (q1 * q3 - q0 * q2);
  Rm[7] = 2.0 * (q2 * q3 + q0 * q1);
  Rm[8] = ((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3;
}

// PC0.  blockIdx = (block of rows, item).
__global__ void __launch_bounds__(kPcaBlock) k_pca_init(const PcaItem* __restrict__ items) {
  const PcaItem& it = items[blockIdx.y];
  if ((int)blockIdx.x >= it.nblkR) return;
  const int t = threadIdx.x, e = blockIdx.x * kPcaBlock + t, R = it.R, n = it.n;
  if (blockIdx.x == 0)
    for (int k = t; k < 12 * n; k += kPcaBlock) {
      const int c = k % 12;
      it.tf[k] = c == 0 || c == 4 || c == 8 ? 1.0 : 0.0;
    }
  if (e >= R) return;
  double s = 0.0;
  for (int j = 0; j < n; ++j) {
    const double v = as_global(it.src[j])[e];
    it.X[(size_t)j * R + e] = v;
    s = s + v;
  }
  it.mean[e] = s / (double)n;
}

// has the item stopped before `round`?  PC2 .. PC4: the cap, or the flag PC1 of this round or an earlier one has set
__device__ __forceinline__ bool pca_stopped(const PcaItem& it, int round) { return round >= it.max_rounds || it.stop[0] != 0; }

// PC1.  blockIdx = (block of vertices, mesh 0 .. n with n = the mean shape, item).
__global__ void __launch_bounds__(kPcaBlock) k_pca_centroids(const PcaItem* __restrict__ items, int round) {
  __shared__ double sr[3 * kPcaBlock], sx[3 * kPcaBlock];
  const PcaItem& it = items[blockIdx.z];
  const int mesh = blockIdx.y, blk = blockIdx.x, t = threadIdx.x;
  if (blk >= it.nblk || mesh > it.n || round >= it.max_rounds) return;
  // the halt test behind the previous round: the same partials, the same order, the same bits in every workgroup and in every later
  // round (a stopped item's partials are never written again)
  if (round > 0 && pca_rms(it, sr) < it.halt) {
    if (blk == 0 && mesh == 0 && t == 0) it.stop[0] = 1;
    return;
  }
  const int v0 = blk * kPcaBlock, cnt = min(kPcaBlock, it.N - v0);
  const double* src = mesh < it.n ? it.X + (size_t)mesh * it.R : it.mean;
  __syncthreads();
  pca_stage(src + 3 * (size_t)v0, cnt, sx);
  __syncthreads();
  double v[3] = {0.0, 0.0, 0.0};
  if (t < cnt) { v[0] = sx[3 * t]; v[1] = sx[3 * t + 1]; v[2] = sx[3 * t + 2]; }
  pca_block_sum<3>(v, sr);
  if (t == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) it.cpart[((size_t)mesh * 3 + k) * it.nblk + blk] = v[k];
}

// PC2.  blockIdx = (block of vertices, mesh, item).
__global__ void __launch_bounds__(kPcaBlock) k_pca_cross(const PcaItem* __restrict__ items, int round) {
  __shared__ double sr[9 * kPcaBlock], sx[3 * kPcaBlock], sy[3 * kPcaBlock];
  const PcaItem& it = items[blockIdx.z];
  const int mesh = blockIdx.y, blk = blockIdx.x, t = threadIdx.x;
  if (blk >= it.nblk || mesh >= it.n || pca_stopped(it, round)) return;
  double cx[3], cy[3];
  pca_reduce_partials<3>(it.cpart + (size_t)mesh * 3 * it.nblk, it.nblk, cx, sr);
  pca_reduce_partials<3>(it.cpart + (size_t)it.n * 3 * it.nblk, it.nblk, cy, sr);
#pragma unroll
  for (int k = 0; k < 3; ++k) { cx[k] = cx[k] / (double)it.N; cy[k] = cy[k] / (double)it.N; }
  const int v0 = blk * kPcaBlock, cnt = min(kPcaBlock, it.N - v0);
  pca_stage(it.X + (size_t)mesh * it.R + 3 * (size_t)v0, cnt, sx);
  pca_stage(it.mean + 3 * (size_t)v0, cnt, sy);
  __syncthreads();
  double h[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = 0.0;
  if (t < cnt) {
    double x[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[k] = sx[3 * t + k] - cx[k]; y[k] = sy[3 * t + k] - cy[k]; }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) h[3 * a + b] = x[a] * y[b];
  }
  pca_block_sum<9>(h, sr);
  if (t == 0)
#pragma unroll
    for (int k = 0; k < 9; ++k) it.hpart[((size_t)mesh * 9 + k) * it.nblk + blk] = h[k];
}

// PC3.  blockIdx = (block of vertices, mesh, item).
__global__ void __launch_bounds__(kPcaBlock) k_pca_apply(const PcaItem* __restrict__ items, int round) {
  __shared__ double sr[9 * kPcaBlock], sx[3 * kPcaBlock], rot[9];
  const PcaItem& it = items[blockIdx.z];
  const int mesh = blockIdx.y, blk = blockIdx.x, t = threadIdx.x;
  if (blk >= it.nblk || mesh >= it.n || pca_stopped(it, round)) return;
  double cx[3], cy[3], h[9];
  pca_reduce_partials<3>(it.cpart + (size_t)mesh * 3 * it.nblk, it.nblk, cx, sr);
  pca_reduce_partials<3>(it.cpart + (size_t)it.n * 3 * it.nblk, it.nblk, cy, sr);
  pca_reduce_partials<9>(it.hpart + (size_t)mesh * 9 * it.nblk, it.nblk, h, sr);
#pragma unroll
  for (int k = 0; k < 3; ++k) { cx[k] = cx[k] / (double)it.N; cy[k] = cy[k] / (double)it.N; }
  if (t == 0) {
    double Rm[9];
    pca_horn(h, Rm);
#pragma unroll
    for (int k = 0; k < 9; ++k) rot[k] = Rm[k];
  }
  const int v0 = blk * kPcaBlock, cnt = min(kPcaBlock, it.N - v0);
  double* X = it.X + (size_t)mesh * it.R + 3 * (size_t)v0;
  pca_stage(X, cnt, sx);
  __syncthreads();
  double Rm[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rm[k] = rot[k];
  if (t < cnt) {
    const double u0 = sx[3 * t] - cx[0], u1 = sx[3 * t + 1] - cx[1], u2 = sx[3 * t + 2] - cx[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) sx[3 * t + a] = ((Rm[3 * a] * u0 + Rm[3 * a + 1] * u1) + Rm[3 * a + 2] * u2) + cy[a];
  }
  __syncthreads();
  for (int k = t; k < 3 * cnt; k += kPcaBlock) X[k] = sx[k];
  if (blk == 0 && t == 0) {  // the composite: R ← R_k·R, t ← R_k·t + t_k with t_k = c_y − R_k·c_x
    double* tf = it.tf + 12 * (size_t)mesh;
    double old[12], tk[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) old[k] = tf[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) tk[a] = cy[a] - ((Rm[3 * a] * cx[0] + Rm[3 * a + 1] * cx[1]) + Rm[3 * a + 2] * cx[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) tf[3 * a + b] = (Rm[3 * a] * old[b] + Rm[3 * a + 1] * old[3 + b]) + Rm[3 * a + 2] * old[6 + b];
      tf[9 + a] = ((Rm[3 * a] * old[9] + Rm[3 * a + 1] * old[10]) + Rm[3 * a + 2] * old[11]) + tk[a];
    }
  }
}

// PC4.  blockIdx = (block of rows, item).
__global__ void __launch_bounds__(kPcaBlock) k_pca_mean(const PcaItem* __restrict__ items, int round) {
  __shared__ double sr[kPcaBlock];
  const PcaItem& it = items[blockIdx.y];
  if ((int)blockIdx.x >= it.nblkR || pca_stopped(it, round)) return;
  const int t = threadIdx.x, e = blockIdx.x * kPcaBlock + t, R = it.R, n = it.n;
  double d[1] = {0.0};
  if (e < R) {
    const global_ptr<const double> X = as_global((const double*)it.X) + e;
    double s = 0.0;
    for (int j = 0; j < n; ++j) s = s + X[(size_t)j * R];
    const double m = s / (double)n, diff = m - it.mean[e];
    it.mean[e] = m;
    d[0] = diff * diff;
  }
  pca_block_sum<1>(d, sr);
  if (t == 0) {
    it.dpart[blockIdx.x] = d[0];
    if (blockIdx.x == 0) it.state[0] = (double)(round + 1);
  }
}

// PC5.  blockIdx = (block of rows, item).  Every item, stopped or not.
__global__ void __launch_bounds__(kPcaBlock) k_pca_centre(const PcaItem* __restrict__ items) {
  __shared__ double sr[2 * kPcaBlock];
  const PcaItem& it = items[blockIdx.y];
  if ((int)blockIdx.x >= it.nblkR) return;
  const int t = threadIdx.x, e = blockIdx.x * kPcaBlock + t, R = it.R, n = it.n;
  if (blockIdx.x == 0) {  // (uniform over the workgroup)
    const double rms = pca_rms(it, sr);
    if (t == 0) it.state[1] = it.state[0] > 0.0 ? rms : 0.0;
  }
  double v[2] = {0.0, 0.0};
  if (e < R) {
    const double m = it.mean[e], sq = sqrt((double)(n - 1));
    for (int j = 0; j < n; ++j) {
      const double x = it.X[(size_t)j * R + e];
      const double c = (x - m) / sq;
      it.X[(size_t)j * R + e] = c;
      v[0] = v[0] + c * c;
      v[1] = v[1] + x * x;
    }
  }
  pca_block_sum<2>(v, sr);
  if (t == 0) { it.tpart[blockIdx.x] = v[0]; it.tpart[it.nblkR + blockIdx.x] = v[1]; }
}

// PC6.  blockIdx = item; thread j looks at eigenvalue j (me <= kGpmMaxPivots = the workgroup).  A count does not depend on an order.
__global__ void __launch_bounds__(kGpmMaxPivots) k_pca_rank(GpmSpace* __restrict__ items) {
  __shared__ int cnt[kGpmMaxPivots];
  GpmSpace& it = items[blockIdx.x];
  const int t = threadIdx.x;
  cnt[t] = t < it.me && it.lam[t] / it.scale > it.tau ? 1 : 0;
  __syncthreads();
  for (int o = kGpmMaxPivots / 2; o > 0; o >>= 1) {
    if (t < o) cnt[t] += cnt[t + o];
    __syncthreads();
  }
  if (t == 0) it.re = min(it.rank, cnt[0]);
}

}  // namespace

void launch_pca_init(hipStream_t st, int n_items, int nblkR_max, const PcaItem* items) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(k_pca_init, dim3(nblkR_max, n_items), dim3(kPcaBlock), 0, st, items);
}
void launch_pca_round(hipStream_t st, int n_items, int n_max, int nblk_max, int nblkR_max, int round, const PcaItem* items) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(k_pca_centroids, dim3(nblk_max, n_max + 1, n_items), dim3(kPcaBlock), 0, st, items, round);
  hipLaunchKernelGGL(k_pca_cross, dim3(nblk_max, n_max, n_items), dim3(kPcaBlock), 0, st, items, round);
  hipLaunchKernelGGL(k_pca_apply, dim3(nblk_max, n_max, n_items), dim3(kPcaBlock), 0, st, items, round);
  hipLaunchKernelGGL(k_pca_mean, dim3(nblkR_max, n_items), dim3(kPcaBlock), 0, st, items, round);
}
void launch_pca_centre(hipStream_t st, int n_items, int nblkR_max, const PcaItem* items) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(k_pca_centre, dim3(nblkR_max, n_items), dim3(kPcaBlock), 0, st, items);
}
void launch_pca_rank(hipStream_t st, int n, GpmSpace* items) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_pca_rank, dim3(n), dim3(kGpmMaxPivots), 0, st, items);
}

}  // namespace icp
