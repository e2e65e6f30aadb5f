// kernels_posterior_model.hip — posterior shape models from given correspondences, many side by side (icp_posterior_models_many;
// Scalismo's model.posterior(correspondences, noise) as api/other/IcpBasedSurfaceFitting.scala:81 and NonRigidIcpProposal.scala:152
// call it, and its discretisation as a model, NonRigidIcpProposal.scala:77).  SURVEY App. A.4:
//   M = I + Σ Q_iᵀ W_i Q_i,  b = Σ Q_iᵀ W_i (y_i − x̄_i − μ_i),  α = M⁻¹ b,  D M⁻¹ D = V S Vᵀ,  W_i = Σ_i⁻¹
// and the posterior model is (mean μ + Q·α, basis Φ·V, variances S).
//
//   PM1 k_pm_regression     the split-K partial sums of every item's normal equations on the f64 matrix cores: regression_tile's tiles,
//                           splits and partial layout (what launch_posterior_factor reads), with a full 3 × 3 precision W_i per
//                           observation where regression_tile has w_t·I + κ·n̂n̂ᵀ
//   PM2 k_pm_operand        Bm = [D⁻¹V | α], zero-padded to multiples of 16 both ways: the right operand of PM3 (Q = Φ·D is the basis
//                           the context keeps, so Φ·V = Q·D⁻¹V and the mean's Q·α is one more column)
//   PM3 k_pm_gemm           rows of Q·Bm on the f64 matrix cores into the chunk buffer: a wave owns 32 rows × 64 columns
//   PM4 k_pm_point_variance one wave per vertex over the rows PM3 has just written: Σ_d Σ_j S_j·(ΦV)[3i+d][j]²
// The factorisations and decompositions between PM1 and PM2 are the resident many-problem kernels (kernels_factor.hip, kernels_eigen.hip).
//
// An item's bits depend on nothing but the item.  PM1: an item's splits are regression_splits of its own observation count, a split's
// sum runs over its observations in order, one matrix instruction each.  PM3: an output element reads its own row of Q and its own
// column of Bm; the contraction runs over the basis columns in blocks of 16 from 0.0, four instructions per block, instruction u
// summing columns u, 4+u, 8+u, 12+u of the block (fused inside the instruction) — whatever rows share the wave, the piece or the chunk.
// PM4: lane l sums columns l, l+64, … in order, coordinate by coordinate, then the lanes' sums meet in a fixed butterfly.
// No floating-point atomics.
#include "icp_kernels.hpp"
#include "icp_dense.hpp"

#include <algorithm>

namespace icp {

namespace {

// PM1.  blockIdx = (split, tile, item).  Operand maps as regression_tile (icp_dense.hpp): lane l supplies A[i = l&15][k = l>>4] and
// B[k = l>>4][j = l&15]; here k = coordinate (k = 3: nothing), A = X_i = [Q_i | e_i], B = W_i·X_i.
__global__ void __launch_bounds__(64) k_pm_regression(const PmItem* __restrict__ items) {
  const PmItem& it = items[blockIdx.z];
  const int r = it.r, n = r + 1, S = it.splits, K = it.K;
  const int tile = blockIdx.y, split = blockIdx.x;
  if (split >= S || tile >= regression_tiles(r)) return;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  const int tj = tile - ti * (ti + 1) / 2;
  const int l = threadIdx.x & 63, i16 = l & 15, kk = l >> 4;
  const int a = 16 * ti + i16, b = 16 * tj + i16;
  const int ca = a < r ? a : 0, cb = b < r ? b : 0;
  const double ma = a < r ? 1.0 : 0.0, mb = b < r ? 1.0 : 0.0;   // basis column?
  const double ea = a == r ? 1.0 : 0.0, eb = b == r ? 1.0 : 0.0; // the appended observation column?
  const int kchunk = cdiv(K, S), k0 = split * kchunk, k1 = min(K, k0 + kchunk);
  const global_ptr<const double> Q = as_global(it.Q), ref = as_global(it.ref), mean = as_global(it.mean), pt = as_global(it.pt),
                                 W = as_global(it.W);
  const global_ptr<const int> ids = as_global(it.id);
  d4_t acc = {0.0, 0.0, 0.0, 0.0};
  for (int k = k0; k < k1; ++k) {
    const int id = ids[k];
    const global_ptr<const double> q = Q + (size_t)3 * id * r;
    const double e0 = (pt[3 * k] - ref[3 * id]) - mean[3 * id], e1 = (pt[3 * k + 1] - ref[3 * id + 1]) - mean[3 * id + 1],
                 e2 = (pt[3 * k + 2] - ref[3 * id + 2]) - mean[3 * id + 2];
    const double a0 = fma(ma, q[ca], ea * e0), a1 = fma(ma, q[r + ca], ea * e1), a2 = fma(ma, q[2 * r + ca], ea * e2);
    const double b0 = fma(mb, q[cb], eb * e0), b1 = fma(mb, q[r + cb], eb * e1), b2 = fma(mb, q[2 * r + cb], eb * e2);
    const global_ptr<const double> w = W + (size_t)6 * k;  // xx xy xz yy yz zz
    const double w0 = kk == 0 ? w[0] : kk == 1 ? w[1] : w[2], w1 = kk == 0 ? w[1] : kk == 1 ? w[3] : w[4],
                 w2 = kk == 0 ? w[2] : kk == 1 ? w[4] : w[5];
    const double A_op = kk == 0 ? a0 : kk == 1 ? a1 : kk == 2 ? a2 : 0.0;
    const double B_op = kk == 3 ? 0.0 : (w0 * b0 + w1 * b1) + w2 * b2;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A_op, B_op, acc, 0, 0, 0);
  }
  const global_ptr<double> out = as_global(it.Mpart) + (size_t)split * n * n;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int row = 16 * ti + kk + 4 * g, col = 16 * tj + i16;
    if (row < n && col < n) out[(size_t)row * n + col] = acc[g];
  }
}

// PM2.  blockIdx.y = item.  Bm[k][j] = V[k][j]/√λ_k for j < r, α_k for j = r, zero in the padding.
__global__ void __launch_bounds__(256) k_pm_operand(const PmItem* __restrict__ items) {
  const PmItem& it = items[blockIdx.y];
  const int r = it.r, ldb = it.ldb, rp = (r + 15) & ~15;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= rp * ldb) return;
  const int k = e / ldb, j = e - k * ldb;
  double v = 0.0;
  if (k < r) {
    if (j < r) v = it.V[(size_t)k * r + j] * it.inv_sqrt_lambda[k];
    else if (j == r) v = it.alpha[k];
  }
  it.Bm[e] = v;
}

// PM3.  One wave; blockIdx = (block of kPmColTiles column tiles, block of kPmRowTiles row tiles, piece).  v_mfma_f64_16x16x4_f64 with
// k_proj_gemm's operand maps: i = row of Q, j = column of Bm, result register g of lane l is out[row = (l>>4) + 4g][col = l&15].  Lane
// (i, kk) reads the four neighbouring basis columns 4·kk .. 4·kk+3 of its row for a block of 16 (a quarter wave: 128 contiguous bytes
// of a row) and supplies column 4·kk + u to instruction u.  Rows past the piece and columns past the rank supply zeros (a repeated,
// in-range load whose value is replaced).
constexpr int kPmRowTiles = 2, kPmColTiles = 4;
__global__ void __launch_bounds__(64) k_pm_gemm(const PmPiece* __restrict__ pieces) {
  const PmPiece& pc = pieces[blockIdx.z];
  const int r = pc.r, ldb = pc.ldb;
  const int t0 = pc.t0 + blockIdx.x * kPmColTiles, nt = ldb >> 4;
  const int row_a = blockIdx.y * 16 * kPmRowTiles;
  if (t0 >= nt || row_a >= pc.rows) return;
  const int tn = min(kPmColTiles, nt - t0);  // (uniform) column tiles of this block
  const int l = threadIdx.x, i16 = l & 15, kk = l >> 4;
  const global_ptr<const double> Bm = as_global(pc.Bm) + 16 * t0 + i16;
  global_ptr<const double> qrow[kPmRowTiles];
  bool rok[kPmRowTiles];
#pragma unroll
  for (int t = 0; t < kPmRowTiles; ++t) {
    const int row = row_a + 16 * t + i16;
    rok[t] = row < pc.rows;
    qrow[t] = as_global(pc.Q) + (size_t)(pc.row0 + (rok[t] ? row : pc.rows - 1)) * r;
  }
  d4_t acc[kPmRowTiles][kPmColTiles];
#pragma unroll
  for (int t = 0; t < kPmRowTiles; ++t)
#pragma unroll
    for (int c = 0; c < kPmColTiles; ++c) acc[t][c] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < r; k0 += 16) {
    double a[kPmRowTiles][4], b[4][kPmColTiles];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 4 * kk + u;
      const bool kok = k < r;
      const int kc = kok ? k : r - 1;
#pragma unroll
      for (int t = 0; t < kPmRowTiles; ++t) {
        const double v = qrow[t][kc];
        a[t][u] = kok && rok[t] ? v : 0.0;
      }
#pragma unroll
      for (int c = 0; c < kPmColTiles; ++c) b[u][c] = c < tn ? Bm[(size_t)k * ldb + 16 * c] : 0.0;  // (rows of Bm are padded to 16: in range)
    }
    __builtin_amdgcn_sched_barrier(0);  // (all loads requested before the first product)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < kPmRowTiles; ++t)
#pragma unroll
        for (int c = 0; c < kPmColTiles; ++c)
          if (c < tn) acc[t][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][u], b[u][c], acc[t][c], 0, 0, 0);
  }
  const global_ptr<double> basis = as_global(pc.basis), mean = as_global(pc.mean);
  const global_ptr<const double> mu = as_global(pc.mu);
#pragma unroll
  for (int t = 0; t < kPmRowTiles; ++t)
#pragma unroll
    for (int c = 0; c < kPmColTiles; ++c) {
      if (c >= tn) continue;
      const int col = 16 * (t0 + c) + i16;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = row_a + 16 * t + kk + 4 * g;
        if (row >= pc.rows) continue;
        if (col < r) {
          if (pc.basis) basis[(size_t)row * r + col] = acc[t][c][g];
        } else if (col == r && pc.mean) {
          mean[row] = mu[pc.row0 + row] + acc[t][c][g];  // μ + Q·α
        }
      }
    }
}

// PM4.  blockIdx = (block of 4 vertices, piece); one wave per vertex of the piece.
__global__ void __launch_bounds__(256) k_pm_point_variance(const PmPiece* __restrict__ pieces) {
  const PmPiece& pc = pieces[blockIdx.y];
  if (!pc.pvar) return;
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63, r = pc.r;
  if (3 * v >= pc.rows) return;  // (wave-uniform; a piece holds whole vertices)
  const global_ptr<const double> row = as_global((const double*)pc.basis) + (size_t)3 * v * r, S = as_global(pc.S);
  double s = 0.0;
  for (int d = 0; d < 3; ++d)
    for (int j = l; j < r; j += 64) {
      const double x = row[(size_t)d * r + j];
      s = s + S[j] * (x * x);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  if (l == 0) pc.pvar[v] = s;
}

}  // namespace

void launch_pm_regression(hipStream_t st, int n, int splits_max, int rmax, const PmItem* items) {
  if (n <= 0) return;
  ProfScope _ps(st, KID_REGRESSION);
  hipLaunchKernelGGL(k_pm_regression, dim3(splits_max, regression_tiles(rmax), n), dim3(64), 0, st, items);
}
void launch_pm_operand(hipStream_t st, int n, int rmax, const PmItem* items) {
  if (n <= 0) return;
  const int rp = cdiv(rmax, 16) * 16, ldb = cdiv(rmax + 1, 16) * 16;
  hipLaunchKernelGGL(k_pm_operand, dim3(cdiv(rp * ldb, 256), n), dim3(256), 0, st, items);
}
void launch_pm_gemm(hipStream_t st, int n_pieces, int rows_max, int col_tiles_max, const PmPiece* pieces) {
  if (n_pieces <= 0) return;
  hipLaunchKernelGGL(k_pm_gemm, dim3(cdiv(col_tiles_max, kPmColTiles), cdiv(rows_max, 16 * kPmRowTiles), n_pieces), dim3(64), 0, st, pieces);
}
void launch_pm_point_variance(hipStream_t st, int n_pieces, int rows_max, const PmPiece* pieces) {
  if (n_pieces <= 0) return;
  hipLaunchKernelGGL(k_pm_point_variance, dim3(cdiv(cdiv(rows_max, 3), 4), n_pieces), dim3(256), 0, st, pieces);
}

}  // namespace icp
