// kernels_gp_model.hip — Gaussian-process shape models from analytic kernels, many side by side (icp_gp_models_many; what
// apps/femur/CreateGPModel.scala and apps/bfm/CreateGPModel.scala make, by Scalismo's pivoted Cholesky route, approximateGPCholesky,
// instead of the Nyström one).  K = the 3N × 3N matrix of k(x, y) = Σ_t scale_t·exp(−‖x−y‖²/σ_t²)·A_t on the mesh's own points:
//   K ≈ L·Lᵀ with m columns, one per pivot;  LᵀL = W·Θ·Wᵀ;  variances Θ/N, basis √N·L·W·Θ^-1/2.
//
//   GP0 k_gpm_init        d = diag K; every workgroup's partial (max d, its row, Σ d); pivots = −1, columns made = 0
//   GP1 k_gpm_pivot_step  ONE launch per pivot step for all items (blockIdx.y = item): every workgroup reduces the previous launch's
//                         partials itself — a few hundred values, the same bits in every workgroup, so no workgroup waits for another
//                         and no launch sits between two steps —, decides whether the loop has stopped, and otherwise makes its
//                         256 rows of the new column: the kernel's value against the pivot row analytically, minus the product with
//                         the columns made so far, divided by √d[p]; d −= L²; its new partial.
//   GP2 k_gpm_gram        LᵀL on the f64 matrix cores, split over slabs of rows, lower 16 × 16 tiles
//   GP3 k_gpm_gram_sum    the slabs' sums in slab order, times the item's power of two, mirrored: an exactly symmetric m × m matrix
//   GP4a-d k_gpm_refine_* one refinement step on the decomposition's eigenvectors (they are good to 1e-11: enough for the chain's samples,
//                         not for a basis orthonormal to rounding), the refined eigenvalues, their descending order
//   GP4 k_gpm_operand     Op = W·Θ^-1/2·√N in descending θ, zero-padded to 16s; the variances
//   GP5 k_gpm_gemm        rows of L·Op on the f64 matrix cores into the chunk buffer: a wave owns 32 rows × 64 columns
// General terms (icp_gp_models_general_many, what apps/bfm/CreateGPModel.scala needs: cubic B-spline base kernels, per-vertex weights on
// both arguments, the mirror symmetrisation) run in the <true> instances of GP0 and GP1, which a call with at least one such item
// launches; there an item's flag — uniform over the workgroup — chooses between the plain expressions and gpm_general_value.  A call
// of plain items launches the <false> instances: the code as it is without general terms.  K's diagonal of a general item is the
// kernel's value of the row against itself.  k_gpm_region_weights (icp_region_weights_many) makes FaceMask's smoothed region weights.
// The decomposition between GP3 and GP4a is the chain's (kernels_eigen.hip) with sqrt_lambda ≡ 1; only its eigenvectors are used.
//
// Layout of L: column by column ([m][3N]).  GP1 reads one value per row and column made so far, a wave's 64 rows next to each other
// (512 contiguous bytes per load), and the pivot's row of L once per workgroup into LDS; GP2 and GP5 read runs of 16 rows per column.
//
// An item's bits depend on nothing but the item.  GP0/GP1: a workgroup owns kGpmBlockRows rows whatever shares the launch; its
// partial is a fixed tree over its rows; the reduction of the partials is thread t over partials t, t + 256, … in order, then the same
// tree; the maximum is the lexicographic one of (value, −row), so ties go to the lowest row whatever the grid.  A row's product with the
// columns made so far is summed in column order, one product and one addition at a time.  GP2: a slab is gpm_slab_rows(3N) rows, summed 16
// rows at a time in order (four instructions, instruction u taking rows 4·kk + u of the 16); GP3 adds the slabs in order.  GP5 as
// k_pm_gemm: the contraction runs over the columns of L in blocks of 16 from 0.0, whatever rows share the wave, the piece or the chunk.
// No floating-point atomics anywhere.
#include "icp_kernels.hpp"
#include "icp_dense.hpp"
#include "icp_gp_terms.hpp"

#include <algorithm>
#include <climits>

namespace icp {

namespace {

struct GpmBest { double v; int i; double s; };  // max d, its row, Σ d

__device__ __forceinline__ void gpm_fold(GpmBest& a, double v, int i, double s) {
  if (v > a.v || (v == a.v && i < a.i)) { a.v = v; a.i = i; }
  a.s = a.s + s;
}

// the workgroup's (max, row, sum) of its 256 threads' values, in every thread; a fixed tree
__device__ __forceinline__ GpmBest gpm_block_reduce(GpmBest x, double* sv, double* ss, int* si) {
  const int t = threadIdx.x;
  __syncthreads();  // (the arrays may still be read from an earlier reduction)
  sv[t] = x.v; ss[t] = x.s; si[t] = x.i;
  __syncthreads();
  for (int o = kGpmBlockRows / 2; o > 0; o >>= 1) {
    if (t < o) {
      const double v = sv[t + o];
      const int i = si[t + o];
      if (v > sv[t] || (v == sv[t] && i < si[t])) { sv[t] = v; si[t] = i; }
      ss[t] = ss[t] + ss[t + o];
    }
    __syncthreads();
  }
  return GpmBest{sv[0], si[0], ss[0]};
}

// K[row][p] for row = 3·vertex + c against the pivot's point xp and coordinate cp, the terms summed in order
__device__ __forceinline__ double gpm_kernel_value(const GpmItem& it, double x0, double x1, double x2, int c, double p0, double p1, double p2,
                                                   int cp) {
  const double dx = x0 - p0, dy = x1 - p1, dz = x2 - p2;
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  double acc = 0.0;
  for (int t = 0; t < it.n_terms; ++t) {
    const GpmTerm& tm = it.terms[t];
    acc = acc + (tm.scale * exp(-(d2 / tm.sigma2))) * tm.A[3 * c + cp];
  }
  return acc;
}

// ---- general terms (icp_gp_models_general_many): B-spline, weighted, mirrored; the scalar base kernels are icp_gp_terms.hpp's.
// K[3·v + c][3·vp + cp] of a general item, the terms summed in order: ((scale·(w(v)·w(vp)))·(b(x, p) + (γ·s_c)·b(x, p̄)))·A[c][cp].
// A plain term among them has gpm_kernel_value's bits (scale·1 = scale, b + 0·b̄ = b).  `pv` is the pivot as GP1 stages it, uniform
// over the workgroup: the point p [0..2], term t's mirrored point [3 + 3t ..], term t's weight of the pivot's vertex [kGpmPivotW + t].
constexpr int kGpmPivotW = 3 + 3 * kGpmMaxTerms, kGpmPivotDoubles = kGpmPivotW + kGpmMaxTerms;
__device__ __forceinline__ double gpm_general_value(const GpmItem& it, int v, double x0, double x1, double x2, int c, const double* pv, int cp) {
  double acc = 0.0;
  for (int t = 0; t < it.n_terms; ++t) {
    const GpmTerm& tm = it.terms[t];
    const double a = tm.A[3 * c + cp];
    double ww = 1.0;
    if (tm.w) ww = as_global(tm.w)[v] * pv[kGpmPivotW + t];
    double val = gpm_base(tm, x0, x1, x2, pv[0], pv[1], pv[2]);
    if (tm.gain > 0.0) {
      const double sgn = c == tm.axis ? -1.0 : 1.0;
      const double bm = gpm_base(tm, x0, x1, x2, pv[3 + 3 * t], pv[4 + 3 * t], pv[5 + 3 * t]);
      val = val + (tm.gain * sgn) * bm;
    }
    acc = acc + ((tm.scale * ww) * val) * a;
  }
  return acc;
}
// the pivot of a general item into `pv` (LDS), by the workgroup's first kGpmPivotDoubles threads; vp = the pivot's vertex
__device__ __forceinline__ void gpm_stage_pivot(const GpmItem& it, int vp, double* pv) {
  const int t = threadIdx.x;
  const global_ptr<const double> pts = as_global(it.pts);
  if (t < 3) {
    pv[t] = pts[3 * vp + t];
  } else if (t < kGpmPivotW) {
    const int k = (t - 3) / 3, a = (t - 3) - 3 * k;
    const double x = pts[3 * vp + a];
    pv[t] = k < it.n_terms && a == it.terms[k].axis ? -x : x;
  } else if (t < kGpmPivotDoubles) {
    const int k = t - kGpmPivotW;
    pv[t] = k < it.n_terms && it.terms[k].w ? as_global(it.terms[k].w)[vp] : 1.0;
  }
}
// d[3·v + c] of a general item: gpm_general_value's expression of the row against itself
__device__ __forceinline__ double gpm_general_diagonal(const GpmItem& it, int v, double x0, double x1, double x2, int c) {
  double acc = 0.0;
  for (int t = 0; t < it.n_terms; ++t) {
    const GpmTerm& tm = it.terms[t];
    double ww = 1.0;
    if (tm.w) ww = as_global(tm.w)[v] * as_global(tm.w)[v];
    double val = gpm_base(tm, x0, x1, x2, x0, x1, x2);
    if (tm.gain > 0.0) {
      const double sgn = c == tm.axis ? -1.0 : 1.0;
      const double bm = gpm_base(tm, x0, x1, x2, tm.axis == 0 ? -x0 : x0, tm.axis == 1 ? -x1 : x1, tm.axis == 2 ? -x2 : x2);
      val = val + (tm.gain * sgn) * bm;
    }
    acc = acc + ((tm.scale * ww) * val) * tm.A[4 * c];
  }
  return acc;
}

// GP0.  blockIdx = (block of rows, item).
template <bool kGeneral>
__global__ void __launch_bounds__(kGpmBlockRows) k_gpm_init(const GpmItem* __restrict__ items) {
  __shared__ double sv[kGpmBlockRows], ss[kGpmBlockRows];
  __shared__ int si[kGpmBlockRows];
  const GpmItem& it = items[blockIdx.y];
  if ((int)blockIdx.x >= it.nblk) return;
  const int t = threadIdx.x, row = blockIdx.x * kGpmBlockRows + t;
  GpmBest x{-INFINITY, INT_MAX, 0.0};
  if (row < it.R) {
    const int c = row % 3;
    double acc = 0.0;
    if (kGeneral && it.general) {  // (uniform over the workgroup) the kernel's value of the row against itself
      const int v = row / 3;
      const global_ptr<const double> pts = as_global(it.pts);
      const double x0 = pts[3 * v], x1 = pts[3 * v + 1], x2 = pts[3 * v + 2];
      acc = gpm_general_diagonal(it, v, x0, x1, x2, c);
    } else {
      for (int k = 0; k < it.n_terms; ++k) acc = acc + it.terms[k].scale * it.terms[k].A[4 * c];
    }
    it.d[row] = acc;
    x = GpmBest{acc, row, acc};
  }
  if (blockIdx.x == 0) {
    for (int j = t; j < it.m; j += kGpmBlockRows) it.pivots[j] = -1;
    if (t == 0) it.m_eff[0] = 0;
  }
  const GpmBest b = gpm_block_reduce(x, sv, ss, si);
  if (t == 0) { it.pmax[blockIdx.x] = b.v; it.pidx[blockIdx.x] = b.i; it.psum[blockIdx.x] = b.s; }
}

// GP1.  blockIdx = (block of rows, item); `step` = j.  Reads the partials' half j & 1, writes the other one.
template <bool kGeneral>
__global__ void __launch_bounds__(kGpmBlockRows) k_gpm_pivot_step(const GpmItem* __restrict__ items, int step) {
  __shared__ double sv[kGpmBlockRows], ss[kGpmBlockRows];
  __shared__ int si[kGpmBlockRows];
  __shared__ double Lp[kGpmMaxPivots];
  __shared__ double pv[kGpmPivotDoubles];  // (the <true> instance alone uses it)
  const GpmItem& it = items[blockIdx.y];
  if ((int)blockIdx.x >= it.nblk || step >= it.m) return;
  const int t = threadIdx.x, nblk = it.nblk, R = it.R;
  const int prev = (step & 1) * nblk, cur = ((step + 1) & 1) * nblk;
  const global_ptr<const double> pmax = as_global((const double*)it.pmax) + prev, psum = as_global((const double*)it.psum) + prev;
  const global_ptr<const int> pidx = as_global((const int*)it.pidx) + prev;
  GpmBest x{-INFINITY, INT_MAX, 0.0};
  for (int b = t; b < nblk; b += kGpmBlockRows) gpm_fold(x, pmax[b], pidx[b], psum[b]);
  const GpmBest best = gpm_block_reduce(x, sv, ss, si);
  double d0max, trace;
  if (step == 0) {
    d0max = best.v; trace = best.s;
    if (blockIdx.x == 0 && t == 0) { it.start[0] = d0max; it.start[1] = trace; }
  } else {
    d0max = it.start[0]; trace = it.start[1];
  }
  // the loop has stopped: numerical rank reached, or the residual trace is below the tolerance.  The partial is handed on unchanged,
  // so that every later launch decides the same.
  if (best.v <= ((double)it.m * 0x1p-52) * d0max || best.s <= it.rel_tol * trace) {
    if (t == 0) {
      it.pmax[cur + blockIdx.x] = pmax[blockIdx.x]; it.pidx[cur + blockIdx.x] = pidx[blockIdx.x]; it.psum[cur + blockIdx.x] = psum[blockIdx.x];
    }
    return;
  }
  const int p = best.i;
  if (blockIdx.x == 0 && t == 0) { it.pivots[step] = p; it.m_eff[0] = step + 1; }
  const global_ptr<const double> L = as_global((const double*)it.L), pts = as_global(it.pts);
  for (int k = t; k < step; k += kGpmBlockRows) Lp[k] = L[(size_t)k * R + p];
  if (kGeneral && it.general) gpm_stage_pivot(it, p / 3, pv);  // (uniform over the workgroup) the pivot's point, mirrors and weights
  __syncthreads();
  const int row = blockIdx.x * kGpmBlockRows + t;
  x = GpmBest{-INFINITY, INT_MAX, 0.0};
  if (row < R) {
    const int v = row / 3, c = row - 3 * v, vp = p / 3, cp = p - 3 * vp;
    double kv;
    if (kGeneral && it.general)  // (uniform over the workgroup)
      kv = gpm_general_value(it, v, pts[3 * v], pts[3 * v + 1], pts[3 * v + 2], c, pv, cp);
    else
      kv = gpm_kernel_value(it, pts[3 * v], pts[3 * v + 1], pts[3 * v + 2], c, pts[3 * vp], pts[3 * vp + 1], pts[3 * vp + 2], cp);
    double s = 0.0;
    const global_ptr<const double> Lr = L + row;
#pragma unroll 8
    for (int k = 0; k < step; ++k) s = s + Lr[(size_t)k * R] * Lp[k];
    const double l = (kv - s) / sqrt(best.v);
    it.L[(size_t)step * R + row] = l;
    const double dn = it.d[row] - l * l;
    it.d[row] = dn;
    x = GpmBest{dn, row, dn};
  }
  const GpmBest b = gpm_block_reduce(x, sv, ss, si);
  if (t == 0) { it.pmax[cur + blockIdx.x] = b.v; it.pidx[cur + blockIdx.x] = b.i; it.psum[cur + blockIdx.x] = b.s; }
}

// GP2.  One wave; blockIdx = (lower tile, slab, item).  Operand maps as k_proj_gemm's Qᵀ·D: lane l supplies A[i = l&15][k = l>>4] and
// B[k = l>>4][j = l&15] with k a ROW of L, A = column 16·ti + i of L, B = column 16·tj + j; result register g of lane l is
// G[16·ti + (l>>4) + 4g][16·tj + (l&15)].  Sixteen rows at a time: lane (i, kk) reads rows 4·kk .. 4·kk+3 of its two columns (32
// contiguous bytes each) and supplies row 4·kk + u to instruction u.  Rows past the slab and columns past m_eff supply zeros (a
// repeated, in-range load whose value is replaced).
__global__ void __launch_bounds__(64) k_gpm_gram(const GpmSpace* __restrict__ items) {
  const GpmSpace& it = items[blockIdx.z];
  const int tile = blockIdx.x, slab = blockIdx.y, nt = it.mp >> 4;
  if (slab >= it.slabs || tile >= nt * (nt + 1) / 2) return;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  const int tj = tile - ti * (ti + 1) / 2;
  const int l = threadIdx.x, i16 = l & 15, kk = l >> 4;
  const int R = it.R, me = it.me;
  const int ca = 16 * ti + i16, cb = 16 * tj + i16;
  const bool aok = ca < me, bok = cb < me;
  const global_ptr<const double> La = as_global(it.L) + (size_t)(aok ? ca : me - 1) * R, Lb = as_global(it.L) + (size_t)(bok ? cb : me - 1) * R;
  const int r0 = slab * it.slab_rows, r1 = min(R, r0 + it.slab_rows);
  d4_t acc = {0.0, 0.0, 0.0, 0.0};
  for (int rb = r0; rb < r1; rb += 16) {
    double a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = rb + 4 * kk + u;
      const bool rok = row < r1;
      const int rc = rok ? row : r1 - 1;
      const double va = La[rc], vb = Lb[rc];
      a[u] = rok && aok ? va : 0.0;
      b[u] = rok && bok ? vb : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
  }
  const global_ptr<double> out = as_global(it.Gpart) + (size_t)slab * it.mp * it.mp;
#pragma unroll
  for (int g = 0; g < 4; ++g) out[(size_t)(16 * ti + kk + 4 * g) * it.mp + 16 * tj + i16] = acc[g];
}

// GP3.  blockIdx = (block of 256 entries, item).  G[i][j] = scale · Σ_slabs Gpart[slab][max(i, j)][min(i, j)].
__global__ void __launch_bounds__(256) k_gpm_gram_sum(const GpmSpace* __restrict__ items) {
  const GpmSpace& it = items[blockIdx.y];
  const int me = it.me, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= me * me) return;
  const int i = e / me, j = e - i * me, hi = max(i, j), lo = min(i, j);
  const global_ptr<const double> part = as_global((const double*)it.Gpart) + (size_t)hi * it.mp + lo;
  double s = 0.0;
  for (int k = 0; k < it.slabs; ++k) s = s + part[(size_t)k * it.mp * it.mp];
  it.G[e] = s * it.scale;
}

// GP4a-d.  One step of the eigenvector refinement of Ogita and Aishima (Japan J. Indust. Appl. Math. 35, 2018) on the decomposition's V:
// the resident routes stop at eigenvectors good to 1e-11 (the chain draws samples from them), a model's basis wants them to rounding.
//   T = G·V;   S = VᵀT,  R = I − VᵀV  (each entry once, mirrored);   λ_i = S_ii / (1 − R_ii);
//   E_ij = (S_ij + λ_j R_ij) / (λ_j − λ_i)  where |λ_j − λ_i| > kGpmCluster, else R_ij / 2 (inside a cluster — an isotropic kernel has its
//   eigenvalues in threes — only the orthogonality is restored; the diagonal: the normalisation);   W = V + V·E.
// The error of V enters W squared.  kGpmCluster is absolute: G is scaled to a trace of at most 2, and an entry of S is good to a few
// 2⁻⁵² of that, so E carries noise of at most 1e-7, antisymmetric (S is symmetric as bits), whose square is what reaches WᵀW.
// blockIdx = (block of 256 entries, item); every entry's sum runs over k = 0, 1, … in order.
constexpr double kGpmCluster = 1e-8;
__global__ void __launch_bounds__(256) k_gpm_refine_gv(const GpmSpace* __restrict__ items) {
  const GpmSpace& it = items[blockIdx.y];
  const int me = it.me, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= me * me) return;
  const int i = e / me, j = e - i * me;
  const global_ptr<const double> g = as_global((const double*)it.G) + (size_t)i * me, v = as_global(it.V) + j;
  double s = 0.0;
  for (int k = 0; k < me; ++k) s = s + g[k] * v[(size_t)k * me];
  it.T[e] = s;
}
__global__ void __launch_bounds__(256) k_gpm_refine_sr(const GpmSpace* __restrict__ items) {
  const GpmSpace& it = items[blockIdx.y];
  const int me = it.me, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= me * me) return;
  const int i = e / me, j = e - i * me;
  if (i > j) return;
  const global_ptr<const double> vi = as_global(it.V) + i, vj = as_global(it.V) + j, tj = as_global((const double*)it.T) + j;
  double s = 0.0, r = 0.0;
  for (int k = 0; k < me; ++k) {
    const double a = vi[(size_t)k * me];
    s = s + a * tj[(size_t)k * me];
    r = r + a * vj[(size_t)k * me];
  }
  r = (i == j ? 1.0 : 0.0) - r;
  it.Sm[e] = s; it.Sm[(size_t)j * me + i] = s;
  it.Rm[e] = r; it.Rm[(size_t)j * me + i] = r;
}
__global__ void __launch_bounds__(256) k_gpm_refine_e(const GpmSpace* __restrict__ items) {
  const GpmSpace& it = items[blockIdx.y];
  const int me = it.me, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= me * me) return;
  const int i = e / me, j = e - i * me;
  const global_ptr<const double> Sm = as_global((const double*)it.Sm), Rm = as_global((const double*)it.Rm);
  const double li = Sm[(size_t)i * me + i] / (1.0 - Rm[(size_t)i * me + i]), lj = Sm[(size_t)j * me + j] / (1.0 - Rm[(size_t)j * me + j]);
  const double gap = lj - li;
  it.E[e] = i != j && fabs(gap) > kGpmCluster ? (Sm[e] + lj * Rm[e]) / gap : 0.5 * Rm[e];
  if (i == 0) {  // eigenvalue j: its place among all of them, descending
    int rank = 0;
    for (int k = 0; k < me; ++k) {
      const double lk = Sm[(size_t)k * me + k] / (1.0 - Rm[(size_t)k * me + k]);
      rank += lk > lj || (lk == lj && k < j) ? 1 : 0;
    }
    it.lam[j] = lj;
    it.order[rank] = j;
  }
}
__global__ void __launch_bounds__(256) k_gpm_refine_w(const GpmSpace* __restrict__ items) {
  const GpmSpace& it = items[blockIdx.y];
  const int me = it.me, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= me * me) return;
  const int i = e / me, j = e - i * me;
  const global_ptr<const double> v = as_global(it.V) + (size_t)i * me, ej = as_global((const double*)it.E) + j;
  double s = 0.0;
  for (int k = 0; k < me; ++k) s = s + v[k] * ej[(size_t)k * me];
  it.T[e] = v[j] + s;
}

// GP4.  blockIdx = (block of 256 entries, item).  Column j of the operand is the eigenpair order[j]: θ_j = lam / scale, descending.
// Op[k][j] = W[k][order[j]]·√N/√θ_j for j < re, zero elsewhere; variance[j] = θ_j/N.
__global__ void __launch_bounds__(256) k_gpm_operand(const GpmSpace* __restrict__ items) {
  const GpmSpace& it = items[blockIdx.y];
  const int me = it.me, ldb = it.ldb, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= it.mp * ldb) return;
  const int k = e / ldb, j = e - k * ldb;
  double v = 0.0, theta = 0.0;
  if (j < it.re) {
    const int src = min(max(it.order[j], 0), me - 1);  // (in range whatever a decomposition that gave up has left: that item is decomposed again)
    theta = it.lam[src] / it.scale;
    if (k < me) v = it.T[(size_t)k * me + src] * (sqrt(it.n_points) / sqrt(theta));
  }
  it.Op[e] = v;
  if (k == 0 && j < it.rank) it.variance[j] = j < it.re ? theta / it.n_points : 0.0;
}

// GP5.  One wave; blockIdx = (block of kGpmColTiles column tiles, block of kGpmRowTiles row tiles, piece).  k_pm_gemm's operand maps with
// the left operand column by column: lane (i, kk) reads its row of the four neighbouring columns 4·kk .. 4·kk+3 of a block of 16 (for
// one column, the wave's 16 rows are 128 contiguous bytes) and supplies column 4·kk + u to instruction u.
constexpr int kGpmRowTiles = 2, kGpmColTiles = 4;
__global__ void __launch_bounds__(64) k_gpm_gemm(const GpmPiece* __restrict__ pieces) {
  const GpmPiece& pc = pieces[blockIdx.z];
  const int me = pc.me, ldb = pc.ldb, R = pc.R;
  const int t0 = blockIdx.x * kGpmColTiles, nt = ldb >> 4;
  const int row_a = blockIdx.y * 16 * kGpmRowTiles;
  if (t0 >= nt || row_a >= pc.rows) return;
  const int tn = min(kGpmColTiles, nt - t0);  // (uniform) column tiles of this block
  const int l = threadIdx.x, i16 = l & 15, kk = l >> 4;
  const global_ptr<const double> Op = as_global(pc.Op) + 16 * t0 + i16;
  global_ptr<const double> lrow[kGpmRowTiles];
  bool rok[kGpmRowTiles];
#pragma unroll
  for (int t = 0; t < kGpmRowTiles; ++t) {
    const int row = row_a + 16 * t + i16;
    rok[t] = row < pc.rows;
    lrow[t] = as_global(pc.L) + (size_t)(pc.row0 + (rok[t] ? row : pc.rows - 1));
  }
  d4_t acc[kGpmRowTiles][kGpmColTiles];
#pragma unroll
  for (int t = 0; t < kGpmRowTiles; ++t)
#pragma unroll
    for (int c = 0; c < kGpmColTiles; ++c) acc[t][c] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < me; k0 += 16) {
    double a[kGpmRowTiles][4], b[4][kGpmColTiles];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 4 * kk + u;
      const bool kok = k < me;
      const int kc = kok ? k : me - 1;
#pragma unroll
      for (int t = 0; t < kGpmRowTiles; ++t) {
        const double v = lrow[t][(size_t)kc * R];
        a[t][u] = kok && rok[t] ? v : 0.0;
      }
#pragma unroll
      for (int c = 0; c < kGpmColTiles; ++c) b[u][c] = c < tn ? Op[(size_t)k * ldb + 16 * c] : 0.0;  // (Op has m_eff rounded up to 16 rows: in range)
    }
    __builtin_amdgcn_sched_barrier(0);  // (all loads requested before the first product)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < kGpmRowTiles; ++t)
#pragma unroll
        for (int c = 0; c < kGpmColTiles; ++c)
          if (c < tn) acc[t][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][u], b[u][c], acc[t][c], 0, 0, 0);
  }
  const global_ptr<double> out = as_global(pc.out);
#pragma unroll
  for (int t = 0; t < kGpmRowTiles; ++t)
#pragma unroll
    for (int c = 0; c < kGpmColTiles; ++c) {
      if (c >= tn) continue;
      const int col = 16 * (t0 + c) + i16;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = row_a + 16 * t + kk + 4 * g;
        if (row < pc.rows && col < pc.rank) out[(size_t)row * pc.rank + col] = acc[t][c][g];
      }
    }
}

// Region weights (icp_region_weights_many; FaceMask.computeSmoothedRegions).  blockIdx = (block of 256 query points, item); a thread
// owns one query point; the region's points pass through LDS 256 at a time.  A minimum does not depend on the order it is taken in.
constexpr int kGpmRegionTile = 256;
__global__ void __launch_bounds__(kGpmRegionTile) k_gpm_region_weights(const GpmRegion* __restrict__ items) {
  __shared__ double sr[3 * kGpmRegionTile];
  const GpmRegion& it = items[blockIdx.y];
  if ((int)blockIdx.x * kGpmRegionTile >= it.n) return;  // (uniform)
  const int t = threadIdx.x, i = blockIdx.x * kGpmRegionTile + t;
  const bool ok = i < it.n;
  const global_ptr<const double> pts = as_global(it.pts), reg = as_global(it.reg);
  const int ic = ok ? i : it.n - 1;
  const double x0 = pts[3 * ic], x1 = pts[3 * ic + 1], x2 = pts[3 * ic + 2];
  double best = INFINITY;
  for (int r0 = 0; r0 < it.n_reg; r0 += kGpmRegionTile) {
    const int cnt = min(kGpmRegionTile, it.n_reg - r0);
    __syncthreads();  // (the tile may still be read)
    for (int k = t; k < 3 * cnt; k += kGpmRegionTile) sr[k] = reg[(size_t)3 * r0 + k];
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const double dx = x0 - sr[3 * k], dy = x1 - sr[3 * k + 1], dz = x2 - sr[3 * k + 2];
      best = fmin(best, (dx * dx + dy * dy) + dz * dz);
    }
  }
  if (ok) it.w[i] = exp(-(best / it.s2));
}

}  // namespace

// rows of a slab of the Gram sum: 1,024, or as many more (in steps of 1,024) as keep the slabs at kGpmMaxSlabs
int gpm_slab_rows(int R) { return 1024 * std::max(1, cdiv(R, 1024 * kGpmMaxSlabs)); }

void launch_gpm_init(hipStream_t st, int n_items, int nblk_max, const GpmItem* items, bool any_general) {
  if (n_items <= 0) return;
  if (any_general) hipLaunchKernelGGL(k_gpm_init<true>, dim3(nblk_max, n_items), dim3(kGpmBlockRows), 0, st, items);
  else hipLaunchKernelGGL(k_gpm_init<false>, dim3(nblk_max, n_items), dim3(kGpmBlockRows), 0, st, items);
}
void launch_gpm_pivot_step(hipStream_t st, int n_items, int nblk_max, int step, const GpmItem* items, bool any_general) {
  if (n_items <= 0) return;
  if (any_general) hipLaunchKernelGGL(k_gpm_pivot_step<true>, dim3(nblk_max, n_items), dim3(kGpmBlockRows), 0, st, items, step);
  else hipLaunchKernelGGL(k_gpm_pivot_step<false>, dim3(nblk_max, n_items), dim3(kGpmBlockRows), 0, st, items, step);
}
void launch_gpm_region_weights(hipStream_t st, int n_items, int n_max, const GpmRegion* items) {
  if (n_items <= 0 || n_max <= 0) return;
  hipLaunchKernelGGL(k_gpm_region_weights, dim3(cdiv(n_max, kGpmRegionTile), n_items), dim3(kGpmRegionTile), 0, st, items);
}
void launch_gpm_gram(hipStream_t st, int n, int mp_max, int slabs_max, const GpmSpace* items) {
  if (n <= 0) return;
  const int nt = mp_max >> 4;
  hipLaunchKernelGGL(k_gpm_gram, dim3(nt * (nt + 1) / 2, slabs_max, n), dim3(64), 0, st, items);
  hipLaunchKernelGGL(k_gpm_gram_sum, dim3(cdiv(mp_max * mp_max, 256), n), dim3(256), 0, st, items);
}
void launch_gpm_refine(hipStream_t st, int n, int me_max, const GpmSpace* items) {
  if (n <= 0) return;
  const dim3 grid(cdiv(me_max * me_max, 256), n);
  hipLaunchKernelGGL(k_gpm_refine_gv, grid, dim3(256), 0, st, items);
  hipLaunchKernelGGL(k_gpm_refine_sr, grid, dim3(256), 0, st, items);
  hipLaunchKernelGGL(k_gpm_refine_e, grid, dim3(256), 0, st, items);
  hipLaunchKernelGGL(k_gpm_refine_w, grid, dim3(256), 0, st, items);
}
void launch_gpm_operand(hipStream_t st, int n, int mp_max, int ldb_max, const GpmSpace* items) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gpm_operand, dim3(cdiv(mp_max * ldb_max, 256), n), dim3(256), 0, st, items);
}
void launch_gpm_gemm(hipStream_t st, int n_pieces, int rows_max, int col_tiles_max, const GpmPiece* pieces) {
  if (n_pieces <= 0) return;
  hipLaunchKernelGGL(k_gpm_gemm, dim3(cdiv(col_tiles_max, kGpmColTiles), cdiv(rows_max, 16 * kGpmRowTiles), n_pieces), dim3(64), 0, st, pieces);
}

}  // namespace icp
