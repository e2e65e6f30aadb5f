// kernels_nystrom_model.hip — Gaussian-process shape models by the Nyström approximation on sample points, many side by side
// (icp_nystrom_models_many; what apps/femur/CreateGPModel.scala and apps/bfm/CreateGPModel.scala call, approximateGPNystrom).  For the
// mesh points X (N), the sample points S (n), R = 3n:
//   K = k(S, S) = U·Λ·Uᵀ;  variance_i = λ_i/n;  basis column i = k(X, S)·u_i·√n/λ_i;  k_eff = #{i < k : λ_i/n >= min_variance}.
//
//   NY0 k_nys_kernel_matrix  K into the padded Rp × Rp buffer (Rp = R rounded up to an even number of 32-blocks; the padding is zero):
//                            a thread owns a pair of sample points i <= j and writes both triangles from ONE evaluation
//   NY1 k_nys_norm           ‖K‖_F², trace K, the stop level and the rotation threshold; V = I; the item's state
//   The eigenproblem is a two-sided block Jacobi iteration on blocks of 32 columns.  A round is one step of a round-robin tournament,
//   Rp/64 disjoint block pairs at once; a sweep is Rp/32 − 1 rounds; per round:
//   NY2 k_nys_pair           a workgroup per pair: the 64 × 64 pair matrix into LDS, its pre-rotation off-diagonal mass, and — unless
//                            it is diagonal to the threshold already — cyclic Jacobi sweeps in LDS STARTED FROM THE IDENTITY, the
//                            rotation of the smaller angle, no re-ordering: the pair's U is the one nearest the identity (a kernel
//                            matrix has a flat tail; arbitrary bases inside its clusters make the iteration stagnate).  One
//                            Newton–Schulz step U ← U + U·(I − UᵀU)/2 then makes U orthogonal to rounding: without it the thousands
//                            of rotations behind V leave it orthogonal to 1e-13 only, and the residuals at 1e-13·λ₁.
//   NY3 k_nys_rows           A ← UᵀA on the pair's row panel, on the f64 matrix cores: a workgroup per (pair, tile of 64 columns)
//   NY4 k_nys_cols           A ← A·U and V ← V·U on the pair's column panels: a workgroup per (pair, tile of 64 rows, matrix)
//   NY5 k_nys_sweep_end      the sweep's mass, summed in a fixed order; an item whose mass is <= (R·2⁻⁵²·‖K‖_F)² is done, and every
//                            later launch returns at once for it; the items still iterating are counted into ONE word for the host
//   NY6 k_nys_sort           the eigenvalues (the diagonal of A over the R real rows) in descending order
//   NY7 k_nys_operand        W = U_k·√n·diag(1/λ) over the first k_eff columns, zero-padded to 16s; variances; k_eff; U_k as handed out
//   NY8 k_nys_basis          rows of k(X, S)·W on the f64 matrix cores into the chunk buffer; the left operand is evaluated on the fly
//                            from the points and the terms, 16 sample rows at a time, and never stored
//
// An item's bits depend on nothing but the item: every reduction is a fixed tree or a fixed order over the item's own sizes, a pair's
// work does not depend on which other pairs or items share the launch, and the contraction of NY8 runs over the sample rows in blocks of
// 16 from 0.0 whatever shares the wave, the piece or the round.  No floating-point atomics; no workgroup waits for another.
// The padding never mixes with the data: its rows of K are exactly zero, a rotation is skipped where the entry is below the
// threshold, so every U is exactly the identity on padded indices and the products keep the zeros exact.
#include "icp_kernels.hpp"
#include "icp_dense.hpp"
#include "icp_gp_terms.hpp"

#include <algorithm>

namespace icp {

namespace {

constexpr int kNysPair = 2 * kNysBlock;  // 64
constexpr int kNysLd = kNysPair + 1;     // LDS row stride where a wave walks down a column
constexpr int kNysInnerSweeps = 30;

// pair k of step `step` of the round-robin tournament of m players (m even): p < q
__device__ __forceinline__ void nys_pair_of(int m, int step, int k, int& p, int& q) {
  int a, b;
  if (k == 0) {
    a = m - 1; b = step;
  } else {
    a = (step + k) % (m - 1); b = (step - k + (m - 1)) % (m - 1);
  }
  p = min(a, b); q = max(a, b);
}

// K[3·vx + c][3·j + cp] between a point x — sample vx (kXSample) or mesh vertex vx — and sample j, the terms summed in order: the
// expressions of kernels_gp_model.hip (gpm_kernel_value for an item of plain terms, gpm_general_value otherwise)
template <bool kXSample>
__device__ __forceinline__ double nys_entry(const NysItem& it, int vx, double x0, double x1, double x2, int j, double y0, double y1, double y2,
                                            int c, int cp) {
  double acc = 0.0;
  if (!it.general) {
    const double dx = x0 - y0, dy = x1 - y1, dz = x2 - y2;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    for (int t = 0; t < it.n_terms; ++t) {
      const GpmTerm& tm = it.terms[t];
      acc = acc + (tm.scale * exp(-(d2 / tm.sigma2))) * tm.A[3 * c + cp];
    }
    return acc;
  }
  for (int t = 0; t < it.n_terms; ++t) {
    const GpmTerm& tm = it.terms[t];
    const double a = tm.A[3 * c + cp];
    double ww = 1.0;
    if (tm.w) ww = as_global(kXSample ? it.sw[t] : tm.w)[vx] * as_global(it.sw[t])[j];
    double val = gpm_base(tm, x0, x1, x2, y0, y1, y2);
    if (tm.gain > 0.0) {
      const double sgn = c == tm.axis ? -1.0 : 1.0;
      const double bm = gpm_base(tm, x0, x1, x2, tm.axis == 0 ? -y0 : y0, tm.axis == 1 ? -y1 : y1, tm.axis == 2 ? -y2 : y2);
      val = val + (tm.gain * sgn) * bm;
    }
    acc = acc + ((tm.scale * ww) * val) * a;
  }
  return acc;
}

// the workgroup's sum (or maximum) of its 256 threads' values, in every thread; a fixed tree
template <bool kMax>
__device__ __forceinline__ double nys_block_reduce(double x, double* red) {
  const int t = threadIdx.x;
  __syncthreads();  // (the array may still be read from an earlier reduction)
  red[t] = x;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] = kMax ? fmax(red[t], red[t + o]) : red[t] + red[t + o];
    __syncthreads();
  }
  return red[0];
}

// NY0.  blockIdx = (block of 256 pairs of sample points, item).
__global__ void __launch_bounds__(256) k_nys_kernel_matrix(const NysItem* __restrict__ items) {
  const NysItem& it = items[blockIdx.y];
  const int n = it.n, Rp = it.Rp;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)n * n) return;
  const int i = (int)(e / n), j = (int)(e - (long long)i * n);
  if (i > j) return;
  const global_ptr<const double> s = as_global(it.smp);
  const double x0 = s[3 * i], x1 = s[3 * i + 1], x2 = s[3 * i + 2], y0 = s[3 * j], y1 = s[3 * j + 1], y2 = s[3 * j + 2];
  const global_ptr<double> A = as_global(it.A);
  for (int c = 0; c < 3; ++c)
    for (int cp = 0; cp < 3; ++cp) {
      if (i == j && cp < c) continue;  // (the diagonal block: its upper triangle, mirrored)
      const double v = nys_entry<true>(it, i, x0, x1, x2, j, y0, y1, y2, c, cp);
      A[(size_t)(3 * i + c) * Rp + 3 * j + cp] = v;
      A[(size_t)(3 * j + cp) * Rp + 3 * i + c] = v;
    }
}

// NY1.  One workgroup per item: thread t owns rows t, t + 256, … of K, summed in order; a fixed tree over the threads.
__global__ void __launch_bounds__(256) k_nys_norm(const NysItem* __restrict__ items) {
  __shared__ double red[256];
  const NysItem& it = items[blockIdx.x];
  const int t = threadIdx.x, R = it.R, Rp = it.Rp;
  const global_ptr<const double> A = as_global((const double*)it.A);
  double f = 0.0, tr = 0.0;
  for (int r = t; r < R; r += 256) {
    double s = 0.0;
    for (int k = 0; k < R; ++k) {
      const double a = A[(size_t)r * Rp + k];
      s = s + a * a;
    }
    f = f + s;
    tr = tr + A[(size_t)r * Rp + r];
  }
  for (int r = t; r < Rp; r += 256) it.V[(size_t)r * Rp + r] = 1.0;  // (V was zeroed in front of the launch)
  f = nys_block_reduce<false>(f, red);
  tr = nys_block_reduce<false>(tr, red);
  if (t == 0) {
    const double fro = sqrt(f);
    const double level = ((double)R * 0x1p-52) * fro;
    it.norm[0] = f; it.norm[1] = tr; it.norm[2] = level * level; it.norm[3] = 0x1p-54 * fro;
    it.state[0] = 0; it.state[1] = 0; it.state[2] = 0; it.state[3] = 0;
    it.offmass[0] = 0.0;
  }
}

// NY2.  blockIdx = (pair, item); 256 threads; dynamic LDS: the pair matrix and U (64 × 65 each), the step's rotations, a reduction array.
constexpr size_t kNysPairLds = sizeof(double) * (2 * kNysPair * kNysLd + 2 * kNysBlock + 256) + sizeof(int) * (2 * kNysBlock + 2);
__global__ void __launch_bounds__(256) k_nys_pair(const NysItem* __restrict__ items, int round) {
  extern __shared__ double nys_lds[];
  double* As = nys_lds;
  double* Us = As + kNysPair * kNysLd;
  double* cs = Us + kNysPair * kNysLd;
  double* sn = cs + kNysBlock;
  double* red = sn + kNysBlock;
  int* pq = (int*)(red + 256);
  int* nrot = pq + 2 * kNysBlock;
  const NysItem& it = items[blockIdx.y];
  const int pair = blockIdx.x, np = it.nb >> 1;
  if (pair >= np || round >= it.nb - 1 || it.state[0]) return;  // (uniform)
  int I, J;
  nys_pair_of(it.nb, round, pair, I, J);
  const int t = threadIdx.x, Rp = it.Rp;
  const global_ptr<const double> A = as_global((const double*)it.A);
  // the pair matrix from the upper triangle of A, mirrored: exactly symmetric.  Thread t owns column t & 63 of rows (t >> 6) + 4i.
  double m = 0.0, big = 0.0;
  for (int e = t; e < kNysPair * kNysPair; e += 256) {
    const int a = e >> 6, b = e & 63, lo = min(a, b), hi = max(a, b);
    const int gl = lo < kNysBlock ? kNysBlock * I + lo : kNysBlock * J + lo - kNysBlock;
    const int gh = hi < kNysBlock ? kNysBlock * I + hi : kNysBlock * J + hi - kNysBlock;
    const double v = A[(size_t)gl * Rp + gh];
    As[a * kNysLd + b] = v;
    Us[a * kNysLd + b] = a == b ? 1.0 : 0.0;
    if (a != b) {
      big = fmax(big, fabs(v));
      // every block pair meets once a sweep; the diagonal blocks' own off-diagonal entries count in the sweep's first round, where every
      // block appears once
      if (((a < kNysBlock) != (b < kNysBlock)) || round == 0) m = m + v * v;
    }
  }
  m = nys_block_reduce<false>(m, red);
  big = nys_block_reduce<true>(big, red);
  const double tau = it.norm[3];
  if (t == 0) {
    it.mass[(size_t)round * np + pair] = m;
    it.rotated[pair] = big > tau ? 1 : 0;
  }
  if (!(big > tau)) return;  // (uniform) diagonal to the stop level already: U is the identity and nothing is applied

  for (int sw = 0; sw < kNysInnerSweeps; ++sw) {
    if (t == 0) *nrot = 0;
    __syncthreads();
    for (int step = 0; step < kNysPair - 1; ++step) {
      if (t < kNysBlock) {
        int p, q;
        nys_pair_of(kNysPair, step, t, p, q);
        const double apq = As[p * kNysLd + q];
        double c = 1.0, s = 0.0;
        if (fabs(apq) > tau) {
          const double th = (As[q * kNysLd + q] - As[p * kNysLd + p]) / (2.0 * apq);
          const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));  // the smaller root: |angle| <= π/4
          c = 1.0 / sqrt(tt * tt + 1.0);
          s = tt * c;
          atomicAdd(nrot, 1);
        }
        cs[t] = c; sn[t] = s; pq[2 * t] = p; pq[2 * t + 1] = q;
      }
      __syncthreads();
      // every thread owns 8 (rotation, row) and then 8 (rotation, column) places of the step: all of a phase's values are read before the
      // first is written (the places of one phase are distinct, which the compiler cannot see through LDS)
      const int lane64 = t & 63;
      double c8[8], s8[8];
      int p8[8], q8[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = (t >> 6) + 4 * i;
        c8[i] = cs[k]; s8[i] = sn[k]; p8[i] = pq[2 * k]; q8[i] = pq[2 * k + 1];
      }
      {  // columns p, q of A and of U, row lane64
        double ap[8], aq[8], up[8], uq[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          ap[i] = As[lane64 * kNysLd + p8[i]]; aq[i] = As[lane64 * kNysLd + q8[i]];
          up[i] = Us[lane64 * kNysLd + p8[i]]; uq[i] = Us[lane64 * kNysLd + q8[i]];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (s8[i] == 0.0) continue;
          As[lane64 * kNysLd + p8[i]] = c8[i] * ap[i] - s8[i] * aq[i];
          As[lane64 * kNysLd + q8[i]] = s8[i] * ap[i] + c8[i] * aq[i];
          Us[lane64 * kNysLd + p8[i]] = c8[i] * up[i] - s8[i] * uq[i];
          Us[lane64 * kNysLd + q8[i]] = s8[i] * up[i] + c8[i] * uq[i];
        }
      }
      __syncthreads();
      {  // rows p, q of A, column lane64
        double ap[8], aq[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          ap[i] = As[p8[i] * kNysLd + lane64]; aq[i] = As[q8[i] * kNysLd + lane64];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (s8[i] == 0.0) continue;
          As[p8[i] * kNysLd + lane64] = c8[i] * ap[i] - s8[i] * aq[i];
          As[q8[i] * kNysLd + lane64] = s8[i] * ap[i] + c8[i] * aq[i];
        }
      }
      __syncthreads();
    }
    const int rotations = *nrot;
    __syncthreads();  // (read by everyone before thread 0 zeroes it again)
    if (rotations == 0) break;
  }
  // one Newton–Schulz step: E = I − UᵀU into the pair matrix's place, then U + U·E/2
  for (int e = t; e < kNysPair * kNysPair; e += 256) {
    const int i = e >> 6, j = e & 63;
    double s = 0.0;
    for (int k = 0; k < kNysPair; ++k) s = s + Us[k * kNysLd + i] * Us[k * kNysLd + j];
    As[i * kNysLd + j] = (i == j ? 1.0 : 0.0) - s;
  }
  __syncthreads();
  const global_ptr<double> Uo = as_global(it.U) + (size_t)pair * kNysPair * kNysPair;
  for (int e = t; e < kNysPair * kNysPair; e += 256) {
    const int i = e >> 6, j = e & 63;
    double s = 0.0;
    for (int k = 0; k < kNysPair; ++k) s = s + Us[i * kNysLd + k] * As[k * kNysLd + j];
    Uo[e] = Us[i * kNysLd + j] + 0.5 * s;
  }
}

// row or column g of the pair (I, J) in the item's matrices
__device__ __forceinline__ int nys_global_index(int I, int J, int g) { return g < kNysBlock ? kNysBlock * I + g : kNysBlock * J + g - kNysBlock; }

// a wave's 16 rows × 64 columns of X·Y for 64 × 64 operands in LDS: X element (i, k) at X[i·xi + k·xk], Y row-major with stride 64.
// Operand maps of v_mfma_f64_16x16x4_f64 as k_gpm_gemm's: lane (i = l & 15, kk = l >> 4) supplies X[16w + i][k0 + kk] and
// Y[k0 + kk][16c + i]; result register g of tile c is row 16w + kk + 4g, column 16c + i.  k0 = 0, 4, … in order.
__device__ __forceinline__ void nys_tile_product(const double* X, int xi, int xk, const double* Y, int w, int i16, int kk, d4_t acc[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < kNysPair; k0 += 4) {
    const double a = X[(16 * w + i16) * xi + (k0 + kk) * xk];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Y[(k0 + kk) * kNysPair + 16 * c + i16], acc[c], 0, 0, 0);
  }
}

constexpr size_t kNysApplyLds = sizeof(double) * (kNysPair * kNysPair + kNysPair * kNysLd);
// NY3.  blockIdx = (tile of 64 columns, pair, item); 256 threads = 4 waves, wave w owns rows 16w .. 16w+15 of the panel.
__global__ void __launch_bounds__(256) k_nys_rows(const NysItem* __restrict__ items, int round) {
  extern __shared__ double nys_lds[];
  double* Us = nys_lds;
  double* Ps = Us + kNysPair * kNysPair;
  const NysItem& it = items[blockIdx.z];
  const int tile = blockIdx.x, pair = blockIdx.y, Rp = it.Rp;
  if (pair >= (it.nb >> 1) || tile >= (Rp >> 6) || round >= it.nb - 1 || it.state[0] || !it.rotated[pair]) return;  // (uniform)
  int I, J;
  nys_pair_of(it.nb, round, pair, I, J);
  const int t = threadIdx.x;
  const global_ptr<const double> U = as_global((const double*)it.U) + (size_t)pair * kNysPair * kNysPair;
  const global_ptr<double> A = as_global(it.A) + (size_t)kNysPair * tile;
  for (int e = t; e < kNysPair * kNysPair; e += 256) {
    const int i = e >> 6, j = e & 63;
    Us[e] = U[e];
    Ps[e] = A[(size_t)nys_global_index(I, J, i) * Rp + j];
  }
  __syncthreads();
  const int w = t >> 6, l = t & 63, i16 = l & 15, kk = l >> 4;
  d4_t acc[4];
  nys_tile_product(Us, 1, kNysPair, Ps, w, i16, kk, acc);  // X = Uᵀ
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g) A[(size_t)nys_global_index(I, J, 16 * w + kk + 4 * g) * Rp + 16 * c + i16] = acc[c][g];
}

// NY4.  blockIdx = (tile of 64 rows of A, then of V; pair; item).
__global__ void __launch_bounds__(256) k_nys_cols(const NysItem* __restrict__ items, int round) {
  extern __shared__ double nys_lds[];
  double* Us = nys_lds;
  double* Qs = Us + kNysPair * kNysPair;  // stride kNysLd
  const NysItem& it = items[blockIdx.z];
  const int pair = blockIdx.y, Rp = it.Rp, tiles = Rp >> 6;
  if (pair >= (it.nb >> 1) || (int)blockIdx.x >= 2 * tiles || round >= it.nb - 1 || it.state[0] || !it.rotated[pair]) return;  // (uniform)
  const bool onV = (int)blockIdx.x >= tiles;
  const int tile = onV ? blockIdx.x - tiles : blockIdx.x;
  int I, J;
  nys_pair_of(it.nb, round, pair, I, J);
  const int t = threadIdx.x;
  const global_ptr<const double> U = as_global((const double*)it.U) + (size_t)pair * kNysPair * kNysPair;
  const global_ptr<double> M = as_global(onV ? it.V : it.A) + (size_t)kNysPair * tile * Rp;
  for (int e = t; e < kNysPair * kNysPair; e += 256) {
    const int i = e >> 6, j = e & 63;
    Us[e] = U[e];
    Qs[i * kNysLd + j] = M[(size_t)i * Rp + nys_global_index(I, J, j)];
  }
  __syncthreads();
  const int w = t >> 6, l = t & 63, i16 = l & 15, kk = l >> 4;
  d4_t acc[4];
  nys_tile_product(Qs, kNysLd, 1, Us, w, i16, kk, acc);
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g) M[(size_t)(16 * w + kk + 4 * g) * Rp + nys_global_index(I, J, 16 * c + i16)] = acc[c][g];
}

// NY5.  One workgroup per item: thread t sums the masses t, t + 256, … in order; a fixed tree.
__global__ void __launch_bounds__(256) k_nys_sweep_end(const NysItem* __restrict__ items, int* __restrict__ active) {
  __shared__ double red[256];
  const NysItem& it = items[blockIdx.x];
  if (it.state[0]) return;  // (uniform)
  const int t = threadIdx.x, cnt = (it.nb - 1) * (it.nb >> 1);
  double s = 0.0;
  for (int k = t; k < cnt; k += 256) s = s + it.mass[k];
  s = nys_block_reduce<false>(s, red);
  if (t == 0) {
    it.state[1] = it.state[1] + 1;
    it.offmass[0] = s;
    // one pair is the whole problem: its decomposition is complete, there is no iteration
    if (s <= it.norm[2] || it.nb == 2) it.state[0] = 1;
    else atomicAdd(active, 1);
  }
}

// NY6.  blockIdx = (block of 256 eigenvalues, item): eigenvalue j's place among the R real ones, descending, ties to the lower index.
__global__ void __launch_bounds__(256) k_nys_sort(const NysItem* __restrict__ items) {
  const NysItem& it = items[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x, R = it.R;
  if (j >= R) return;
  const global_ptr<const double> A = as_global((const double*)it.A);
  const size_t ld = (size_t)it.Rp + 1;
  const double lj = A[j * ld];
  int rank = 0;
  for (int k = 0; k < R; ++k) {
    const double lk = A[k * ld];
    rank += lk > lj || (lk == lj && k < j) ? 1 : 0;
  }
  it.lam[rank] = lj;
  it.order[rank] = j;
}

// NY7.  blockIdx = (block of 256 entries of W, item).
__global__ void __launch_bounds__(256) k_nys_operand(const NysItem* __restrict__ items) {
  const NysItem& it = items[blockIdx.y];
  const int t = threadIdx.x, R = it.R, Rp = it.Rp, kp = it.kp, rank = it.rank;
  const double n = (double)it.n;
  const int keff = __syncthreads_count(t < rank && it.lam[min(t, R - 1)] / n >= it.min_variance);
  const int e = blockIdx.x * 256 + t;
  if (e >= Rp * kp) return;
  const int r = e / kp, j = e - r * kp;
  double v = 0.0;
  if (r < R && j < rank) {
    const double u = it.V[(size_t)r * Rp + it.order[j]];
    it.Uk[(size_t)r * rank + j] = u;
    if (j < keff) v = u * (sqrt(n) / it.lam[j]);
  }
  it.W[e] = v;
  if (r == 0 && j < rank) it.variance[j] = it.lam[j] / n;
  if (e == 0) it.state[2] = keff;
}

// NY8.  One wave; blockIdx = (block of kNysColTiles column tiles, tile of 16 rows, piece).  Lane (i, kk) owns row i of the tile — a
// vertex and a coordinate of the mesh — and evaluates its kernel values against the sample rows 4·kk .. 4·kk+3 of a block of 16,
// supplying sample row 4·kk + u to instruction u (k_gpm_gemm's maps).
constexpr int kNysColTiles = 8;
__global__ void __launch_bounds__(64) k_nys_basis(const NysPiece* __restrict__ pieces) {
  const NysPiece& pc = pieces[blockIdx.z];
  const NysItem& it = *pc.item;
  const int kp = it.kp, R = it.R, rank = it.rank;
  const int t0 = blockIdx.x * kNysColTiles, nt = kp >> 4, row_a = blockIdx.y * 16;
  if (t0 >= nt || row_a >= pc.rows) return;
  const int tn = min(kNysColTiles, nt - t0);  // (uniform)
  const int l = threadIdx.x, i16 = l & 15, kk = l >> 4;
  const bool rok = row_a + i16 < pc.rows;
  const int grow = pc.row0 + (rok ? row_a + i16 : pc.rows - 1), v = grow / 3, c = grow - 3 * v;
  const global_ptr<const double> pts = as_global(it.pts), smp = as_global(it.smp);
  const double x0 = pts[3 * v], x1 = pts[3 * v + 1], x2 = pts[3 * v + 2];
  const global_ptr<const double> W = as_global((const double*)it.W) + 16 * t0 + i16;
  d4_t acc[kNysColTiles];
#pragma unroll
  for (int cc = 0; cc < kNysColTiles; ++cc) acc[cc] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < R; k0 += 16) {
    double a[4], b[4][kNysColTiles];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 4 * kk + u;
      const bool kok = k < R;
      const int kc = kok ? k : R - 1, j = kc / 3, cs = kc - 3 * j;
      const double val = nys_entry<false>(it, v, x0, x1, x2, j, smp[3 * j], smp[3 * j + 1], smp[3 * j + 2], c, cs);
      a[u] = kok && rok ? val : 0.0;
#pragma unroll
      for (int cc = 0; cc < kNysColTiles; ++cc) b[u][cc] = cc < tn ? W[(size_t)k * kp + 16 * cc] : 0.0;  // (W has Rp >= k0 + 16 rows: in range)
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int cc = 0; cc < kNysColTiles; ++cc)
        if (cc < tn) acc[cc] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][cc], acc[cc], 0, 0, 0);
  }
  const global_ptr<double> out = as_global(pc.out);
#pragma unroll
  for (int cc = 0; cc < kNysColTiles; ++cc) {
    if (cc >= tn) continue;
    const int col = 16 * (t0 + cc) + i16;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = row_a + kk + 4 * g;
      if (row < pc.rows && col < rank) out[(size_t)row * rank + col] = acc[cc][g];
    }
  }
}

}  // namespace

void launch_nys_kernel_matrix(hipStream_t st, int n_items, int n_max, const NysItem* items) {
  if (n_items <= 0 || n_max <= 0) return;
  hipLaunchKernelGGL(k_nys_kernel_matrix, dim3(cdiv(n_max * n_max, 256), n_items), dim3(256), 0, st, items);
  hipLaunchKernelGGL(k_nys_norm, dim3(n_items), dim3(256), 0, st, items);
}
void launch_nys_round(hipStream_t st, int n_items, int rp_max, int round, const NysItem* items) {
  if (n_items <= 0) return;
  const int tiles = rp_max / kNysPair;  // (rp_max is a multiple of 64; an item has Rp/64 pairs of blocks and Rp/64 tiles of 64)
  set_dyn_lds((const void*)k_nys_pair, kNysPairLds);
  set_dyn_lds((const void*)k_nys_rows, kNysApplyLds);
  set_dyn_lds((const void*)k_nys_cols, kNysApplyLds);
  hipLaunchKernelGGL(k_nys_pair, dim3(tiles, n_items), dim3(256), kNysPairLds, st, items, round);
  hipLaunchKernelGGL(k_nys_rows, dim3(tiles, tiles, n_items), dim3(256), kNysApplyLds, st, items, round);
  hipLaunchKernelGGL(k_nys_cols, dim3(2 * tiles, tiles, n_items), dim3(256), kNysApplyLds, st, items, round);
}
void launch_nys_sweep_end(hipStream_t st, int n_items, const NysItem* items, int* active_word) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(k_nys_sweep_end, dim3(n_items), dim3(256), 0, st, items, active_word);
}
void launch_nys_finish(hipStream_t st, int n_items, int rp_max, int kp_max, const NysItem* items) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(k_nys_sort, dim3(cdiv(rp_max, 256), n_items), dim3(256), 0, st, items);
  hipLaunchKernelGGL(k_nys_operand, dim3(cdiv(rp_max * kp_max, 256), n_items), dim3(256), 0, st, items);
}
void launch_nys_basis(hipStream_t st, int n_pieces, int rows_max, int col_tiles_max, const NysPiece* pieces) {
  if (n_pieces <= 0) return;
  hipLaunchKernelGGL(k_nys_basis, dim3(cdiv(col_tiles_max, kNysColTiles), cdiv(rows_max, 16), n_pieces), dim3(64), 0, st, pieces);
}

}  // namespace icp
