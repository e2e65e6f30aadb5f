// kernels_eigen.hip — the posterior KL basis: D M⁻¹ D = V S Vᵀ (kernels_posterior.hip's header has the mathematics), everything behind
// launch_posterior_eigen*.
//
// Rank -> route: ranks <= 64 the fixed-position Jacobi kernel k_posterior_eigen_rr (or, opt-in, the Cholesky-root sampler
// k_posterior_root); ranks 65..256 the tridiagonal route (device code: icp_tridiag.hpp) with the in-place Jacobi kernel k_eigen_big
// (ranks <= 200) or the generic kernel k_posterior_eigen as its status-2 fall-back; the generic kernel above.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>

#include "icp_kernels.hpp"
#include "icp_dense.hpp"

namespace icp {

#ifdef ICP_EIGEN_TIMING  // tools/eigen_bench only: phase stamps (100 MHz) of the last eigen kernel
__device__ long long g_eigen_stamps[64];
#define EIG_STAMP(i) do { if (threadIdx.x == 0) g_eigen_stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define EIG_STAMP(i)
#endif
}  // namespace icp
#include "icp_tridiag.hpp"
namespace icp {

namespace {

constexpr int kEigenMaxSweeps = 40;
#ifndef ICP_LOOSE_TAU
#define ICP_LOOSE_TAU 5e-7
#endif
constexpr double kLooseTau = ICP_LOOSE_TAU;  // loose stopping test of the Jacobi kernels (see k_posterior_eigen_rr)

// ---------------------------------------------------------------- posterior KL basis: parallel two-sided Jacobi
// Eigen-decomposition of N = D⁻¹ M D⁻¹ (same eigenvectors as D M⁻¹ D, reciprocal eigenvalues) in one workgroup of
// 1024 threads, matrices in LDS (odd leading dimension).  Round-robin ordering: each round rotates n/2 disjoint
// index pairs concurrently:
//   phase 1: one thread per pair computes (c, s) from three matrix entries (reciprocal/rsqrt seeds + Newton: the
//            f64 division/sqrt expansions would dominate the round), barrier;
//   phase 2: every 2×2 block (rows of pair P1 × columns of pair P2) is transformed as R1ᵀ·B·R2 by ONE thread, so each
//            matrix element is read and written once per round; other threads rotate the column pairs of V; barrier.
// Warm start: if `Vwarm` is given, the iteration starts from Vwarmᵀ N Vwarm (nearly diagonal when Vwarm diagonalised a
// nearby posterior) with V = Vwarm, which cuts the number of sweeps roughly in half; the result is the same
// eigen-decomposition (to rounding) either way.

__global__ void __launch_bounds__(1024) k_posterior_eigen(int r, const double* __restrict__ M, const double* __restrict__ sqrt_lambda,
                                                           const double* __restrict__ Vwarm, double* __restrict__ Vout,
                                                           double* __restrict__ Vtout, double* __restrict__ Sout,
                                                           double* __restrict__ work, int* __restrict__ status, int a_in_lds, int v_in_lds,
                                                           const int* __restrict__ gate = nullptr) {
  __shared__ double s_red[16], s_mu[512], s_sgn[512], s_c[256], s_s[256];
  __shared__ int s_rank[512];
  __shared__ short s_p[256], s_q[256];
  // (as the tridiagonal route's fall-back above rank 200, where the in-place kernel's triangle no longer fits a CU's LDS: runs only if
  // the multisection could not separate the spectrum — status 2)
  if (gate && gate[0] != 2) return;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lda = a_in_lds ? (r | 1) : r, ldv = v_in_lds ? (r | 1) : r;
  double* A = a_in_lds ? s_dyn : work;
  double* V = v_in_lds ? (s_dyn + (a_in_lds ? (size_t)r * lda : 0)) : Vout;
  for (int e = tid; e < r * r; e += nt) {
    const int i = e / r, j = e - i * r;
    const double mij = 0.5 * (M[e] + M[(size_t)j * r + i]);
    A[(size_t)i * lda + j] = mij / (sqrt_lambda[i] * sqrt_lambda[j]);
    V[(size_t)i * ldv + j] = Vwarm ? Vwarm[e] : (i == j ? 1.0 : 0.0);
  }
  __syncthreads();
  if (Vwarm) {
    // A <- Vᵀ A V in two passes through `work` (T = A V, then A = Vᵀ T); `work` is free when A lives in LDS,
    // otherwise the warm start is skipped by the launcher.
    for (int e = tid; e < r * r; e += nt) {
      const int i = e / r, j = e - i * r;
      double s = 0.0;
      for (int k = 0; k < r; ++k) s = fma(A[(size_t)i * lda + k], V[(size_t)k * ldv + j], s);
      work[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < r * r; e += nt) {
      const int i = e / r, j = e - i * r;
      double s = 0.0;
      for (int k = 0; k < r; ++k) s = fma(V[(size_t)k * ldv + i], work[(size_t)k * r + j], s);
      A[(size_t)i * lda + j] = s;
    }
    __syncthreads();
    for (int e = tid; e < r * r; e += nt) {  // symmetrise against rounding
      const int i = e / r, j = e - i * r;
      if (i < j) {
        const double v = 0.5 * (A[(size_t)i * lda + j] + A[(size_t)j * lda + i]);
        A[(size_t)i * lda + j] = v;
        A[(size_t)j * lda + i] = v;
      }
    }
    __syncthreads();
  }
  const int n2 = (r + 1) & ~1, half = n2 >> 1, mm = n2 - 1;
  // work items of a round: n_blocks 2×2 blocks of A (upper triangle of the pair×pair grid, mirrored) + r·half column
  // pairs of V.  Item -> thread mapping is fixed, so everything but the pair's current (p,q) is precomputed.
  const int n_blocks = half * (half + 1) / 2, n_items = n_blocks + r * half;
  constexpr int kItems = 2;  // items with precomputed descriptors; more (large ranks) go through the generic loop
  int it_a[kItems], it_b[kItems];  // block item: (P1 <= P2); V item: (k | 0x40000000, P)
#pragma unroll
  for (int m = 0; m < kItems; ++m) {
    const int w = tid + nt * m;
    it_a[m] = -1; it_b[m] = 0;
    if (w < n_blocks) {  // unrank the upper triangle row-major: P1 <= P2
      int P1 = 0, base = 0;
      while (base + (half - P1) <= w) { base += half - P1; ++P1; }
      it_a[m] = P1; it_b[m] = P1 + (w - base);
    } else if (w < n_items) {
      const int vi = w - n_blocks;
      it_a[m] = (vi / half) | 0x40000000; it_b[m] = vi % half;
    }
  }
  // round-robin state of the pair this thread computes in phase 1 (slot = tid): incremental, no modulo per round
  int ra = 0, rb = 0;
  if (tid < half) {
    if (tid == 0) { ra = mm; rb = 0; }
    else { ra = tid % mm; rb = (mm - tid) % mm; }
  }
  auto do_block = [&](int P1, int P2) {
    const int p1 = s_p[P1], q1 = s_q[P1], p2 = s_p[P2], q2 = s_q[P2];
    const double c1 = s_c[P1], s1 = s_s[P1], c2 = s_c[P2], s2 = s_s[P2];
    const bool hq1 = q1 < r, hq2 = q2 < r;
    const int opp = p1 * lda + p2, opq = p1 * lda + q2, oqp = q1 * lda + p2, oqq = q1 * lda + q2;
    const double bpp = A[opp];
    const double bpq = hq2 ? A[opq] : 0.0;
    const double bqp = hq1 ? A[oqp] : 0.0;
    const double bqq = (hq1 && hq2) ? A[oqq] : 0.0;
    // rows (pair P1): [p; q] <- [c −s; s c][p; q];  columns (pair P2): [p q] <- [p q][c s; −s c]
    const double tpp = c1 * bpp - s1 * bqp, tpq = c1 * bpq - s1 * bqq;
    const double tqp = s1 * bpp + c1 * bqp, tqq = s1 * bpq + c1 * bqq;
    const double npp = c2 * tpp - s2 * tpq, npq = s2 * tpp + c2 * tpq;
    const double nqp = c2 * tqp - s2 * tqq, nqq = s2 * tqp + c2 * tqq;
    A[opp] = npp;
    if (hq2) A[opq] = npq;
    if (hq1) A[oqp] = nqp;
    if (hq1 && hq2) A[oqq] = nqq;
    if (P1 != P2) {  // mirror block (A stays exactly symmetric)
      A[p2 * lda + p1] = npp;
      if (hq2) A[q2 * lda + p1] = npq;
      if (hq1) A[p2 * lda + q1] = nqp;
      if (hq1 && hq2) A[q2 * lda + q1] = nqq;
    }
  };
  auto do_vpair = [&](int k, int P) {
    const int p = s_p[P], q = s_q[P];
    if (q < r) {
      const double c = s_c[P], s = s_s[P];
      const int op = k * ldv + p, oq = k * ldv + q;
      const double vkp = V[op], vkq = V[oq];
      V[op] = c * vkp - s * vkq;
      V[oq] = s * vkp + c * vkq;
    }
  };
  int converged = 0, n_sweeps = 0;
  for (int sweep = 0; sweep < 40 && !converged; ++sweep) {
    for (int rnd = 0; rnd < mm; ++rnd) {
      if (tid < half) {
        const int p = ra < rb ? ra : rb, q = ra < rb ? rb : ra;
        double c = 1.0, s = 0.0;
        if (q < r) {
          const double apq = A[p * lda + q], app = A[p * lda + p], aqq = A[q * lda + q];
          if (fabs(apq) > 1e-300 && apq * apq > 1e-36 * fabs(app * aqq)) {
            // t = sgn(a)·b / (|a| + sqrt(a² + b²)),  a = (aqq − app)/2, b = apq  (smaller root of t² + 2τt − 1 = 0)
            const double a = 0.5 * (aqq - app);
            const double h2 = fma(a, a, apq * apq);
            const double h = h2 * fast_rsqrt(h2);
            const double t = (a >= 0.0 ? apq : -apq) * fast_rcp(fabs(a) + h);
            c = fast_rsqrt(fma(t, t, 1.0));
            s = t * c;
          }
        }
        s_p[tid] = (short)p; s_q[tid] = (short)q; s_c[tid] = c; s_s[tid] = s;
        // next round's pair of this slot (circle method: every player but the fixed one advances by one seat)
        if (tid == 0) { rb = rb + 1 == mm ? 0 : rb + 1; }
        else { ra = ra + 1 == mm ? 0 : ra + 1; rb = rb + 1 == mm ? 0 : rb + 1; }
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < kItems; ++m) {
        if (it_a[m] >= 0) {
          if (it_a[m] & 0x40000000) do_vpair(it_a[m] & 0x3FFFFFFF, it_b[m]);
          else do_block(it_a[m], it_b[m]);
        }
      }
      for (int w = tid + nt * kItems; w < n_items; w += nt) {  // large ranks only
        if (w < n_blocks) {
          int P1 = 0, base = 0;
          while (base + (half - P1) <= w) { base += half - P1; ++P1; }
          do_block(P1, P1 + (w - base));
        } else {
          const int vi = w - n_blocks;
          do_vpair(vi / half, vi % half);
        }
      }
      __syncthreads();
    }
    double off = 0.0, dg = 0.0;
    for (int e = tid; e < r * r; e += nt) {
      const int i = e / r, j = e - i * r;
      const double v = A[(size_t)i * lda + j];
      if (i == j) dg = fma(v, v, dg);
      else off = fma(v, v, off);
    }
    off = block_sum(off, s_red);
    dg = block_sum(dg, s_red);
    converged = off <= 1e-26 * dg;
    n_sweeps = sweep + 1;
  }
  if (tid == 0) { status[0] = converged ? 0 : 2; status[-1] = n_sweeps; }
  // eigenvalues of D M⁻¹ D are 1/μ; S descending = μ ascending (ties: lower original index first)
  for (int i = tid; i < r; i += nt) s_mu[i] = A[(size_t)i * lda + i];
  __syncthreads();
  for (int i = tid; i < r; i += nt) {
    int rank = 0;
    const double mi = s_mu[i];
    for (int j = 0; j < r; ++j) rank += (s_mu[j] < mi) || (s_mu[j] == mi && j < i);
    s_rank[i] = rank;
    int best = 0;  // canonical sign: the largest-|.| component of each eigenvector is positive
    double bv = fabs(V[i]);
    for (int k = 1; k < r; ++k) {
      const double a = fabs(V[(size_t)k * ldv + i]);
      if (a > bv) { bv = a; best = k; }
    }
    s_sgn[i] = V[(size_t)best * ldv + i] < 0.0 ? -1.0 : 1.0;
    Sout[rank] = 1.0 / mi;
  }
  __syncthreads();
  if (!v_in_lds) {  // V aliases Vout: permute through `work` (free if A sat in LDS; otherwise A lived there and is dead now)
    for (int e = tid; e < r * r; e += nt) work[e] = V[e];
    __syncthreads();
    V = work;
  }
  for (int e = tid; e < r * r; e += nt) {
    const int k = e / r, i = e - k * r;
    const double v = V[(size_t)k * ldv + i] * s_sgn[i];
    Vout[(size_t)k * r + s_rank[i]] = v;
    Vtout[(size_t)s_rank[i] * r + k] = v;
  }
}

// ---------------------------------------------------------------- posterior KL basis, ranks <= 64: fixed-position Jacobi
// Same method (cyclic two-sided Jacobi, round-robin pairing, warm start) re-laid for the LDS pipe, which bounds the kernel
// above: there every round gathers its pair indices and rotation parameters through dependent LDS reads and touches each
// matrix element with scalar 8-byte accesses.  Here the PAIRING never changes — pair K always sits at positions (2K, 2K+1)
// — and the matrix itself is permuted by the round-robin rotation while it is written back (Brent–Luk style), so
//   * every thread reads and writes the SAME addresses every round (all offsets precomputed in registers);
//   * the two elements of a pair are adjacent: one 16-byte read fetches both;
//   * A and V are double-buffered (read `cur`, write the permuted result to `nxt`): ONE barrier per round;
//   * the rotation of a pair of the NEXT round is computed in the same round by a dedicated thread, from the three
//     transformed entries it needs (evaluated with the expressions the block threads use, so both agree bit for bit).
// A is kept exactly symmetric (block (J,I) is computed as the transpose of block (I,J) by the same arithmetic).  An odd
// rank is padded with a dummy index (zero row/column, diagonal 1e300): its rotations are identities.

__device__ __forceinline__ int rr_dst(int pos, int m) {  // where the content of position `pos` goes after a round
  const int k = pos >> 1;
  if ((pos & 1) == 0) return k == 0 ? 0 : (k == m - 1 ? 2 * (m - 1) + 1 : 2 * (k + 1));
  return k == 0 ? 2 : 2 * (k - 1) + 1;
}
__device__ __forceinline__ int rr_src(int pos, int m) {  // inverse of rr_dst
  const int k = pos >> 1;
  if ((pos & 1) == 0) return k == 0 ? 0 : (k == 1 ? 1 : 2 * (k - 1));
  return k == m - 1 ? 2 * (m - 1) : 2 * (k + 1) + 1;
}

struct Rot { double c, s; };

// Rotation (nearly) annihilating apq, branch free; the dependent chain is two reciprocal square roots and no division:
//   a = aqq − app, b = 2·apq (the angle depends on their ratio only), h ≈ sqrt(a² + b²), u = h + |a|:
//   c = u/sqrt(u² + b²), s = sgn(a)·b/sqrt(u² + b²)          (t = s/c = sgn(a)·b/(|a| + h), the smaller root)
// c² + s² = 1 holds to rounding for ANY h, so h comes from the bare hardware seed (relative error 5e-8): the rotated
// off-diagonal entry is then 5e-8·apq instead of 0, which the next sweep removes — the callers store the computed entry,
// never an assumed zero.
__device__ __forceinline__ Rot jacobi_rotation(double app, double apq, double aqq) {
  const double a = aqq - app, b = apq + apq, b2 = b * b;
  const bool rot = apq * apq > 1e-36 * fabs(app * aqq);  // false for zero / underflowing entries and for the dummy index
  const double h2 = fma(a, a, b2);
  const double h = h2 * __builtin_amdgcn_rsq(h2);
  const double u = h + fabs(a);
  const double w = fma(u, u, b2);
  // 1/sqrt(w): seed (5e-8) and one third-order step, y·(1 + e + 1.5e²) with e = ½ − ½w·y²: error ~e³
  const double y0 = __builtin_amdgcn_rsq(w);
  const double e = fma(-(0.5 * w) * y0, y0, 0.5);
  const double y = fma(y0, e * fma(1.5, e, 1.0), y0);
  Rot R;
  R.c = rot ? u * y : 1.0;            // not rotating (negligible or zero entry, dummy index): NaN/inf above are discarded
  R.s = rot ? (a >= 0.0 ? b : -b) * y : 0.0;
  return R;
}

struct B22 { double a00, a01, a10, a11; };

// R1ᵀ·B·R2 with R = [c s; −s c]
__device__ __forceinline__ B22 rot_block(B22 b, double c1, double s1, double c2, double s2) {
  const double t00 = fma(c1, b.a00, -(s1 * b.a10)), t01 = fma(c1, b.a01, -(s1 * b.a11));
  const double t10 = fma(s1, b.a00, c1 * b.a10), t11 = fma(s1, b.a01, c1 * b.a11);
  return B22{fma(c2, t00, -(s2 * t01)), fma(s2, t00, c2 * t01), fma(c2, t10, -(s2 * t11)), fma(s2, t10, c2 * t11)};
}
typedef double dbl2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ dbl2 lds2(const double* p) { return *(const dbl2*)p; }

// Work split of one round (1024 threads launched; ranks <= 64).  Only the upper triangle of A is stored: element {R, C}
// lives at [min][max], so every element is written once per round and no mirror is kept.
//   wave 3         lane K prepares the rotation of pair K of the next round — the longest dependent chain of a round; it
//                  has its SIMD (waves 3, 7, 11, 15) to itself — and appends it to the rotation log in global memory
//   block waves    (0-2, 4-6, …) one 2×2 block (I <= J) of A per thread: read, rotate, write to the permuted places
// The rotation table holds R = [c s; −s c] column by column, [c, −s | s, c] per pair, so that a thread that needs column
// `side` of a pair's rotation reads it with one 16-byte load at a precomputed offset (no selects on the critical chain).
// V is not touched inside the loop: its 2·r·n2 stores per round cost more than the whole round (measured: ≥ 500 cycles
// of LDS time per round on one CU in every layout tried, against a ~1000-cycle round).  The rotations are logged instead,
// and k_eigen_vreplay applies them to V afterwards on many CUs at once (rows of V are independent).

// ---- progress word shared by the two roles of k_posterior_eigen_rr (meta[0]); every launch carries its own id so that
// whatever an earlier launch left there is never mistaken for news
constexpr int kPwRoundsMask = 0x3FFFF, kPwAbort = 1 << 18, kPwFinished = 1 << 19, kPwIdShift = 20, kPwIdMask = 0x7FF;
__device__ __forceinline__ void progress_publish(int* meta, int id, int rounds, int flags) {
  // no fence: everything the word announces (rotation log, final diagonal, correction) is written with write-through
  // stores that the storing waves have waited for (s_waitcnt vmcnt(0), then the workgroup's barrier) before this store
  __hip_atomic_store(meta, (id << kPwIdShift) | flags | rounds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// whole-wave shifts by one lane on the DPP path of the VALU (gfx9 wave_shr:1 / wave_shl:1): no LDS crossbar trip
__device__ __forceinline__ double wave_shr1_f64(double v) {  // lane l receives the value of lane l−1 (lane 0 keeps its own)
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), 0x138, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), 0x138, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_shl1_f64(double v) {  // lane l receives the value of lane l+1 (lane 63 keeps its own)
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), 0x130, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), 0x130, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// ---------------------------------------------------------------- V <- V·J_0·J_1···  (replay of the rotation log)
// Workgroups 1.. of a problem of k_posterior_eigen_rr (one per 32 rows of V), running BESIDE its Jacobi workgroup
// (workgroup 0) on other CUs: they follow the progress word — the producer's log wave advances it every round, a few
// rounds behind its write-through stores — and apply the rotations to the eigenvector matrix while the iteration goes on,
// so that when it ends only a handful of rounds, the first-order correction and the final sort are left.
// One wave per FOUR coordinates (rows of V): lane = pair + 32·(row pair), two rows per lane, 8 row-carrying waves per
// workgroup (one CU cannot keep pace with the iteration for all 64 rows: ≈ 60 cycles per row and round).  A lane keeps its
// pair's two entries of each row in registers; one round rotates the pair and hands the results to the neighbouring pairs
// (the round-robin move: first entries travel to pair+1, second entries to pair−1, with the two turn-arounds at the
// ends): two 64-bit DPP wave shifts per row and round, no LDS traffic for the data.  The rotations of the published
// rounds are staged in LDS once per pass.  At the end every workgroup applies the correction V <- V·(I + X) (see
// k_posterior_eigen_rr) to its rows, ranks the eigenvalues, and the two workgroups exchange, per column, their
// largest-|.| candidate (one 1-KB message each, write-through stores and a flag) to fix the signs — largest-|.| component
// of every eigenvector positive, the first among equals — before every lane writes its own entries of V and Vᵀ.
constexpr int kReplayStageRounds = 64;   // rounds staged per pass (>= one sweep for ranks <= 64)
constexpr int kReplayWaves = 8;          // waves of a replay workgroup that carry rows (the others help with staging)
constexpr int kReplayRows = 4 * kReplayWaves;  // rows of V per replay workgroup
constexpr int kEigMetaCorr = 7;          // meta word: the producer left a first-order correction X in `xcorr`
constexpr int kEigMetaMu = 64;           // (double*)meta + this: the final diagonal, by position
constexpr int kEigMetaXchg = 128;        // (double*)meta + this: [2 workgroups][64 values | 64 rows] sign candidates

constexpr unsigned long long kEigenWaitTicks = 500000;  // 5 ms of s_memrealtime (100 MHz): the bound of every device-side wait here
constexpr int kPwGaveUp = (int)0x80000000;     // never published: a replay workgroup's own mark on the word it acts on

__device__ __forceinline__ void sc1_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double sc1_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A replay workgroup that waited in vain: the host learns it from the pinned status and repeats the decomposition the ordinary way
// (chain_step_record), and the basis that was never written is marked so that no later decomposition takes it for a warm start
__device__ __forceinline__ void eigen_replay_gave_up(int* host_status, double* Vout) {
  if (host_status) __hip_atomic_store(host_status, kEigenGaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  Vout[0] = __builtin_nan("");
}

__device__ void eigen_replay_consumer(int r, const double* Vwarm, const double* rotlog, int* meta, const double* xcorr /* [n2][n2] */,
                                      double* Vout, double* Vtout, double* Sout, int launch_id, int me, int nb, int* done_word,
                                      int done_value, int* host_status, bool awaits_input) {
  __shared__ int s_pw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n2 = (r + 1) & ~1, m = n2 >> 1;
  double* s_log = s_dyn;  // kReplayStageRounds × m entries of (c, −s)
  const int kc = lane >> 5, q = lane & 31, ka = kReplayRows * me + 4 * wave + 2 * kc, kb = ka + 1;
  const bool carry = wave < kReplayWaves && kReplayRows * me + 4 * wave < r;  // (uniform) this wave holds rows of V
  const bool act = q < m && carry;
  const int qc = q < m ? q : 0;
  // this lane's pair of each of its two rows: positions 2q (first) and 2q+1 (second)
  auto v0_at = [&](int k, int p) { return (k < r && p < r) ? (Vwarm ? Vwarm[(size_t)k * r + p] : (k == p ? 1.0 : 0.0)) : 0.0; };
  double a0 = act ? v0_at(ka, 2 * q) : 0.0, a1 = act ? v0_at(ka, 2 * q + 1) : 0.0;
  double b0 = act ? v0_at(kb, 2 * q) : 0.0, b1 = act ? v0_at(kb, 2 * q + 1) : 0.0;
  int done = 0;
  bool aborted = false;
  for (;;) {
    if (tid == 0) {  // follow the producer (relaxed polls: an acquiring load would invalidate this CU's L1 every time round)
      // No news for 5 ms (the producer publishes every few rounds, a few µs apart) — twice that before the first news of a launch
      // whose producer may itself wait 5 ms for its input: the decomposition is dropped as if it had been aborted, and the
      // pinned status says so (see eigen_replay_gave_up)
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime(), limit = (awaits_input && done == 0) ? 2 * kEigenWaitTicks : kEigenWaitTicks;
      int pw;
      for (;;) {
        pw = __hip_atomic_load(meta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (((pw >> kPwIdShift) & kPwIdMask) == launch_id && ((pw & kPwRoundsMask) > done || (pw & (kPwAbort | kPwFinished)))) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > limit) { pw = kPwAbort | kPwGaveUp; break; }
        __builtin_amdgcn_s_sleep(2);
      }
      s_pw = pw;
#ifdef ICP_EIGEN_TIMING
      if (me == 0 && (pw & kPwFinished)) g_eigen_stamps[40] = __builtin_amdgcn_s_memrealtime();
#endif
    }
    __syncthreads();
    const int pw = s_pw;
    if (pw & kPwAbort) {  // cancelled decomposition: V stays untouched
      aborted = true;
      if ((pw & kPwGaveUp) && tid == 0) eigen_replay_gave_up(host_status, Vout);
      break;
    }
    const int avail = pw & kPwRoundsMask;
    while (done < avail) {
      const int n = min(avail - done, kReplayStageRounds);
      // (the log is written with write-through stores and read with loads served by L2: its addresses are reused by every
      // decomposition, a plain load could hit a stale line of this CU's L1; the word is advanced behind the stores' return)
      for (int e = tid; e < 2 * n * m; e += blockDim.x) s_log[e] = sc1_load(rotlog + 2 * (size_t)done * m + e);
      __syncthreads();
      if (carry) {
        for (int rl = 0; rl < n; rl += 8) {
          dbl2 cs[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) cs[u] = *(const dbl2*)&s_log[2 * (min(rl + u, n - 1) * m + qc)];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (rl + u < n) {  // uniform
              // rotated first / second entry of both rows
              const double fa = fma(cs[u].x, a0, cs[u].y * a1), ga = fma(-cs[u].y, a0, cs[u].x * a1);
              const double fb = fma(cs[u].x, b0, cs[u].y * b1), gb = fma(-cs[u].y, b0, cs[u].x * b1);
              // round-robin move (rr_dst): first entries go one pair up, except pair 0 (stays) and pair m−1 (becomes its
              // own second); second entries go one pair down, except pair 0 (becomes the first of pair 1)
              const double ua = wave_shr1_f64(q == 0 ? ga : fa), da = wave_shl1_f64(ga);
              const double ub = wave_shr1_f64(q == 0 ? gb : fb), db = wave_shl1_f64(gb);
              a0 = q == 0 ? fa : ua; a1 = q == m - 1 ? fa : da;
              b0 = q == 0 ? fb : ub; b1 = q == m - 1 ? fb : db;
            }
          }
        }
      }
      __syncthreads();
      done += n;
    }
    if (pw & kPwFinished) break;
  }
#ifdef ICP_EIGEN_TIMING
  if (me == 0 && tid == 0) g_eigen_stamps[41] = __builtin_amdgcn_s_memrealtime();
#endif
  // ---- correction, ranks, signs, output
  double* s_x = s_dyn;                       // [n2][n2] first-order correction (the log's region: every wave is past it)
  double* s_mu = s_dyn + 4096;               // [64] final diagonal by position
  int* s_rank = (int*)(s_dyn + 4096 + 64);   // [64]
  double* s_bv = s_dyn + 4096 + 128;         // [64] signed winner per position
  int* s_bk = (int*)(s_dyn + 4096 + 192);    // [64] … and its row
  double* s_pv = s_dyn + 4096 + 256;         // [8 waves][64 positions] candidate value (signed)
  int* s_pk = (int*)(s_dyn + 4096 + 256 + kReplayWaves * 64);  // … and its row
  // s_dyn[5632 …): [32 rows][64 positions] the workgroup's rows, for the correction
  double* xchg = (double*)meta + kEigMetaXchg;
  if (!aborted) {
    const int has_corr = __hip_atomic_load(meta + kEigMetaCorr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < n2) s_mu[tid] = sc1_load((const double*)meta + kEigMetaMu + tid);
    if (has_corr)
      for (int e = tid; e < n2 * n2; e += blockDim.x) s_x[e] = sc1_load(xcorr + e);
    __syncthreads();
    if (has_corr) {  // row·(I + X): entry p of a row gains Σ_i row[i]·X[i][p].  The rows go through LDS (every lane then reads
      // the SAME two entries of its row — a broadcast — beside its own two columns of X): a quarter of the LDS cycles of
      // fetching the entries from their lanes by shuffles, which is what this step is bound by
      if (act) {
        *(dbl2*)&s_dyn[5632 + (4 * wave + 2 * kc) * 64 + 2 * q] = dbl2{a0, a1};
        *(dbl2*)&s_dyn[5632 + (4 * wave + 2 * kc + 1) * 64 + 2 * q] = dbl2{b0, b1};
      }
      __syncthreads();
      if (carry) {
        double ca0 = 0.0, ca1 = 0.0, cb0 = 0.0, cb1 = 0.0;
        const int ra = 5632 + (4 * wave + 2 * kc) * 64, rb = ra + 64;
        for (int i = 0; i < n2; i += 2) {
          const dbl2 va = *(const dbl2*)&s_dyn[ra + i], vb = *(const dbl2*)&s_dyn[rb + i];
          const dbl2 xe = *(const dbl2*)&s_dyn[i * n2 + 2 * qc], xo = *(const dbl2*)&s_dyn[(i + 1) * n2 + 2 * qc];
          ca0 = fma(va.x, xe.x, ca0); ca1 = fma(va.x, xe.y, ca1); cb0 = fma(vb.x, xe.x, cb0); cb1 = fma(vb.x, xe.y, cb1);
          ca0 = fma(va.y, xo.x, ca0); ca1 = fma(va.y, xo.y, ca1); cb0 = fma(vb.y, xo.x, cb0); cb1 = fma(vb.y, xo.y, cb1);
        }
        if (act) { a0 += ca0; a1 += ca1; b0 += cb0; b1 += cb1; }
      }
    }
    // sign candidates per position: largest |.| over the rows, the lowest row among equals
    if (wave < kReplayWaves) {
      const bool va = act && ka < r, vb = act && kb < r;
      double m0 = va ? fabs(a0) : -1.0, m1 = va ? fabs(a1) : -1.0, c0 = a0, c1 = a1;
      int k0 = ka, k1 = ka;
      if (vb && fabs(b0) > m0) { m0 = fabs(b0); c0 = b0; k0 = kb; }
      if (vb && fabs(b1) > m1) { m1 = fabs(b1); c1 = b1; k1 = kb; }
      const double o0 = __shfl_xor(m0, 32, 64), o1 = __shfl_xor(m1, 32, 64), w0 = __shfl_xor(c0, 32, 64), w1 = __shfl_xor(c1, 32, 64);
      const int ok0 = __shfl_xor(k0, 32, 64), ok1 = __shfl_xor(k1, 32, 64);
      if (o0 > m0 || (o0 == m0 && ok0 < k0)) { m0 = o0; c0 = w0; k0 = ok0; }
      if (o1 > m1 || (o1 == m1 && ok1 < k1)) { m1 = o1; c1 = w1; k1 = ok1; }
      if (lane < 32 && q < m) {
        s_pv[wave * 64 + 2 * q] = m0 < 0.0 ? 0.0 : c0; s_pk[wave * 64 + 2 * q] = m0 < 0.0 ? 0x7fffffff : k0;
        s_pv[wave * 64 + 2 * q + 1] = m1 < 0.0 ? 0.0 : c1; s_pk[wave * 64 + 2 * q + 1] = m1 < 0.0 ? 0x7fffffff : k1;
      }
    }
    __syncthreads();
    if (tid < n2) {
      double bv = s_pv[tid];
      int bk = s_pk[tid];
      for (int w = 1; w < kReplayWaves; ++w) {
        const double v = s_pv[w * 64 + tid];
        const int kk = s_pk[w * 64 + tid];
        if (kk != 0x7fffffff && (bk == 0x7fffffff || fabs(v) > fabs(bv) || (fabs(v) == fabs(bv) && kk < bk))) { bv = v; bk = kk; }
      }
      s_bv[tid] = bv; s_bk[tid] = bk;
      if (nb > 1) { sc1_store(xchg + me * 128 + tid, bv); sc1_store(xchg + me * 128 + 64 + tid, (double)bk); }
      // eigenvalues of D M⁻¹ D are 1/μ; S descending = μ ascending (ties: lower position first); the dummy sorts last
      int rank = 0;
      const double mi = s_mu[tid];
      for (int j = 0; j < n2; ++j) rank += (s_mu[j] < mi) || (s_mu[j] == mi && j < tid);
      s_rank[tid] = rank;
      if (me == 0 && rank < r) sc1_store(Sout + rank, 1.0 / mi);
    }
    bool lost = false;  // the other workgroup never came to the exchange (it gave up on the producer at the last moment)
    if (nb > 1) {  // exchange with the other workgroup: message out (write-through, drained), flag up; its flag, its message
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const int o = 1 - me;
      if (tid == 0) {
        __hip_atomic_store(meta + 2 + me, launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(meta + 2 + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != launch_id) {
          if (__builtin_amdgcn_s_memrealtime() - t0 > kEigenWaitTicks) { s_pw = kPwAbort | kPwGaveUp; break; }
          __builtin_amdgcn_s_sleep(1);
        }
      }
      __syncthreads();
      lost = (s_pw & kPwGaveUp) != 0;
      if (lost && tid == 0) eigen_replay_gave_up(host_status, Vout);
      if (tid < n2 && !lost) {
        const double v = sc1_load(xchg + o * 128 + tid);
        const int kk = (int)sc1_load(xchg + o * 128 + 64 + tid);
        double bv = s_bv[tid];
        const int bk = s_bk[tid];
        if (kk != 0x7fffffff && (bk == 0x7fffffff || fabs(v) > fabs(bv) || (fabs(v) == fabs(bv) && kk < bk))) bv = v;
        s_bv[tid] = bv;
      }
      if (tid == 0) __hip_atomic_store(meta + 2 + o, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // read: back to idle (ids repeat after 2047 launches)
    }
    __syncthreads();
    if (act && !lost) {  // (write-through stores: nothing to write back before the completion word)
      const int p0 = 2 * q, p1 = 2 * q + 1, r0 = s_rank[p0], r1 = s_rank[p1];
      const bool n0 = s_bv[p0] < 0.0, n1 = s_bv[p1] < 0.0;
      if (ka < r) {
        if (r0 < r) { const double v = n0 ? -a0 : a0; sc1_store(Vout + (size_t)ka * r + r0, v); sc1_store(Vtout + (size_t)r0 * r + ka, v); }
        if (r1 < r) { const double v = n1 ? -a1 : a1; sc1_store(Vout + (size_t)ka * r + r1, v); sc1_store(Vtout + (size_t)r1 * r + ka, v); }
      }
      if (kb < r) {
        if (r0 < r) { const double v = n0 ? -b0 : b0; sc1_store(Vout + (size_t)kb * r + r0, v); sc1_store(Vtout + (size_t)r0 * r + kb, v); }
        if (r1 < r) { const double v = n1 ? -b1 : b1; sc1_store(Vout + (size_t)kb * r + r1, v); sc1_store(Vtout + (size_t)r1 * r + kb, v); }
      }
    }
  }
#ifdef ICP_EIGEN_TIMING
  if (me == 0 && tid == 0) g_eigen_stamps[42] = __builtin_amdgcn_s_memrealtime();
#endif
  // every wave's (write-through) stores have left before the workgroup is counted out; the last workgroup out puts the
  // shared words back to idle and raises the completion word
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    if (nb == 1 || __hip_atomic_fetch_add(meta + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nb - 1) {
      __hip_atomic_store(meta + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(meta, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (the producer has long finished; nobody reads it any more)
      // this decomposition is complete (or dropped): whoever waits for it alone need not wait for the rest of the launch
      if (done_word) __hip_atomic_store(done_word, done_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

constexpr int kRrLd = 66;                 // row stride of A (doubles): rows 16 B apart modulo the 256-B bank window
constexpr int kRrSzA = 64 * kRrLd;        // one buffer of A, sized for rank 64 whatever r is: every offset below is a constant
constexpr int kRrSzC = 4 * 32;            // one rotation table
constexpr int kRrOC = 0, kRrOA = 2 * kRrSzC, kRrOV = kRrOA + 2 * kRrSzA;  // table[2] | A[2] | Vt (warm start) | T (its transform)
constexpr int kRrLogWave = 14;            // never a block wave (at most 9 of those, on waves 0-2, 4-6, 8-10)
constexpr int kRrPollWave = 13;           // … nor this one: a speculative decomposition's cancel word is polled here (a slow read of
                                          // pinned memory, which must not sit in the log wave's memory queue: it counts its stores)
constexpr int kRrLogLag = 8;              // the progress word trails the log wave's write-through stores by this many rounds
template <int N> struct IntC { static constexpr int value = N; };

// One launch decomposes up to four posteriors side by side (the two ICP directions of a chain step; of both lanes of a twin pass:
// EigenBatch<4>): problem p owns the workgroups [p·per, (p+1)·per), the first of which iterates while the others replay.
// (struct EigenProblem: icp_kernels.hpp — the on-device chain loop patches these records in device memory)
// The batch record.  EigenBatch<2>: the two directions of one chain step, by value in the kernel arguments.  EigenBatchMem: the
// decompositions of a batch of chains (icp_chain_step_batched) — any number of them in ONE launch, the records read in place from
// pinned host memory (136 bytes per workgroup, once); every workgroup announces itself in `arrive` when it starts, so that the
// batch's launch sequence can be held back until all of them are resident (k_step_batch_args: its first launch fills the chip with
// workgroups that spin on these decompositions' completion words, and must not get there first).
template <int CAP> struct EigenBatch {
  int n; EigenProblem p[CAP];
  __device__ __forceinline__ void announce() const {}
  __device__ __forceinline__ bool skipped(int) const { return false; }
};
struct EigenBatchMem {
  int n; const EigenProblem* p; int* arrive;
  const int* skip = nullptr;  // (optional) skip[problem] != 0: nothing to decompose this time (the on-device chain loop launches the
                              // decompositions of every chain every step; only the chains that moved have one)
  __device__ __forceinline__ void announce() const {
    if (arrive && threadIdx.x == 0) __hip_atomic_fetch_add(arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ bool skipped(int which) const { return skip != nullptr && skip[which] != 0; }
};
static_assert(sizeof(EigenBatch<kEigenPairMax>) + 64 <= 4096, "the batch record must fit the kernel argument segment");

template <class Batch>
__global__ void __launch_bounds__(1024) k_posterior_eigen_rr(int r, const double* __restrict__ sqrt_lambda_launch, int ldk, int max_sweeps,
                                                              int no_corr /* 1: sweep to the strict test (A/B, tests) */, Batch batch) {
  batch.announce();
  const int per = 1 + (r + kReplayRows - 1) / kReplayRows;  // workgroups per problem: the iteration + the replay (32 rows each)
  const int which = (int)blockIdx.x / per, local = (int)blockIdx.x - which * per;
  if (batch.skipped(which)) return;  // (uniform per workgroup)
  const EigenProblem pb = batch.p[which];
  const double* __restrict__ sqrt_lambda = pb.sqrt_lambda ? pb.sqrt_lambda : sqrt_lambda_launch;
  const double* __restrict__ M = pb.M;
  const double* Vwarm = pb.Vwarm;
  double* Vout = pb.Vout;
  double* Vtout = pb.Vtout;
  double* __restrict__ Sout = pb.Sout;
  int* __restrict__ status = pb.status;
  double* rotlog = pb.rotlog;
  int* meta = pb.meta;
  double* vpos = pb.vpos;
  const EigenSpec spec = pb.spec;
  const int launch_id = pb.launch_id;
  int* host_status = pb.host_status;
  if (Vwarm && !(Vwarm[0] == Vwarm[0])) Vwarm = nullptr;  // the basis of a decomposition that gave up (see below): cold start
  if (local != 0) {
    eigen_replay_consumer(r, Vwarm, rotlog, meta, vpos, Vout, Vtout, Sout, launch_id, local - 1, per - 1, pb.done_word, pb.done_value,
                          host_status, spec.ready != nullptr);
    return;
  }
  __shared__ double s_red[16], s_red2[16];
  __shared__ int s_cancel, s_bad[16];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int n2 = (r + 1) & ~1, m = n2 >> 1;
  // buffers are addressed as s_dyn[offset] with integer offsets: a table of pointers would turn every access into a
  // FLAT instruction (address space lost), several times slower than the DS path.  The offsets of the round loop are
  // compile-time constants plus one per-thread register, so they fold into the DS instructions' immediate fields.
  constexpr int ld = kRrLd, szA = kRrSzA, szC = kRrSzC, oA = kRrOA, oV = kRrOV, oC = kRrOC;
  const int szV = n2 * ldk, oT = oV + szV;
#define LDS_A(b, i) s_dyn[oA + (b) * szA + (i)]
#define LDS_VT(i) s_dyn[oV + (i)]
#define LDS_T(i) s_dyn[oT + (i)]
#define LDS_C(b, i) s_dyn[oC + (b) * szC + (i)]
  EIG_STAMP(0);
  // a speculative decomposition polls its cancel word (pinned host memory: a slow read, so one thread of an otherwise
  // idle wave fetches it while the others work, and the block looks at the copy at the next convenient barrier)
  const bool is_poll = spec.cancel != nullptr && tid == 64 * kRrPollWave + 63;
  if (tid == 0) s_cancel = 0;
  // (the first look at the word is issued here and used behind the staging below: a launch that starts after it was cancelled —
  // the eigen stream was busy — leaves without a wait)
  int polled = 0x80000000;
  if (is_poll) polled = __hip_atomic_load(spec.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // ---- N = D⁻¹ M D⁻¹ (symmetrised), padded; Vt = (warm start or identity)ᵀ, padded with zeros
  for (int e = tid; e < szV; e += nt) LDS_VT(e) = 0.0;
  __syncthreads();
  // ---- fixed work of this thread (indices only: nothing here depends on the matrix, so a speculative launch does it —
  // and the staging of the warm-start basis — while it still waits for its input)
  const int nA = m * (m + 1) / 2, nbw = (nA + 63) >> 6;
  const int widx = (wave & 3) == 3 ? -1 : wave - (wave >> 2);  // index among the waves of SIMDs 0-2 (12 of them)
  const int bidx = (widx >= 0 && widx < nbw) ? widx * 64 + lane : nA;
  const bool is_blk = bidx < nA;
  int bI = 0, bJ = 0, b_rd = 0, w00 = 0, w01 = 0, w10 = 0, w11 = 0;
  if (is_blk) {  // unrank the upper triangle row-major
    int base = 0;
    while (base + (m - bI) <= bidx) { base += m - bI; ++bI; }
    bJ = bI + (bidx - base);
    b_rd = 2 * bI * ld + 2 * bJ;
    const int R0 = rr_dst(2 * bI, m), R1 = rr_dst(2 * bI + 1, m), C0 = rr_dst(2 * bJ, m), C1 = rr_dst(2 * bJ + 1, m);
    w00 = min(R0, C0) * ld + max(R0, C0); w01 = min(R0, C1) * ld + max(R0, C1);
    w10 = min(R1, C0) * ld + max(R1, C0); w11 = min(R1, C1) * ld + max(R1, C1);
  }
  const bool is_rot = wave == 3 && lane < m;
  int rp_dp = 0, rp_dq = 0, rp_ob = 0, rp_cp = 0, rp_cq = 0, rp_cl = 0, rp_ch = 0, rp_k = 0;
  if (wave == 3) {
    __builtin_amdgcn_s_setprio(3);
    rp_k = is_rot ? lane : 0;
    const int p = rr_src(2 * rp_k, m), q = rr_src(2 * rp_k + 1, m);
    const int ip = p >> 1, ap = p & 1, iq = q >> 1, aq = q & 1, lo = min(ip, iq), hi = max(ip, iq);
    const int ra = ip < iq ? ap : aq, ca = ip < iq ? aq : ap;  // (row in pair lo, column in pair hi) of the new off-diagonal entry
    rp_dp = 2 * ip * ld + 2 * ip; rp_dq = 2 * iq * ld + 2 * iq; rp_ob = 2 * lo * ld + 2 * hi;
    rp_cp = 4 * ip + 2 * ap; rp_cq = 4 * iq + 2 * aq; rp_cl = 4 * lo + 2 * ra; rp_ch = 4 * hi + 2 * ca;
  }
  for (int e = tid; e < r * r; e += nt) {  // i = coordinate, j = position
    const int i = e / r, j = e - i * r;
    LDS_VT(j * ldk + i) = Vwarm ? Vwarm[e] : (i == j ? 1.0 : 0.0);
  }
  EIG_STAMP(50);
  if (spec.ready || spec.cancel) {  // (uniform) a speculative launch: cancelled already?  Enqueued ahead of its input (`ready`):
    // wait for the launch that announces it, or for the cancellation.  Should that launch not come forward within 5 ms — kernels
    // of different streams forced to run one at a time by a tool, say — give up and say so in the pinned status: the host then
    // repeats the decomposition the ordinary way.
    if (is_poll) {
      if (polled == spec.seq) s_cancel = 1;  // the word first: an input that is there does not hide it
      else if (spec.ready) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();  // 100 MHz
        for (;;) {
          if (__hip_atomic_load(spec.ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - spec.ready_seq >= 0) break;
          if (__hip_atomic_load(spec.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == spec.seq) { s_cancel = 1; break; }
          if (__builtin_amdgcn_s_memrealtime() - t0 > kEigenWaitTicks) { s_cancel = 2; break; }
          __builtin_amdgcn_s_sleep(32);
        }
        if (spec.wait_ticks) atomicAdd((unsigned long long*)spec.wait_ticks, (unsigned long long)(__builtin_amdgcn_s_memrealtime() - t0));
      }
    }
    __syncthreads();
    if (spec.ready) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // (acquire side for the plain loads of the partials below)
    if (s_cancel) {  // cancelled (or timed out) before it started: nothing is assembled, nothing is written
      if (tid == 0) {
        progress_publish(meta, launch_id, 0, kPwAbort);
        if (s_cancel == 2) {  // timed out: tell the host, and mark the basis that was never written so that no later
          // decomposition takes it for a warm start (a NaN in its first entry; a finished decomposition overwrites it)
          if (host_status) __hip_atomic_store(host_status, kEigenGaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          Vout[0] = __builtin_nan("");
        }
      }
      return;
    }
  }
  EIG_STAMP(51);
  if (spec.splits > 0) {
    // M = I + Σ_s partial_s from the split-K partials of the regression launch (lower triangle of (r+1)² matrices, summed in
    // split order from 0.0 like the factorisation does).  One 16-byte piece (row i, columns 2jp, 2jp+1) per thread and row
    // half, every split's load in flight at once: the partials sit in other CUs' L2 slices, and this CU's share of them
    // (13 × 21 KB at rank 51) is what the step costs — dependent loads took 8-10 µs here, this takes ≈ 2.
    for (int e = tid; e < n2 * n2; e += nt) {
      const int i = e / n2, j = e - i * n2;
      LDS_A(0, i * ld + j) = (i == j && i >= r) ? 1e300 : 0.0;
    }
    __syncthreads();
    const size_t nn = (size_t)(r + 1) * (r + 1);
    const int jp = tid & 31, j0 = 2 * jp;
    dbl2 acc[2] = {dbl2{0.0, 0.0}, dbl2{0.0, 0.0}};
    bool live[2];
    size_t off[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = (tid >> 5) + 32 * h;
      live[h] = i < r && j0 <= i;
      off[h] = live[h] ? (size_t)i * (r + 1) + j0 : 0;  // (r + 1 even or odd: the piece is read as two 8-byte halves when unaligned)
    }
    const bool aligned = ((r + 1) & 1) == 0;
    int sp = 0;
    for (; sp + 8 <= spec.splits; sp += 8) {
      dbl2 p[8][2];
#pragma unroll
      for (int q8 = 0; q8 < 8; ++q8)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double* src = M + (size_t)(sp + q8) * nn + off[h];
          p[q8][h] = aligned ? *(const dbl2*)src : dbl2{src[0], src[1]};
        }
#pragma unroll
      for (int q8 = 0; q8 < 8; ++q8)
#pragma unroll
        for (int h = 0; h < 2; ++h) acc[h] += p[q8][h];
    }
    for (; sp < spec.splits; ++sp) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const double* src = M + (size_t)sp * nn + off[h];
        acc[h] += aligned ? *(const dbl2*)src : dbl2{src[0], src[1]};
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (live[h]) {
        const int i = (tid >> 5) + 32 * h;
        const double si = sqrt_lambda[i];
        double v0 = acc[h].x + (i == j0 ? 1.0 : 0.0);
        v0 = v0 / (si * sqrt_lambda[j0]);
        LDS_A(0, i * ld + j0) = v0; LDS_A(0, j0 * ld + i) = v0;
        if (j0 + 1 <= i) {
          double v1 = acc[h].y + (i == j0 + 1 ? 1.0 : 0.0);
          v1 = v1 / (si * sqrt_lambda[j0 + 1]);
          LDS_A(0, i * ld + j0 + 1) = v1; LDS_A(0, (j0 + 1) * ld + i) = v1;
        }
      }
  } else {
    for (int e = tid; e < n2 * n2; e += nt) {
      const int i = e / n2, j = e - i * n2;
      double v = i == j ? 1e300 : 0.0;
      if (i < r && j < r) v = 0.5 * (M[(size_t)i * r + j] + M[(size_t)j * r + i]) / (sqrt_lambda[i] * sqrt_lambda[j]);
      LDS_A(0, i * ld + j) = v;
    }
  }
  __syncthreads();
  EIG_STAMP(1);
  if (Vwarm) {  // A <- Vᵀ A V (nearly diagonal when V diagonalised a nearby posterior) on the f64 matrix cores: one 16×16
    // output tile per wave, the contraction in steps of 4 (v_mfma_f64_16x16x4_f64: lane l supplies A[l&15][l>>4] and
    // B[l>>4][l&15], result register g is D[(l>>4) + 4g][l&15]).  Both products read their operands along rows of LDS
    // images (row = l&15, k = l>>4: rows are 16 B apart modulo the 256-B bank window, conflict free); indices >= r (the
    // dummy of an odd rank, the padding of the tiles) enter as zeros.
    const int tI = wave >> 2, tJ = wave & 3, nT = (n2 + 15) >> 4, l15 = lane & 15, l4 = lane >> 4;
    {  // Tt[j][i] = Σ_k Vt[j][k]·A[k][i]   (tile rows j, tile columns i)
      const int j = 16 * tI + l15, i = 16 * tJ + l15;
      const bool vj = j < r, vi = i < r;
      const int jc = vj ? j : 0, ic = vi ? i : 0;
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      if (tI < nT && tJ < nT) {
        // eight steps' operands at a time (one trip of LDS latency), then their MFMAs back to back
#pragma unroll
        for (int h = 0; h < 16; h += 8) {
        double av[8], bv[8];
#pragma unroll
        for (int st = 0; st < 8; ++st) {
          const int k = 4 * (h + st) + l4;
          const bool vk = k < r;
          const int kk = vk ? k : 0;
          const double a = LDS_VT(jc * ldk + kk), b = LDS_A(0, kk * ld + ic);
          av[st] = (vj && vk) ? a : 0.0; bv[st] = (vi && vk) ? b : 0.0;
        }
#pragma unroll
        for (int st = 0; st < 8; ++st)
          if (4 * (h + st) < n2) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], bv[st], acc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * tI + l4 + 4 * g;
          if (row < n2 && i < n2) LDS_T(row * ldk + i) = acc[g];
        }
      }
    }
    __syncthreads();
    {  // A[i][j] = Σ_k Vt[i][k]·Tt[j][k], tiles of the upper triangle only
      const int i = 16 * tI + l15, j = 16 * tJ + l15;
      const bool vi = i < r, vj = j < r;
      const int ic = vi ? i : 0, jc = vj ? j : 0;
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      if (tI <= tJ && tJ < nT) {
#pragma unroll
        for (int h = 0; h < 16; h += 8) {
        double av[8], bv[8];
#pragma unroll
        for (int st = 0; st < 8; ++st) {
          const int k = 4 * (h + st) + l4;
          const bool vk = k < r;
          const int kk = vk ? k : 0;
          const double a = LDS_VT(ic * ldk + kk), b = LDS_T(jc * ldk + kk);
          av[st] = (vi && vk) ? a : 0.0; bv[st] = (vj && vk) ? b : 0.0;
        }
#pragma unroll
        for (int st = 0; st < 8; ++st)
          if (4 * (h + st) < n2) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], bv[st], acc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * tI + l4 + 4 * g;
          if (row <= j && j < r) LDS_A(0, row * ld + j) = acc[g];
        }
      }
    }
    __syncthreads();
  }
  EIG_STAMP(2);

  if (wave == 3) {
    // rotations of the first round, straight from the diagonal blocks
    const int o = 2 * rp_k * ld + 2 * rp_k;
    const Rot R = jacobi_rotation(LDS_A(0, o), LDS_A(0, o + 1), LDS_A(0, o + ld + 1));
    if (is_rot) { LDS_C(0, 4 * rp_k) = R.c; LDS_C(0, 4 * rp_k + 1) = -R.s; LDS_C(0, 4 * rp_k + 2) = R.s; LDS_C(0, 4 * rp_k + 3) = R.c; }
  }
  const bool is_log = wave == kRrLogWave && lane < m;
  const size_t lstride = (size_t)2 * m;  // doubles per logged round: (c, −s) of every pair
  __syncthreads();
  EIG_STAMP(3);

  // One round: reads buffers `cur`, writes buffers `cur ^ 1`.  `cur` is a template constant (the loop below alternates
  // the two instantiations), so no address is computed inside the loop at all.
  int n_rounds = 0, pub_floor = 0;
  auto round = [&](auto CUR) {
    constexpr int cur = decltype(CUR)::value;
    constexpr int ac = oA + cur * szA, an = oA + (cur ^ 1) * szA, cc = oC + cur * szC, cn = oC + (cur ^ 1) * szC;
    if (is_blk) {
      const dbl2 r0 = lds2(&s_dyn[ac + b_rd]), r1 = lds2(&s_dyn[ac + b_rd + ld]);
      const dbl2 c1 = lds2(&s_dyn[cc + 4 * bI]), c2 = lds2(&s_dyn[cc + 4 * bJ]);  // (c, −s)
      const bool dg = bI == bJ;  // diagonal block: its lower entry is not stored
      const B22 n = rot_block(B22{r0.x, r0.y, dg ? r0.y : r1.x, r1.y}, c1.x, -c1.y, c2.x, -c2.y);
      // (diagonal block: w01 and w10 are the same address and a01, a10 agree to rounding — either store serves)
      s_dyn[an + w00] = n.a00; s_dyn[an + w01] = n.a01; s_dyn[an + w10] = n.a10; s_dyn[an + w11] = n.a11;
    } else if (wave == 3) {
      // the next round pairs the contents of old positions p (pair ip, side ap) and q (pair iq, side aq); their three
      // entries after this round's rotations, by the block threads' own expressions
      const dbl2 dp0 = lds2(&s_dyn[ac + rp_dp]), dp1 = lds2(&s_dyn[ac + rp_dp + ld]);
      const dbl2 dq0 = lds2(&s_dyn[ac + rp_dq]), dq1 = lds2(&s_dyn[ac + rp_dq + ld]);
      const dbl2 b0 = lds2(&s_dyn[ac + rp_ob]), b1 = lds2(&s_dyn[ac + rp_ob + ld]);
      const dbl2 kp = lds2(&s_dyn[cc + rp_cp]), kq = lds2(&s_dyn[cc + rp_cq]);  // rotation column (p, q) of each factor
      const dbl2 kl = lds2(&s_dyn[cc + rp_cl]), kh = lds2(&s_dyn[cc + rp_ch]);
      __builtin_amdgcn_sched_barrier(0);  // all ten reads in flight together: ONE trip of LDS latency on the chain
      // entry = Σ (rotation entry products)·(block entries), as two independent multiply-add pairs and one add; it
      // only steers the next angle, so it need not match the block threads' rounding
      const double app = fma(kp.x * kp.x, dp0.x, (kp.x * kp.y) * dp0.y) + fma(kp.y * kp.x, dp0.y, (kp.y * kp.y) * dp1.y);
      const double aqq = fma(kq.x * kq.x, dq0.x, (kq.x * kq.y) * dq0.y) + fma(kq.y * kq.x, dq0.y, (kq.y * kq.y) * dq1.y);
      const double apq = fma(kh.x * kl.x, b0.x, (kh.x * kl.y) * b1.x) + fma(kh.y * kl.x, b0.y, (kh.y * kl.y) * b1.y);
      const Rot R = jacobi_rotation(app, apq, aqq);
      if (is_rot) {
        *(dbl2*)&s_dyn[cn + 4 * rp_k] = dbl2{R.c, -R.s};
        *(dbl2*)&s_dyn[cn + 4 * rp_k + 2] = dbl2{R.s, R.c};
      }
    } else if (wave == kRrLogWave) {  // the rotations this round applies, for the replay workgroups (negligible ones as
      // identities): two write-through stores per pair; every fourth round the progress word is advanced to kRrLogLag rounds
      // behind — 2 + ¼ memory operations per round in this wave's queue, so all but the youngest 2·lag + lag/4 − 1 of them
      // being done means the rounds up to n_rounds − lag have arrived
      if (is_log) {
        const dbl2 k = lds2(&s_dyn[cc + 4 * lane]);
        const dbl2 w = fabs(k.y) >= 2e-17 ? k : dbl2{1.0, 0.0};
        double* dst = rotlog + (size_t)n_rounds * lstride + 2 * lane;
        sc1_store(dst, w.x); sc1_store(dst + 1, w.y);
      }
      if ((n_rounds & 3) == 3) {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * kRrLogLag + kRrLogLag / 4 - 1) : "memory");
        const int upto = n_rounds + 1 - kRrLogLag;
        if (lane == 0 && upto > pub_floor) __hip_atomic_store(meta, (launch_id << kPwIdShift) | upto, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
    ++n_rounds;
  };
  int converged = 0, n_sweeps = 0, in_sweep = 0, use_corr = 0;
  // (a warm-started iteration has never met either test after one sweep, a cold one never before its third: those passes
  // — two barriers and a reduction each — are skipped; were the matrix diagonal already, one more sweep would be harmless)
  const int first_test = Vwarm ? 1 : 2;
  auto sweep_end = [&](int cur) -> bool {  // -> stop?
    EIG_STAMP(4 + 2 * n_sweeps);
    in_sweep = 0;
    if (n_sweeps < first_test && n_sweeps + 1 < max_sweeps) {
      ++n_sweeps;
      EIG_STAMP(3 + 2 * n_sweeps);
      return false;
    }
    // this sweep's rotations are in the log (written through; the log wave's own progress stores have landed, too): the
    // replay workgroups may have all of them (published behind the barrier below)
    if (wave == kRrLogWave) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pub_floor = n_rounds;
    // Two ways to be done, both from one pass over the stored upper triangle (thread = row, 4 columns; one barrier):
    //   strict  off(A)² <= 1e-26·Σ diag²: nothing left to do;
    //   loose   every |A_ij| <= kLooseTau·|A_jj − A_ii| (5e-7): what one more sweep would do to the eigenvectors is, to first
    //           order, V <- V·(I + X) with X_ij = A_ij/(A_jj − A_ii) (antisymmetric), all |X_ij| <= 5e-7 — the replay workgroups
    //           apply that instead (error of the correction ~ X²: 2.5e-13, against 19 µs for the sweep; at 4e-6, the value until
    //           the rank ladder of tests/test_gpu_small_ranks.py, V·S·Vᵀ missed D·M⁻¹·D by up to 5.9e-12).  The Jacobi sweeps
    //           converge quadratically, so the sweep before the last is the one that meets this test.
    double off = 0.0, dg = 0.0;
    bool bad = false;
    {
      const int i = tid >> 4, j0 = (tid & 15) << 2;
      if (i < n2 && j0 + 3 >= i && j0 < n2) {
        const dbl2 u = lds2(&LDS_A(cur, i * ld + j0)), w = lds2(&LDS_A(cur, i * ld + j0 + 2));
        const double dii = LDS_A(cur, i * ld + i);
        const double v[4] = {u.x, u.y, w.x, w.y};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = j0 + c;
          if (j < n2) {
            if (j == i) { if (v[c] < 1e299) dg = fma(v[c], v[c], dg); }
            else if (j > i) {
              off = fma(2.0 * v[c], v[c], off);
              bad = bad || fabs(v[c]) > kLooseTau * fabs(LDS_A(cur, j * ld + j) - dii);
            }
          }
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) { off += __shfl_xor(off, o, 64); dg += __shfl_xor(dg, o, 64); }
    const bool wave_bad = __any(bad);
    if (lane == 0) { s_red[wave] = off; s_red2[wave] = dg; s_bad[wave] = wave_bad ? 1 : 0; }
    __syncthreads();
    if (tid == 0) progress_publish(meta, launch_id, n_rounds, 0);
    off = 0.0; dg = 0.0;
    int any_bad = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { off += s_red[w]; dg += s_red2[w]; any_bad |= s_bad[w]; }
    const int strict = off <= 1e-26 * dg;
    const int loose = !any_bad && off <= dg;  // (off <= dg: false for NaN)
    converged = strict || (loose && !no_corr);
    use_corr = converged && !strict;
    if (tid == 0 && n_sweeps < 8) ((double*)(meta + 80))[n_sweeps] = off / dg;  // diagnostic: off(A)²/Σdiag² after each sweep
    ++n_sweeps;
    EIG_STAMP(3 + 2 * n_sweeps);
    return converged || n_sweeps >= max_sweeps;
  };
  // The cancel word of a speculative decomposition, on a fixed schedule of the round counter (whatever the sweeps' length: a
  // decomposition whose result nobody wants holds the eigen stream, and the next one waits behind it):
  //   rounds ≡ 0 (mod 8)  the poll wave issues its read of the pinned word — never waited for on the spot, that would hold
  //                       every wave at the round's barrier for a microsecond or two;
  //   rounds ≡ 4          … and its last lane stores the outcome to s_cancel, ahead of that round's barrier;
  //   rounds ≡ 6          every wave reads s_cancel behind the round's barrier and leaves the loop.
  // Store and read are two barriers apart, and the next store is five rounds behind the read: every wave reads the same value
  // in the same round (a wave that left a loop of barriers alone would hang the others).  Nothing else in the loop reads s_cancel.
  const bool cancellable = spec.cancel != nullptr;                                           // (uniform)
  const bool poll_wave = cancellable && __builtin_amdgcn_readfirstlane(wave) == kRrPollWave;  // (a scalar: real branches below)
  bool cancelled = false;
  int cur = 0, word = 0;
  if (max_sweeps > 0)
    for (;;) {  // (two rounds per pass: n_rounds is even here)
      const int phase = n_rounds & 7;
      if (poll_wave) {
        if (phase == 0) word = __hip_atomic_load(spec.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (phase == 4) {
          // (the wait for the word stays inside this branch — hoisted out of it, every wave would wait for its own memory
          // operations here, the log wave for the stores it keeps in flight)
          asm volatile("" : "+v"(word));
          if (lane == 63 && word == spec.seq) s_cancel = 1;
        }
      }
      round(IntC<0>{}); cur = 1;
      if (cancellable && phase == 6) cancelled = __builtin_amdgcn_readfirstlane(s_cancel) != 0;  // (one value: a uniform branch)
      if (cancelled || (++in_sweep == n2 - 1 && sweep_end(cur))) break;
      round(IntC<1>{}); cur = 0;
      if (++in_sweep == n2 - 1 && sweep_end(cur)) break;
    }
  if (cancelled) {  // given up: no status, no eigenvalues; the replay workgroups drop what they have.  The log wave's stores —
    // those of the progress word among them — have landed before the barrier behind which the abort word is published: a late
    // one on top of it would leave the replay workgroups waiting for rounds that never come
    if (wave == kRrLogWave) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) progress_publish(meta, launch_id, n_rounds, kPwAbort);
    return;
  }
  if (tid == 0) {
    ++meta[100 + min(n_sweeps, 15)];  // diagnostic: histogram of sweep counts on this work buffer
    status[0] = converged ? 0 : 2; status[-1] = n_sweeps;
    if (host_status) __hip_atomic_store(host_status, converged ? 0 : 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  EIG_STAMP(62);
  // ---- hand-over to the replay workgroup: the final diagonal by position (it ranks the eigenvalues: those of D M⁻¹ D are
  // 1/μ, S descending = μ ascending, the dummy sorts last and is dropped) and, when the iteration stopped on the loose
  // test, the first-order correction X
  double* xg = vpos;
  if (tid < n2) sc1_store((double*)meta + kEigMetaMu + tid, LDS_A(cur, tid * ld + tid));
  if (use_corr) {
    const int i = tid >> 4, j0 = (tid & 15) << 2;
    if (i < n2 && j0 + 3 >= i && j0 < n2) {
      const double dii = LDS_A(cur, i * ld + i);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + c;
        if (j < n2 && j >= i) {
          const double a = LDS_A(cur, i * ld + j);
          const double x = (j == i || a == 0.0) ? 0.0 : a / (LDS_A(cur, j * ld + j) - dii);
          sc1_store(xg + i * n2 + j, x);
          if (j != i) sc1_store(xg + j * n2 + i, -x);
        }
      }
    }
  }
  if (tid == 0) __hip_atomic_store(meta + kEigMetaCorr, use_corr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's stores, before the barrier behind which they are released
  __syncthreads();
  if (tid == 0) progress_publish(meta, launch_id, n_rounds, kPwFinished);  // (max_sweeps == 0: nothing to replay)
  EIG_STAMP(63);
#undef LDS_A
#undef LDS_VT
#undef LDS_T
#undef LDS_C
}

// ---------------------------------------------------------------- posterior KL basis, ranks 65..200: in-place parallel Jacobi
// One CU's LDS cannot hold these matrices twice (the fixed-position kernel above reads one copy and writes the permuted
// other), but it holds the strict upper triangle ONCE, packed, beside the diagonal (rank 200: 159 KB + 1.6 KB): the classical
// parallel-order Jacobi iteration updates it in place — pair P of a round rotates (p, q) of the round-robin tournament, block
// (P1, P2) owns the four entries A[{p1,q1}][{p2,q2}] and nobody else touches them in that round.
//   workgroup 0      phase 1: one thread per pair computes (c, s) from three entries and logs it; barrier;
//                    phase 2: every thread transforms its (up to five) 2×2 blocks, R1ᵀ·B·R2, in place; barrier.
//                    ≈ 2.3 µs per round at rank 200 (LDS cycles: 5,050 blocks × 8 accesses), 199 rounds per sweep.
//   workgroups 1..   64 coordinates (rows of V) each, the slab in LDS: they follow the published sweeps and apply every
//                    round's rotations to their rows (the tournament's pairs are recomputed, only (c, s) is read from the log).
// Warm start: the launcher transforms N by the basis of a nearby posterior first (k_eigen_big_warm, two plain GEMM passes on
// many CUs), the slabs start from that basis.  Sort, signs and the two output layouts are taken by k_eigen_big_finish (one
// wave per eigenvector) behind this launch.  Ranks above 200 take the generic kernel further up.
constexpr int kBigBlocksPerThread = 5;   // 1024 threads × 5 >= 100·101/2 blocks (rank 200)
constexpr int kBigMaxRank = 200;
constexpr int kBigSlabRows = 64;
constexpr int kBigStageRounds = 16;      // rounds of (c, s) staged per pass by a replay workgroup

__device__ __forceinline__ int big_idx(int i, int j, int n) {  // packed strict upper triangle, i < j
  return i * (2 * n - i - 1) / 2 + (j - i - 1);
}
// round-robin tournament (circle method) on n2 players: slot 0 holds (mm, 0) in round 0 and keeps its first player; every
// other seat advances by one per round.  State (ra, rb) of a slot; the pair is (min, max)
__device__ __forceinline__ void rr_init(int slot, int mm, int& ra, int& rb) {
  if (slot == 0) { ra = mm; rb = 0; }
  else { ra = slot % mm; rb = (mm - slot) % mm; }
}
__device__ __forceinline__ void rr_advance(int slot, int mm, int& ra, int& rb) {
  if (slot == 0) { rb = rb + 1 == mm ? 0 : rb + 1; }
  else { ra = ra + 1 == mm ? 0 : ra + 1; rb = rb + 1 == mm ? 0 : rb + 1; }
}

// SQUARE: the upper triangle inside a full n × ld image (ranks <= 140: it fits, and an entry's address is i·ld + j); otherwise the
// packed triangle, row bases carried along with the tournament's players
template <bool SQUARE>
__global__ void __launch_bounds__(1024) k_eigen_big(int r, const double* __restrict__ A0 /* r×r, symmetric */, const double* __restrict__ Vwarm,
                                                     double* __restrict__ Vwork /* [coordinate][index] eigenvectors, unsorted */,
                                                     double* __restrict__ mu_out, double* rotlog, double* xcorr /* r×r */, int* meta,
                                                     int max_sweeps, int no_corr, int launch_id, int* __restrict__ status,
                                                     const int* __restrict__ gate /* optional: run only if *gate == 2 */) {
  if (gate && gate[0] != 2) return;  // (the fall-back of the tridiagonal route: its eigenvalues were told apart)
  const int tid = threadIdx.x, nt = blockDim.x;
  const int n = r, n2 = (r + 1) & ~1, half = n2 >> 1, mm = n2 - 1;
  __shared__ short s_p[128], s_q[128];
  __shared__ double s_red[16], s_red2[16];
  __shared__ int s_pw, s_bad[16];
  if (blockIdx.x != 0) {
    // ---------------- replay: rows [row0, row0 + rows) of V in LDS, rotated as the sweeps are published
    const int row0 = ((int)blockIdx.x - 1) * kBigSlabRows, rows = min(kBigSlabRows, r - row0);
    double* s_cs = s_dyn + kBigSlabRows * n;  // kBigStageRounds × half × (c, s); later: 16 columns of the correction
    for (int e = tid; e < rows * n; e += nt) {
      const int k = e / n, p = e - k * n;
      s_dyn[e] = Vwarm ? Vwarm[(size_t)(row0 + k) * r + p] : (row0 + k == p ? 1.0 : 0.0);
    }
    int ra = 0, rb = 0;
    if (tid < half) rr_init(tid, mm, ra, rb);
    // items of a round: (row k, pair P); the same ones every round
    constexpr int kItems = 7;  // 64 rows × 100 pairs / 1024 threads
    int itk[kItems], itP[kItems];
#pragma unroll
    for (int m = 0; m < kItems; ++m) {
      const int it = tid + m * nt;
      itk[m] = it < rows * half ? it / half : -1;
      itP[m] = it < rows * half ? it - itk[m] * half : 0;
    }
    int done = 0;
    for (;;) {
      if (tid == 0) {
        int pw;
        for (;;) {
          pw = __hip_atomic_load(meta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (((pw >> kPwIdShift) & kPwIdMask) == launch_id && ((pw & kPwRoundsMask) > done || (pw & (kPwAbort | kPwFinished)))) break;
          __builtin_amdgcn_s_sleep(8);
        }
        s_pw = pw;
      }
      __syncthreads();
      const int pw = s_pw;
      const int avail = pw & kPwRoundsMask;
      while (done < avail) {
        const int nr = min(avail - done, kBigStageRounds);
        for (int e = tid; e < 2 * nr * half; e += nt) s_cs[e] = sc1_load(rotlog + 2 * (size_t)done * half + e);
        __syncthreads();
        for (int rl = 0; rl < nr; ++rl) {
          if (tid < half) {
            const int p = ra < rb ? ra : rb, q = ra < rb ? rb : ra;
            s_p[tid] = (short)p; s_q[tid] = (short)q;
            rr_advance(tid, mm, ra, rb);
          }
          __syncthreads();
#pragma unroll
          for (int m = 0; m < kItems; ++m) {
            if (itk[m] < 0) continue;
            const int k = itk[m], P = itP[m];
            const int p = s_p[P], q = s_q[P];
            if (q < r) {
              const dbl2 cs = *(const dbl2*)&s_cs[2 * (rl * half + P)];
              const double vp = s_dyn[k * n + p], vq = s_dyn[k * n + q];
              s_dyn[k * n + p] = fma(cs.x, vp, -(cs.y * vq));   // columns: [p q] <- [p q]·[c s; −s c]
              s_dyn[k * n + q] = fma(cs.y, vp, cs.x * vq);
            }
          }
          __syncthreads();
        }
        done += nr;
      }
      if (pw & (kPwFinished | kPwAbort)) break;
    }
    if (__hip_atomic_load(meta + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == launch_id) {
      // the iteration stopped on the loose test: rows·(I + X), sixteen columns of X through LDS at a time (k_posterior_eigen_rr)
      for (int j0 = 0; j0 < n; j0 += 16) {
        __syncthreads();
        for (int e = tid; e < n * 16; e += nt) {
          const int i = e >> 4, j = j0 + (e & 15);
          s_cs[e] = j < n ? sc1_load(xcorr + (size_t)i * n + j) : 0.0;
        }
        __syncthreads();
        const int k = tid >> 4, j = j0 + (tid & 15);
        if (k < rows && j < n) {
          double acc = 0.0;
          for (int i = 0; i < n; ++i) acc = fma(s_dyn[k * n + i], s_cs[i * 16 + (tid & 15)], acc);
          Vwork[(size_t)(row0 + k) * r + j] = s_dyn[k * n + j] + acc;
        }
      }
    } else {
      for (int e = tid; e < rows * n; e += nt) Vwork[(size_t)row0 * r + e] = s_dyn[e];
    }
    return;
  }
  // ---------------- the iteration
  const int ld = SQUARE ? (n | 1) : 0;
  const int n_off = SQUARE ? n * ld : n * (n - 1) / 2;
  double* s_diag = s_dyn + n_off;
  double* s_cs = s_diag + n;  // [half] (c, s) of the round's pairs
  auto at = [&](int i, int j) { return SQUARE ? i * ld + j : big_idx(i, j, n); };  // i < j
  for (int e = tid; e < n * n; e += nt) {
    const int i = e / n, j = e - i * n;
    if (i < j) s_dyn[at(i, j)] = 0.5 * (A0[e] + A0[(size_t)j * n + i]);
    else if (i == j) s_diag[i] = A0[e];
  }
  const int n_blocks = half * (half + 1) / 2;
  // this thread's blocks (P1 <= P2) and the players sitting at their four seats, advanced round by round in registers
  int bP1[kBigBlocksPerThread], bP2[kBigBlocksPerThread], a1[kBigBlocksPerThread], b1[kBigBlocksPerThread], a2[kBigBlocksPerThread],
      b2[kBigBlocksPerThread];
#pragma unroll
  for (int m = 0; m < kBigBlocksPerThread; ++m) {
    const int w = tid + nt * m;
    bP1[m] = -1; bP2[m] = 0; a1[m] = b1[m] = a2[m] = b2[m] = 0;
    if (w < n_blocks) {  // unrank the upper triangle of the pair × pair grid, row-major
      int P1 = 0, base = 0;
      while (base + (half - P1) <= w) { base += half - P1; ++P1; }
      bP1[m] = P1; bP2[m] = P1 + (w - base);
      rr_init(bP1[m], mm, a1[m], b1[m]);
      rr_init(bP2[m], mm, a2[m], b2[m]);
    }
  }
  int ra = 0, rb = 0;
  if (tid < half) rr_init(tid, mm, ra, rb);
  __syncthreads();
  int converged = 0, use_corr = 0, n_sweeps = 0, n_rounds = 0;
  for (int sweep = 0; sweep < max_sweeps && !converged; ++sweep) {
    for (int rnd = 0; rnd < mm; ++rnd) {
      if (tid < half) {
        const int p = ra < rb ? ra : rb, q = ra < rb ? rb : ra;
        Rot R{1.0, 0.0};
        if (q < r) R = jacobi_rotation(s_diag[p], s_dyn[at(p, q)], s_diag[q]);
        *(dbl2*)&s_cs[2 * tid] = dbl2{R.c, R.s};
        *(dbl2*)(rotlog + 2 * ((size_t)n_rounds * half + tid)) = dbl2{R.c, R.s};
        rr_advance(tid, mm, ra, rb);
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < kBigBlocksPerThread; ++m) {
        if (bP1[m] < 0) continue;
        const int P1 = bP1[m], P2 = bP2[m];
        const int p1 = min(a1[m], b1[m]), q1 = max(a1[m], b1[m]), p2 = min(a2[m], b2[m]), q2 = max(a2[m], b2[m]);
        rr_advance(P1, mm, a1[m], b1[m]);
        rr_advance(P2, mm, a2[m], b2[m]);
        const dbl2 r1 = *(const dbl2*)&s_cs[2 * P1], r2 = *(const dbl2*)&s_cs[2 * P2];
        if (P1 == P2) {
          if (q1 < r) {
            const int o = at(p1, q1);
            const double apq = s_dyn[o];
            const B22 nb = rot_block(B22{s_diag[p1], apq, apq, s_diag[q1]}, r1.x, r1.y, r1.x, r1.y);
            s_diag[p1] = nb.a00; s_diag[q1] = nb.a11; s_dyn[o] = nb.a01;
          }
        } else {
          // entries A[x][y], x in {p1, q1}, y in {p2, q2}; a bye (q >= r) has no row / column and an identity rotation
          // (taken block by block: holding all five blocks' entries at once — one trip of LDS latency for the lot — needs
          // more than the 128 registers a 1024-thread workgroup has, and the spills cost more than the latency: 648 -> 899 µs at rank 101)
          const bool h1 = q1 < r, h2 = q2 < r;
          const int opp = p1 < p2 ? at(p1, p2) : at(p2, p1);
          const int opq = h2 ? (p1 < q2 ? at(p1, q2) : at(q2, p1)) : 0;
          const int oqp = h1 ? (q1 < p2 ? at(q1, p2) : at(p2, q1)) : 0;
          const int oqq = (h1 && h2) ? (q1 < q2 ? at(q1, q2) : at(q2, q1)) : 0;
          B22 b{s_dyn[opp], h2 ? s_dyn[opq] : 0.0, h1 ? s_dyn[oqp] : 0.0, (h1 && h2) ? s_dyn[oqq] : 0.0};
          const B22 nb = rot_block(b, r1.x, r1.y, r2.x, r2.y);
          s_dyn[opp] = nb.a00;
          if (h2) s_dyn[opq] = nb.a01;
          if (h1) s_dyn[oqp] = nb.a10;
          if (h1 && h2) s_dyn[oqq] = nb.a11;
        }
      }
      __syncthreads();
      ++n_rounds;
    }
    // convergence (thread = row of the triangle): strict off(A)² <= 1e-26·Σ diag², or loose — every |A_ij| <= 4e-6·|A_jj − A_ii|:
    // the replay workgroups then apply V <- V·(I + X), X_ij = A_ij/(A_jj − A_ii), in place of one more sweep (see k_posterior_eigen_rr)
    double off = 0.0, dg = 0.0;
    bool bad = false;
    if (tid < n) {
      const double dii = s_diag[tid];
      for (int j = tid + 1; j < n; ++j) {
        const double v = s_dyn[at(tid, j)];
        off = fma(2.0 * v, v, off);
        bad = bad || fabs(v) > 4e-6 * fabs(s_diag[j] - dii);
      }
      dg = dii * dii;
    }
    for (int o = 32; o > 0; o >>= 1) { off += __shfl_xor(off, o, 64); dg += __shfl_xor(dg, o, 64); }
    const bool wave_bad = __any(bad);
    if ((tid & 63) == 0) { s_red[tid >> 6] = off; s_red2[tid >> 6] = dg; s_bad[tid >> 6] = wave_bad ? 1 : 0; }
    __syncthreads();
    off = 0.0; dg = 0.0;
    int any_bad = 0;
    for (int w = 0; w < 16; ++w) { off += s_red[w]; dg += s_red2[w]; any_bad |= s_bad[w]; }
    const int strict = off <= 1e-26 * dg;
    converged = strict || (!any_bad && off <= dg && !no_corr);
    use_corr = converged && !strict;
    n_sweeps = sweep + 1;
    const bool last = converged || sweep + 1 >= max_sweeps;
    if (last && use_corr && tid < n) {
      const double dii = s_diag[tid];
      sc1_store(xcorr + (size_t)tid * n + tid, 0.0);
      for (int j = tid + 1; j < n; ++j) {
        const double a = s_dyn[at(tid, j)];
        const double x = a == 0.0 ? 0.0 : a / (s_diag[j] - dii);
        sc1_store(xcorr + (size_t)tid * n + j, x);
        sc1_store(xcorr + (size_t)j * n + tid, -x);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // this sweep's rotations are in the log (plain stores, every storing wave past the barrier above): released, then announced
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (last) __hip_atomic_store(meta + 1, use_corr ? launch_id : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(meta, (launch_id << kPwIdShift) | (last ? kPwFinished : 0) | n_rounds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
  }
  if (tid < n) mu_out[tid] = s_diag[tid];
  if (tid == 0) { status[0] = converged ? 0 : 2; status[-1] = n_sweeps; }
}

// T = A·V (pass 0) or A' = Vᵀ·T (pass 1): plain one-thread-per-entry products (r <= 200: 8 MFLOP, spread over the chip)
__global__ void __launch_bounds__(256) k_eigen_big_warm(int r, const double* __restrict__ X, const double* __restrict__ V, double* __restrict__ out,
                                                         int pass) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= r * r) return;
  const int i = e / r, j = e - i * r;
  double s = 0.0;
  if (pass == 0) { for (int k = 0; k < r; ++k) s = fma(X[(size_t)i * r + k], V[(size_t)k * r + j], s); }
  else { for (int k = 0; k < r; ++k) s = fma(V[(size_t)k * r + i], X[(size_t)k * r + j], s); }
  out[e] = s;
}

// one wave per index p: rank of its eigenvalue (S descending = mu ascending, ties: lower index first), sign by the
// largest-|.| component (the first among equals), the two output layouts
__global__ void __launch_bounds__(64) k_eigen_big_finish(int r, const double* __restrict__ Vwork, const double* __restrict__ mu,
                                                          double* __restrict__ Vout, double* __restrict__ Vtout, double* __restrict__ Sout,
                                                          const int* __restrict__ status, int* __restrict__ host_status,
                                                          const int* __restrict__ gate, int gate_value) {
  if (gate && ((gate[0] >> kPwIdShift) & kPwIdMask) != gate_value) return;  // (gate = the iteration's progress word: did THIS launch's run?)
  const int p = blockIdx.x, l = threadIdx.x;
  const double mp = mu[p];
  int cnt = 0;
  for (int j = l; j < r; j += 64) { const double mj = mu[j]; cnt += (mj < mp) || (mj == mp && j < p); }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  const int rank = cnt;
  double bv = -1.0;
  int bi = 0x7fffffff;
  for (int k = l; k < r; k += 64) {
    const double a = fabs(Vwork[(size_t)k * r + p]);
    if (a > bv) { bv = a; bi = k; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  const double sgn = Vwork[(size_t)bi * r + p] < 0.0 ? -1.0 : 1.0;
  for (int k = l; k < r; k += 64) {
    const double v = Vwork[(size_t)k * r + p] * sgn;
    Vout[(size_t)k * r + rank] = v;
    Vtout[(size_t)rank * r + k] = v;
  }
  if (l == 0) Sout[rank] = 1.0 / mp;
  if (p == 0 && l == 0 && host_status) __hip_atomic_store(host_status, status[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

static size_t jacobi_work_doubles(int r) {
  const size_t n2 = ((size_t)r + 1) & ~(size_t)1;
  if (r > 64) {  // in-place Jacobi (k_eigen_big): A0 | T | Vwork | mu | rotation log of every sweep | meta — or the generic kernel's r×r scratch
    const size_t log = (size_t)kEigenMaxSweeps * (n2 - 1) * n2;  // (c, s) per pair and round
    return 3 * (size_t)r * r + n2 + log + 64;
  }
  const size_t log = ((size_t)kEigenMaxSweeps * (n2 - 1) + 2) * n2;  // 2 doubles per pair and round
  return log + n2 * 64 + 128 + 256;  // fixed-position variant: log + correction + meta (see launch_eigen_rr)
}
// the tridiagonal route's part of `work`, behind the Jacobi kernels': d | e | beta | mu | sync words | reflectors
// (round 6: 208 — the reference's own largest model, femur_gp_model_200-components.h5, has 201 components: apps/femur/CreateGPModel.scala:93)
constexpr int kTriMaxRank = 256;  // = tri::kTriMaxN: four row slots of 64
static size_t tri_work_doubles(int r) { return r <= kTriMaxRank ? 4 * (size_t)tri::kTriMaxN + 8 + (size_t)r * 256 : 0; }
size_t eigen_work_doubles(int r) { return jacobi_work_doubles(r) + tri_work_doubles(r); }  // `work` of launch_posterior_eigen

// Householder tridiagonalisation on one workgroup, then one wave per eigenpair (icp_tridiag.hpp): ranks 65..256
// (developer switch ICP_EIGEN_TRIDIAG=0: the Jacobi kernels at these ranks, too)
static bool tridiag_route(int r) {
  static const int forced = dev_env("ICP_EIGEN_TRIDIAG") ? std::atoi(dev_env("ICP_EIGEN_TRIDIAG")) : -1;
  return r > 64 && r <= kTriMaxRank && forced != 0;
}
bool eigen_tridiag_many_supported(int r) { return r > 64 && r <= kTriMaxRank; }

// The route's areas of a decomposition's `work`.  Behind the Jacobi kernels' part: d | e | beta | mu | sync words | reflectors.  At its
// head, where the Jacobi kernels' log would be (this route replaces them), the refinement step's matrices N | X | Xt | T | S | R — the
// reflector blocks' T factors live where R will be: R is written behind the solve.
struct TriWork {
  double *d, *e, *beta, *mu;
  int* sync;
  double* Hv;
  double *N, *X, *Xt, *T, *S, *R;
  TriWork(double* work, int r) {
    double* base = work + jacobi_work_doubles(r);
    d = base; e = base + tri::kTriMaxN; beta = base + 2 * tri::kTriMaxN; mu = base + 3 * tri::kTriMaxN;
    sync = (int*)(base + 4 * tri::kTriMaxN);
    Hv = base + 4 * tri::kTriMaxN + 8;
    const size_t rr = (size_t)r * r;
    N = work; X = work + rr; Xt = work + 2 * rr; T = work + 3 * rr; S = work + 4 * rr; R = work + 5 * rr;
  }
};

// rank -> the reduction's shape <waves, row slots, column slots per wave, empty column slots>; rank -> row slots of solve and back
template <int NW_, int SI_, int NT_, int TOFF_> struct TriShape { static constexpr int NW = NW_, SI = SI_, NT = NT_, TOFF = TOFF_; };
template <class F> static void tri_reduction_shape(int r, F&& f) {
  if (r <= 128) f(TriShape<4, 2, 32, 0>{});
  else if (r <= 192) f(TriShape<8, 3, 24, 0>{});
  else if (r <= 200) f(TriShape<8, 4, 25, 7>{});
  else if (r <= 208) f(TriShape<8, 4, 26, 6>{});
  else f(TriShape<8, 4, 32, 0>{});
}
template <class F> static void tri_row_slots(int r, F&& f) {
  if (r <= 128) f(tri::Tag<2>{});
  else if (r <= 192) f(tri::Tag<3>{});
  else f(tri::Tag<4>{});
}

// the completion launch of a sequence: pinned status copies and completion words
template <int CAP>
static void launch_tri_done(hipStream_t st, int n, const EigenRequest* rq, const int* skip) {
  tri::TriDoneBatch<CAP> dm{};
  bool any_done = false;  // (nobody to tell — the on-device loop reads the status words on the device —: no launch)
  for (int q = 0; q < n; ++q) {
    dm.status[q] = rq[q].status; dm.host_status[q] = rq[q].host_status; dm.done_word[q] = rq[q].done_word; dm.done_value[q] = rq[q].done_value;
    any_done = any_done || dm.host_status[q] || dm.done_word[q];
  }
  if (any_done) hipLaunchKernelGGL(tri::k_tri_done<CAP>, dim3(n), dim3(1), 0, st, dm, skip);
}
// The launch sequence for n <= CAP decompositions of rank 65..256 side by side: every launch takes all of them — the one-workgroup
// reductions run on n CUs at once.  parts (optional): M = I + the summed partial first.  skip (optional, device): requests to leave
// alone.  part: 0 = everything, 1 = assembly and reduction only, 2 = what follows.  completion = false leaves the completion launch
// to the caller, who has launches of its own to put before it.
template <int CAP>
static void launch_tri_sequence(hipStream_t st, int r, int n, const EigenRequest* rq, const double* const* parts, const int* skip, int part,
                                bool completion) {
  // (test-hooks build, ICP_TEST_TRI_REFINE_ALWAYS=1: the refinement step whatever the gaps are — it is the rare path otherwise)
  static const bool refine_always = dev_env("ICP_TEST_TRI_REFINE_ALWAYS") && std::atoi(dev_env("ICP_TEST_TRI_REFINE_ALWAYS")) != 0;
  const size_t rr = (size_t)r * r;
  const int nwg = (r + 3) / 4, nt = (r + 15) / 16, nwy = (r - 2 + tri::kWyBlock - 1) / tri::kWyBlock;
  tri::TriBatch<tri::TridiagIO, CAP> tm{};
  tri::TriBatch<tri::TriSolveIO, CAP> sm{};
  tri::TriBatch<tri::TriBackIO, CAP> bm{};
  tri::TriBatch<tri::TriGemm, 2 * CAP> g1{}, g2{}, g3{};
  tri::TriCorrBatch<CAP> cm{};
  tri::AssembleMany am{};
  bool assemble = false;
  for (int q = 0; q < n; ++q) {
    const TriWork w(rq[q].work, r);
    tm.p[q] = tri::TridiagIO{r, rq[q].M, rq[q].sqrt_lambda, w.d, w.e, w.beta, w.Hv, w.N};
    sm.p[q] = tri::TriSolveIO{r, w.d, w.e, w.beta, w.Hv, w.X, w.Xt, rq[q].S, w.mu, w.R, w.sync, rq[q].status};
    bm.p[q] = tri::TriBackIO{r, w.Hv, w.R, w.X, w.Xt, rq[q].status, w.sync};
    // one refinement step: T = N·X and R = I − XᵀX, S = XᵀT, E, then V = X + X·E (and Vt).  sync[3], written by the solve launch:
    // 1 = every gap wide enough, the step's launches return at once (the last one handing X on as V)
    const int* wide = refine_always ? nullptr : w.sync + 3;
    g1.p[2 * q] = tri::TriGemm{w.N, w.X, w.T, 0, nullptr, nullptr, wide};
    g1.p[2 * q + 1] = tri::TriGemm{w.X, w.X, w.R, 1, nullptr, nullptr, wide};
    g2.p[q] = tri::TriGemm{w.X, w.T, w.S, 0, nullptr, nullptr, wide};
    cm.S[q] = w.S; cm.R[q] = w.R; cm.E[q] = w.T; cm.Sout[q] = rq[q].S; cm.skip[q] = wide;
    g3.p[q] = tri::TriGemm{w.Xt, w.T, rq[q].V, 2, w.X, rq[q].Vt, wide};
    am.P[q] = parts ? parts[q] : nullptr;
    am.M[q] = const_cast<double*>(rq[q].M);
    assemble = assemble || am.P[q] != nullptr;
  }
  if (part != 2) {  // the reduction (part 1 of a split sequence: the long one-workgroup launch, before anybody knows whom to skip)
    if (assemble) hipLaunchKernelGGL(tri::k_assemble_many, dim3((unsigned)((rr + 255) / 256), n), dim3(256), 0, st, r, am, skip);
    tri_reduction_shape(r, [&](auto shape) {
      using S = decltype(shape);
      hipLaunchKernelGGL((tri::k_tridiag<CAP, S::NW, S::SI, S::NT, S::TOFF>), dim3(n), dim3(S::NW * 64), 0, st, tm, skip);
    });
  }
  if (part == 1) return;
  tri_row_slots(r, [&](auto si) {
    constexpr int SI = decltype(si)::value;
    if constexpr (SI == 4) {  // (above rank 201 the solve launch's dynamic LDS passes 48 KiB: 61 KiB at rank 256)
      static bool lds_set = false;
      set_dyn_lds_once((const void*)tri::k_tri_solve<CAP, SI>, tri::tri_solve_lds_bytes(tri::kTriMaxN), &lds_set);
    }
    // (the reflector blocks' T factors: the solve launch's trailing workgroups — tri_solve_or_wy)
    hipLaunchKernelGGL((tri::k_tri_solve<CAP, SI>), dim3(nwg + nwy, n), dim3(256), tri::tri_solve_lds_bytes(r), st, sm, skip);
    hipLaunchKernelGGL((tri::k_tri_back<CAP, SI>), dim3(nt, n), dim3(256), 0, st, bm, skip);
  });
  hipLaunchKernelGGL(tri::k_tri_gemm<CAP>, dim3(nt, nt, 2 * n), dim3(64), 0, st, r, g1, skip, 2);
  hipLaunchKernelGGL(tri::k_tri_gemm<CAP>, dim3(nt, nt, n), dim3(64), 0, st, r, g2, skip, 1);
  hipLaunchKernelGGL(tri::k_tri_correction<CAP>, dim3((unsigned)((rr + 255) / 256), n), dim3(256), 0, st, r, cm, skip);
  hipLaunchKernelGGL(tri::k_tri_gemm<CAP>, dim3(nt, nt, n), dim3(64), 0, st, r, g3, skip, 1);
  if (completion) launch_tri_done<CAP>(st, n, rq, skip);
}

// Any number of decompositions (the chains of a wide step), kTriMany to a sequence.  No gated Jacobi fall-back behind them (see
// icp_kernels.hpp).
void launch_posterior_eigen_tridiag_many(hipStream_t st, int r, int n_all, const EigenRequest* rq_all, const double* const* parts_all,
                                         const int* skip_all, int part) {
  for (int q0 = 0; q0 < n_all; q0 += tri::kTriMany) {
    const int n = std::min(tri::kTriMany, n_all - q0);
    ProfScope _ps(st, KID_EIGEN);
    if (n == 1) launch_tri_sequence<tri::kTriOne>(st, r, n, rq_all + q0, parts_all ? parts_all + q0 : nullptr, skip_all ? skip_all + q0 : nullptr, part, true);
    else launch_tri_sequence<tri::kTriMany>(st, r, n, rq_all + q0, parts_all ? parts_all + q0 : nullptr, skip_all ? skip_all + q0 : nullptr, part, true);
  }
}

// N = D⁻¹ M D⁻¹ (symmetrised) for the in-place kernel
__global__ void __launch_bounds__(256) k_eigen_big_prepare(int r, const double* __restrict__ M, const double* __restrict__ sqrt_lambda,
                                                           double* __restrict__ A, const int* __restrict__ gate) {
  if (gate && gate[0] != 2) return;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= r * r) return;
  const int i = e / r, j = e - i * r;
  A[e] = 0.5 * (M[(size_t)i * r + j] + M[(size_t)j * r + i]) / (sqrt_lambda[i] * sqrt_lambda[j]);
}

static void launch_eigen_big(hipStream_t st, int r, const double* M, const double* sqrt_lambda, const double* Vwarm, double* V, double* Vt,
                             double* S, double* work, int* status, int* host_status, const int* gate) {
  const size_t n2 = ((size_t)r + 1) & ~(size_t)1, rr = (size_t)r * r;
  double* A0 = work;
  double* T = work + rr;
  double* Vwork = work + 2 * rr;
  double* mu = work + 3 * rr;
  double* rotlog = mu + n2;
  int* meta = (int*)(rotlog + (size_t)kEigenMaxSweeps * (n2 - 1) * n2);
  const int eb = (int)((rr + 255) / 256);
  // (as the tridiagonal route's fall-back — `gate` — the matrix is in place already: k_tridiag has written N = D⁻¹MD⁻¹, entry by
  // entry the values of the launch below, to the head of `work` for its refinement step, which only reads it)
  if (!gate) hipLaunchKernelGGL(k_eigen_big_prepare, dim3(eb), dim3(256), 0, st, r, M, sqrt_lambda, A0, gate);
  if (Vwarm) {  // A0 <- Vwarmᵀ·A0·Vwarm
    hipLaunchKernelGGL(k_eigen_big_warm, dim3(eb), dim3(256), 0, st, r, (const double*)A0, Vwarm, T, 0);
    hipLaunchKernelGGL(k_eigen_big_warm, dim3(eb), dim3(256), 0, st, r, (const double*)T, Vwarm, A0, 1);
  }
  const size_t half = n2 / 2;
  const bool square = r <= 140;  // the full n × (n|1) image fits one CU's LDS
  const size_t lds_iter = sizeof(double) * ((square ? (size_t)r * (r | 1) : (size_t)r * (r - 1) / 2) + r + 2 * half);
  const size_t lds_replay = sizeof(double) * ((size_t)kBigSlabRows * r + std::max(2 * (size_t)kBigStageRounds * half, (size_t)16 * r));
  const size_t shmem = std::max(lds_iter, lds_replay);
  static size_t lds_granted[2] = {0, 0};
  if (shmem > lds_granted[square]) {
    if (square) set_dyn_lds((const void*)k_eigen_big<true>, shmem); else set_dyn_lds((const void*)k_eigen_big<false>, shmem);
    lds_granted[square] = shmem;
  }
  static std::atomic<int> launch_counter{0};
  const int launch_id = 1 + (int)((unsigned)(++launch_counter) % kPwIdMask);
  static const int sweeps_cap = dev_env("ICP_EIGEN_MAX_SWEEPS") ? std::atoi(dev_env("ICP_EIGEN_MAX_SWEEPS")) : kEigenMaxSweeps;
  static const int no_corr = dev_env("ICP_EIGEN_NO_CORRECTION") != nullptr;
  const int nb = (r + kBigSlabRows - 1) / kBigSlabRows;
  double* xcorr = T;  // (the warm transform's scratch is free once the iteration starts)
  if (square)
    hipLaunchKernelGGL(k_eigen_big<true>, dim3(1 + nb), dim3(1024), shmem, st, r, (const double*)A0, Vwarm, Vwork, mu, rotlog, xcorr, meta,
                       std::min(sweeps_cap, kEigenMaxSweeps), no_corr, launch_id, status, gate);
  else
    hipLaunchKernelGGL(k_eigen_big<false>, dim3(1 + nb), dim3(1024), shmem, st, r, (const double*)A0, Vwarm, Vwork, mu, rotlog, xcorr, meta,
                       std::min(sweeps_cap, kEigenMaxSweeps), no_corr, launch_id, status, gate);
  // (as a fall-back the sort runs only if the iteration did: its progress word carries this launch's id then)
  hipLaunchKernelGGL(k_eigen_big_finish, dim3(r), dim3(64), 0, st, r, (const double*)Vwork, (const double*)mu, V, Vt, S, (const int*)status,
                     host_status, gate ? (const int*)meta : nullptr, launch_id);
}

void eigen_debug_dump(const double* work, int r) {  // developer aid: convergence trace of the last decomposition on `work`
  const size_t n2 = ((size_t)r + 1) & ~(size_t)1;
  const size_t log_doubles = ((size_t)kEigenMaxSweeps * (n2 - 1) + 2) * n2;
  double tr[8];
  (void)hipMemcpy(tr, (const char*)(work + log_doubles + n2 * 64) + 80 * sizeof(int), sizeof(tr), hipMemcpyDeviceToHost);
  std::fprintf(stderr, "[icp eigen] off^2/diag^2 after sweeps 1..: %.2e %.2e %.2e %.2e %.2e\n", tr[0], tr[1], tr[2], tr[3], tr[4]);
  int hist[16];
  (void)hipMemcpy(hist, (const char*)(work + log_doubles + n2 * 64) + 100 * sizeof(int), sizeof(hist), hipMemcpyDeviceToHost);
  std::fprintf(stderr, "[icp eigen] decompositions by sweep count 1..8: %d %d %d %d %d %d %d %d\n", hist[1], hist[2], hist[3], hist[4], hist[5], hist[6], hist[7], hist[8]);
}

bool eigen_speculation_supported(int r) { return r >= 3 && r <= 64 && dev_env("ICP_EIGEN_GENERIC") == nullptr; }

namespace {
// workgroups per problem: the iteration + the replay (32 rows each)
inline int eigen_rr_per(int r) { return 1 + (r + kReplayRows - 1) / kReplayRows; }
inline EigenProblem eigen_rr_problem(int r, const EigenRequest& rq) {
  const int n2 = (r + 1) & ~1;
  // work = [rotation log | sign exchange | meta: progress word, counters, rank per position]
  const size_t log_doubles = ((size_t)kEigenMaxSweeps * (n2 - 1) + 2) * n2;
  static std::atomic<int> launch_counter{0};  // (any value the previous launch on this `work` did not use would do)
  double* vpos = rq.work + log_doubles;
  const int launch_id = 1 + (int)((unsigned)(++launch_counter) % kPwIdMask);  // never 0: the idle value of the progress word
  return EigenProblem{rq.M, rq.Vwarm, rq.V, rq.Vt, rq.S, rq.status, rq.work, (int*)(vpos + (size_t)n2 * 64), vpos,
                      rq.spec ? *rq.spec : EigenSpec{0, nullptr, 0, nullptr, 0, nullptr}, launch_id, rq.host_status, rq.done_word,
                      rq.done_value, rq.sqrt_lambda};
}
template <class Batch>
void launch_eigen_rr_batch(hipStream_t st, int r, const double* sqrt_lambda, int n, const Batch& batch) {
  // fixed-position variant: A, V and the rotation table double-buffered in LDS
  const int n2 = (r + 1) & ~1;
  const int ldk = 66;  // ldk: 64 coordinates per position row, rows 16 B apart modulo the 256-B bank window
  const size_t szV = (size_t)n2 * ldk;
  const size_t shmem = sizeof(double) * ((size_t)kRrOV + 2 * szV);
  static const int sweeps_cap = dev_env("ICP_EIGEN_MAX_SWEEPS") ? std::atoi(dev_env("ICP_EIGEN_MAX_SWEEPS")) : kEigenMaxSweeps;
  static bool lds_set = false;
  set_dyn_lds_once((const void*)k_posterior_eigen_rr<Batch>, sizeof(double) * ((size_t)kRrOV + 2 * 64 * 66), &lds_set);
  ProfScope _ps(st, KID_EIGEN);
  // per problem: workgroup 0 iterates, workgroup 1 replays its rotations on V as the sweeps are published
  static const int no_corr = dev_env("ICP_EIGEN_NO_CORRECTION") != nullptr;
  hipLaunchKernelGGL(k_posterior_eigen_rr<Batch>, dim3(n * eigen_rr_per(r)), dim3(1024), shmem, st, r, sqrt_lambda, ldk,
                     std::min(sweeps_cap, kEigenMaxSweeps), no_corr, batch);
}
template <int CAP>
void launch_eigen_rr(hipStream_t st, int r, const double* sqrt_lambda, int n, const EigenRequest* rq) {
  EigenBatch<CAP> batch{};
  batch.n = n;
  for (int i = 0; i < n; ++i) batch.p[i] = eigen_rr_problem(r, rq[i]);
  launch_eigen_rr_batch(st, r, sqrt_lambda, n, batch);
}
}  // namespace

// ---------------------------------------------------------------- opt-in: the Cholesky-root sampler (ranks <= 64)
// The reference draws posterior.sample() in the eigenbasis of the posterior covariance (D M⁻¹ D = V S Vᵀ: the numbers z multiply
// the columns of V√S) — that is what the kernels above are for, and what parity with the reference needs.  ANY square root W of
// D M⁻¹ D gives a sample of the same distribution, and the transition density does not depend on the root: with
// M = L Lᵀ, W = D L⁻ᵀ, i.e. D⁻¹ W z = L⁻ᵀ z — ONE back substitution per proposal (propose_body), no decomposition, no inverse.
// This kernel writes the factor where the decomposition would write its basis — V := L (lower triangular, row-major), S := 1/diag(L)
// — with the same completion protocol and the same front end for a launch enqueued ahead of its input, so the machinery around
// it (speculation, completion words, batches) is unchanged.  One workgroup per posterior; the factorisation is the chain step's own
// (factor_reg_body: 2×4 register tiles, one barrier per column).  No iteration, no warm start, no state from one posterior to the
// next: ≈ 15 µs at rank 51 against 70-110 µs for the warm-started decomposition.
// (icp_proposal_set_sampler; NOT the default: the chain it produces is a different realisation of the same Markov kernel.)
struct RootBatch2 {
  int n; EigenProblem p[2];
  __device__ __forceinline__ void announce() const {}
  __device__ __forceinline__ bool skipped(int) const { return false; }
};
typedef EigenBatchMem RootBatchMem;

template <class Batch, int NT>
__global__ void __launch_bounds__(NT) k_posterior_root(int r, Batch batch) {
  batch.announce();
  if (batch.skipped(blockIdx.x)) return;
  const EigenProblem pb = batch.p[blockIdx.x];
  __shared__ int s_cancel;
  const int tid = threadIdx.x;
  const EigenSpec spec = pb.spec;
  EIG_STAMP(0);
  if (tid == 0) s_cancel = 0;
  __syncthreads();
  if (tid == NT - 1) {  // (the protocol of k_posterior_eigen_rr: wait for the input, or for the cancellation, or give up after 5 ms)
    if (spec.ready) {
      const long long t0 = __builtin_amdgcn_s_memrealtime();  // 100 MHz
      for (;;) {
        if (__hip_atomic_load(spec.ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - spec.ready_seq >= 0) break;
        if (spec.cancel && __hip_atomic_load(spec.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == spec.seq) { s_cancel = 1; break; }
        if (__builtin_amdgcn_s_memrealtime() - t0 > 500000) { s_cancel = 2; break; }
        __builtin_amdgcn_s_sleep(32);
      }
      if (spec.wait_ticks) atomicAdd((unsigned long long*)spec.wait_ticks, (unsigned long long)(__builtin_amdgcn_s_memrealtime() - t0));
    } else if (spec.cancel) {
      if (__hip_atomic_load(spec.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == spec.seq) s_cancel = 1;
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // (acquire side for the plain loads of the partials below)
  if (s_cancel) {
    if (tid == 0) {
      if (s_cancel == 2) {
        if (pb.host_status) __hip_atomic_store(pb.host_status, kEigenGaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        pb.Vout[0] = __builtin_nan("");
      }
      __threadfence();
      if (pb.done_word) __hip_atomic_store(pb.done_word, pb.done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  EIG_STAMP(1);
  // the factor kernel's own body; its by-products (assembled M, α) go to this problem's scratch (`rotlog` = the proposal's work buffer)
  double* scratch = pb.rotlog;
  const bool ok = factor_reg_body<1, NT>(r, pb.M, spec.splits, scratch, scratch + (size_t)r * r, (int*)(scratch + (size_t)r * r + r),
                                         -1, nullptr, spec.splits > 0 ? nullptr : pb.M, false);
  EIG_STAMP(3);
  // ---- V := L = L̃·D̃^{1/2} (L_ik = w_ik / sqrt(d_k), L_kk = sqrt(d_k)), Vt := Lᵀ, S := 1 / L_kk
  const int ld = r | 1;
  const double* W = s_dyn;
  if (ok) {
    for (int e = tid; e < r * r; e += NT) {
      const int i = e / r, k = e - i * r;
      const double v = k <= i ? W[(size_t)i * ld + k] * fast_rsqrt(W[(size_t)k * ld + k]) : 0.0;
      pb.Vout[(size_t)i * r + k] = v;
      pb.Vtout[(size_t)k * r + i] = v;
    }
    if (tid < r) pb.Sout[tid] = fast_rsqrt(W[(size_t)tid * ld + tid]);
  }
  EIG_STAMP(4);
  if (tid == 0) {
    pb.status[0] = ok ? 0 : 2; pb.status[-1] = 0;
    if (pb.host_status) __hip_atomic_store(pb.host_status, ok ? 0 : 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __threadfence();
  __syncthreads();
  if (tid == 0 && pb.done_word) __hip_atomic_store(pb.done_word, pb.done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  EIG_STAMP(5);
}

namespace {
template <class Batch>
void launch_root_batch(hipStream_t st, int r, int n, const Batch& batch) {
  ProfScope _ps(st, KID_EIGEN);
  const size_t shmem = sizeof(double) * (size_t)(r + 1) * (r | 1);
  if (factor_tile_count(r) <= 256) {
    set_dyn_lds((const void*)k_posterior_root<Batch, 256>, shmem);
    hipLaunchKernelGGL((k_posterior_root<Batch, 256>), dim3(n), dim3(256), shmem, st, r, batch);
  } else {
    set_dyn_lds((const void*)k_posterior_root<Batch, 1024>, shmem);
    hipLaunchKernelGGL((k_posterior_root<Batch, 1024>), dim3(n), dim3(1024), shmem, st, r, batch);
  }
}
}  // namespace

bool launch_posterior_eigen_pair(hipStream_t st, int r, const double* sqrt_lambda, int n, const EigenRequest* rq) {
  static const bool force_generic = dev_env("ICP_EIGEN_GENERIC") != nullptr;
  if (!(r >= 3 && r <= 64 && !force_generic) || n < 1 || n > kEigenPairMax) return false;
  if (rq[0].root) {  // the Cholesky-root sampler (icp_proposal_set_sampler): no decomposition at all
    if (n > 2) return false;  // (its lanes are decomposed one call after the other)
    RootBatch2 b{};
    b.n = n;
    for (int i = 0; i < n; ++i) b.p[i] = eigen_rr_problem(r, rq[i]);
    launch_root_batch(st, r, n, b);
    return true;
  }
  // (the warm-started iteration; a direct route at these ranks was measured and lost: DESIGN.md §11)
  if (n <= 2) launch_eigen_rr<2>(st, r, sqrt_lambda, n, rq);
  else launch_eigen_rr<kEigenPairMax>(st, r, sqrt_lambda, n, rq);  // both lanes of a twin pass: the same bodies, a longer record
  return true;
}

size_t eigen_many_record_bytes(int n) { return sizeof(EigenProblem) * (size_t)n; }

EigenProblem eigen_problem_of(int r, const EigenRequest& rq) { return eigen_rr_problem(r, rq); }

void launch_posterior_eigen_resident(hipStream_t st, int r, int n, const EigenProblem* records, const int* skip, int root) {
  if (n < 1) return;
  EigenBatchMem b{n, records, nullptr};
  b.skip = skip;
  if (root) launch_root_batch(st, r, n, b);
  else launch_eigen_rr_batch(st, r, nullptr, n, b);
}

int launch_posterior_eigen_many(hipStream_t st, int r, int n, const EigenRequest* rq, void* pinned_records, int* arrive) {
  static const bool force_generic = dev_env("ICP_EIGEN_GENERIC") != nullptr;
  if (!(r >= 3 && r <= 64 && !force_generic) || n < 1) return -1;
  // ONE launch while all of its workgroups can be resident together on an otherwise idle chip (a replay workgroup waits for its
  // neighbour at the sign exchange): 240 workgroups; more problems than that follow in a second launch on the same stream
  // (test hook ICP_TEST_EIGEN_CHUNK: round 2's 24 per launch, for tools/r3_timeout_repro.py)
  static const int chunk_hook = dev_env("ICP_TEST_EIGEN_CHUNK") ? std::atoi(dev_env("ICP_TEST_EIGEN_CHUNK")) : 0;
  const int per = eigen_rr_per(r), chunk = chunk_hook > 0 ? chunk_hook : 240 / per;
  EigenProblem* rec = (EigenProblem*)pinned_records;
  for (int i = 0; i < n; ++i) rec[i] = eigen_rr_problem(r, rq[i]);
  if (rq[0].root) {  // (all requests of a batch share the sampler: checked by the caller)
    launch_root_batch(st, r, n, RootBatchMem{n, rec, arrive});
    return n;
  }
  for (int i = 0; i < n; i += chunk) {
    const int m = std::min(chunk, n - i);
    launch_eigen_rr_batch(st, r, nullptr, m, EigenBatchMem{m, rec + i, arrive});
  }
  return n * per;
}

void launch_posterior_eigen(hipStream_t st, int r, const double* M, const double* sqrt_lambda, const double* Vwarm, double* V,
                            double* Vt, double* S, double* work, int* status, const EigenSpec* spec, int* host_status, int part) {
  if (tridiag_route(r)) {
    if (spec != nullptr) {  // (the route takes no spec; such a call is not split either)
      if (part == 2) return;
      part = 0;
    }
    const EigenRequest rq{M, nullptr, V, Vt, S, work, status, nullptr, host_status, nullptr, 0, sqrt_lambda};
    ProfScope _ps(st, KID_EIGEN);
    launch_tri_sequence<tri::kTriOne>(st, r, 1, &rq, nullptr, nullptr, part, false);
    if (part == 1) return;
    // eigenvalues that multisection could not tell apart (status 2: a spectrum with (near-)multiple eigenvalues, e.g. a posterior without
    // correspondences over a model with equal variances): the Jacobi iteration takes over, cold, in the same stream — its launches
    // return at once otherwise — on the matrix the reduction left at the head of `work`
    if (r <= kBigMaxRank) launch_eigen_big(st, r, M, sqrt_lambda, nullptr, V, Vt, S, work, status, nullptr, status);
    else  // (matrix behind L2: `work`'s head, whose refinement matrices a failed multisection has no use for)
      hipLaunchKernelGGL(k_posterior_eigen, dim3(1), dim3(1024), 0, st, r, M, sqrt_lambda, (const double*)nullptr, V, Vt, S, work, status, 0, 0,
                         (const int*)status);
    launch_tri_done<tri::kTriOne>(st, 1, &rq, nullptr);
    return;
  }
  if (part == 2) return;  // (the other routes are not split: part 1 has issued all of them)
  {
    const EigenRequest rq{M, Vwarm, V, Vt, S, work, status, spec, host_status, nullptr, 0};
    if (launch_posterior_eigen_pair(st, r, sqrt_lambda, 1, &rq)) return;
  }
  if (r > 64 && r <= kBigMaxRank) {  // in-place parallel Jacobi, packed triangle in one CU's LDS + replay workgroups
    ProfScope _ps(st, KID_EIGEN);
    launch_eigen_big(st, r, M, sqrt_lambda, Vwarm, V, Vt, S, work, status, host_status, nullptr);
    return;
  }
  // ranks above 200: the generic single-workgroup kernel (matrix behind L2)
  const int ld = r | 1;
  const size_t budget = (size_t)kLdsDoubles - 1800;  // static LDS of the kernel
  const int a_in_lds = (size_t)r * ld <= budget;
  const int v_in_lds = 2 * (size_t)r * ld <= budget;
  const size_t shmem = sizeof(double) * ((a_in_lds ? (size_t)r * ld : 0) + (v_in_lds ? (size_t)r * ld : 0));
  if (!a_in_lds) Vwarm = nullptr;  // the warm-start transform needs `work` as scratch
  set_dyn_lds((const void*)k_posterior_eigen, shmem);
  { ProfScope _ps(st, KID_EIGEN);
    hipLaunchKernelGGL(k_posterior_eigen, dim3(1), dim3(1024), shmem, st, r, M, sqrt_lambda, Vwarm, V, Vt, S, work, status, a_in_lds,
                       v_in_lds); }
}

}  // namespace icp
