// kernels_posterior.hip — correspondences -> GP regression -> r-space closed forms.
//
// Math: SURVEY.md App. A.  With Q = Φ·diag(√λ), per-correspondence noise Σ_i = σ_t² I + (σ_n² − σ_t²) n̂n̂ᵀ
// (SurfaceNoiseHelpers.scala:32-60 for an orthonormal frame), so Σ_i⁻¹ = w_t I + κ n̂n̂ᵀ, w_t = 1/σ_t², κ = 1/σ_n² − 1/σ_t²:
//   M = I + Σ_i Q_iᵀ Σ_i⁻¹ Q_i,  b = Σ_i Q_iᵀ Σ_i⁻¹ (y_i − μ_i),  α = M⁻¹ b            (NonRigidIcpProposal.scala:152)
//   propose:   c_new = (G + σ²I)⁻¹ G (α + D⁻¹ V √S z),  D M⁻¹ D = V S Vᵀ, G = QᵀQ, σ² = 1e-5      (:53-68)
//   transition: log T = −½ γᵀMγ − (r/2) ln 2π,  (G + σ²M) γ = G (c̃ − α)                           (:71-85)
//     (equal to the reference's whitened-coefficient form for ANY square root of D M⁻¹ D; derivation in DESIGN.md)
// These kernels are latency-bound r×r work (r = 51…201): one workgroup per matrix, data in LDS when it fits.
// The Cholesky factor kernels live in kernels_factor.hip, the posterior KL basis (Jacobi, tridiagonal route, Cholesky-root sampler) in
// kernels_eigen.hip.
#include <algorithm>
#include <cstdlib>

#include "icp_kernels.hpp"
#include "icp_dense.hpp"

namespace icp {

namespace {

// ---------------------------------------------------------------- correspondences (one thread per correspondence)

// (init: the memo entry's copy of the state's coefficients and its cleared status words, by the launch's first workgroup — as
// runtime copy / fill operations they were two more dependent submissions of ≈ 5 µs each on every posterior's path)
__device__ __forceinline__ void entry_init(const EntryInit& init) {
  if (blockIdx.x != 0 || !init.coeffs_dst) return;
  for (int i = threadIdx.x; i < init.r; i += blockDim.x) init.coeffs_dst[i] = init.coeffs_src[i];
  if (threadIdx.x < 3) init.status[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(kBlock) k_correspond_model(CorrTask c, const double* __restrict__ cp, EntryInit init) {
  entry_init(init);
  int k = blockIdx.x * kBlock + threadIdx.x;
  if (k < c.K) correspond_model_one(c, k, ld3(cp + 3 * k));
}

__global__ void __launch_bounds__(kBlock) k_correspond_target(CorrTask c, const int* __restrict__ nn_id, EntryInit init) {
  entry_init(init);
  int k = blockIdx.x * kBlock + threadIdx.x;
  if (k < c.K) correspond_target_one(c, k, nn_id[k]);
}

__global__ void __launch_bounds__(64) k_regression_mfma(int K, int kchunk, int r, const double* __restrict__ Q, CorrBuffers cb,
                                                         double wt, double kappa, double* __restrict__ Mpart) {
  // (blockIdx.x = split, .y = tile: with 64 splits every tile of a split runs on the XCD "split mod 8" — workgroups go to the XCDs
  // round robin by linear index — and the split's gathered basis rows are fetched into ONE L2; see step_regression_body)
  regression_tile(blockIdx.y, blockIdx.x, K, kchunk, r, Q, cb, wt, kappa, Mpart);
}

// Σ of the split-K partials of up to kFactorMax posteriors into their first partial, on many CUs, in split order (the order of the
// factor kernels' own loops)
struct PartialSumArgs { int n; int nn; double* Mpart[kFactorMax]; int splits[kFactorMax]; };
__global__ void __launch_bounds__(256) k_sum_partials(PartialSumArgs a) {
  const int which = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (which >= a.n || e >= a.nn) return;
  double* P = a.Mpart[which];
  const int S = a.splits[which];
  double acc = 0.0;
  for (int s0 = 0; s0 < S; s0 += 8) {  // eight splits in flight
    double q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) q[u] = P[(size_t)min(s0 + u, S - 1) * a.nn + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) if (s0 + u < S) acc += q[u];
  }
  P[e] = acc;
}

constexpr int kTailMax = 2 * kWideMaxChains;  // tails per launch (a wide step: forward and backward of every chain)
struct TailArgs {
  int n;
  const int* relay_in[kTailMax];
  int* relay_out[kTailMax];
  const double* alpha[kTailMax];
  const double* M[kTailMax];
  const double* c_from[kTailMax];
  const double* c_to[kTailMax];
  double step[kTailMax];
  double* out[kTailMax];
  int* status[kTailMax];
};

template <int NT>
__global__ void __launch_bounds__(NT) k_transition_tails(int r, TailArgs ta, const double* __restrict__ Ginv, double sigma2,
                                                          int n_lds, int tpr_log2) {
  const int t = blockIdx.x;
  if (ta.relay_in[t] && threadIdx.x < 3) ta.relay_out[t][threadIdx.x] = ta.relay_in[t][threadIdx.x];
  if (NT == 1024) __builtin_amdgcn_s_setprio(3);  // (ranks above 134: beside the evaluator's searches, like the factorisation)
  tail_body(r, ta.alpha[t], ta.M[t], ta.c_from[t], ta.c_to[t], ta.step[t], ta.out[t], ta.status[t], Ginv, sigma2, n_lds, tpr_log2);
}

__global__ void __launch_bounds__(1024) k_transition_tail_direct(int r, const double* __restrict__ alpha, const double* __restrict__ M,
                                                                  const double* __restrict__ G, double sigma2,
                                                                  const double* __restrict__ c_from, const double* __restrict__ c_to,
                                                                  double step, double* __restrict__ work, double* __restrict__ out,
                                                                  int* __restrict__ status, int use_lds) {
  __shared__ double s_d[512], s_dinv[512], s_red[16];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int ld = use_lds ? (r | 1) : r;
  double* W = use_lds ? s_dyn : work;  // rows 0..r-1 = G + σ²M, row r = (G d)ᵀ
  for (int j = tid; j < r; j += nt) s_d[j] = (c_from[j] + (c_to[j] - c_from[j]) / step) - alpha[j];
  __syncthreads();
  for (int e = tid; e < r * r; e += nt) {
    const int i = e / r, j = e - i * r;
    W[(size_t)i * ld + j] = fma(sigma2, M[e], G[e]);
  }
  for (int i = tid; i < r; i += nt) {
    double s = 0.0;
    for (int j = 0; j < r; ++j) s = fma(G[(size_t)j * r + i], s_d[j], s);
    W[(size_t)r * ld + i] = s;
  }
  __syncthreads();
  const bool ok = block_cholesky_rootfree(W, r, ld, 1, 5);
  if (!ok) { if (tid == 0) status[0] = 1; return; }
  for (int j = tid; j < r; j += nt) {
    const double d = fast_rsqrt(W[(size_t)j * ld + j]);
    s_dinv[j] = d;
    s_d[j] = W[(size_t)r * ld + j] * d;
  }
  __syncthreads();
  for (int j = r - 1; j >= 0; --j) {
    if (tid == 0) s_d[j] = s_d[j] * s_dinv[j];
    __syncthreads();
    const double xj = s_d[j];
    for (int i = tid; i < j; i += nt) s_d[i] = fma(-(W[(size_t)j * ld + i] * s_dinv[i]), xj, s_d[i]);
    __syncthreads();
  }
  double part = 0.0;
  for (int i = tid; i < r; i += nt) {
    double s = 0.0;
    for (int j = 0; j < r; ++j) s = fma(M[(size_t)j * r + i], s_d[j], s);
    part = fma(s_d[i], s, part);
  }
  const double q = block_sum(part, s_red);
  if (tid == 0) { out[0] = -0.5 * q - 0.5 * (double)r * 1.8378770664093453; status[0] = 0; }
}

// ---------------------------------------------------------------- a8 propose
// c_new = (G + σ²I)⁻¹ G w = w − σ² P w with P = (G + σ²I)⁻¹ precomputed;  w = α + D⁻¹ V (√S ∘ z)

template <int NT>
__global__ void __launch_bounds__(NT) k_propose(int r, ProposeIn in, double* __restrict__ c_out, int tpr_log2, const int* relay_in,
                                                int* relay_out) {
  if (relay_in && threadIdx.x < 3) relay_out[threadIdx.x] = relay_in[threadIdx.x];
  propose_body<true>(r, in, c_out, tpr_log2);
}

// ---------------------------------------------------------------- deterministic ICP helpers

__global__ void __launch_bounds__(kBlock) k_gather_points(int K, const double* __restrict__ x, const int* __restrict__ ids,
                                                           double* __restrict__ P) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  const int i = ids[k];
  P[3 * k] = x[3 * i]; P[3 * k + 1] = x[3 * i + 1]; P[3 * k + 2] = x[3 * i + 2];
}

__global__ void __launch_bounds__(kBlock) k_correspond_plain(int K, const int* __restrict__ ids, const double* __restrict__ pts,
                                                              const double* __restrict__ ref, const double* __restrict__ mean, CorrBuffers cb) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  const int id = ids[k];
  cb.id[k] = id; cb.aux[k] = -1; cb.keep[k] = 1;
  for (int d = 0; d < 3; ++d) {
    const double p = pts[3 * k + d];
    cb.pt[3 * k + d] = p;
    cb.nhat[3 * k + d] = 0.0;
    cb.e[3 * k + d] = (p - ref[3 * id + d]) - mean[3 * id + d];  // the regression sees world-space points (IcpBasedSurfaceFitting.scala:81)
  }
}

__global__ void __launch_bounds__(256) k_mean_step(int r, const double* __restrict__ alpha, const double* __restrict__ P, double sigma2,
                                                    double step, double* __restrict__ c, int tpr_log2) {
  __shared__ double s_a[512], s_y[512];
  for (int i = threadIdx.x; i < r; i += blockDim.x) s_a[i] = alpha[i];
  __syncthreads();
  block_matvec(r, P, r, s_a, s_y, tpr_log2);
  for (int i = threadIdx.x; i < r; i += blockDim.x) {
    const double cnew = fma(-sigma2, s_y[i], s_a[i]);   // model.coefficients(posterior.mean) (:84)
    c[i] = c[i] + (cnew - c[i]) * step;                 // :85
  }
}

}  // namespace

void launch_correspond_model(hipStream_t st, int K, const double* x, const double* cp, const int* nnv,
                             const unsigned char* tgt_boundary, int boundary_aware, const Pose& pose,
                             const double* ref, const double* mean, const int* tris, const int* adj_off,
                             const int* adj, const CorrBuffers& cb, const EntryInit& init) {
  if (K <= 0) return;
  CorrTask c{K, cb, x, nullptr, tgt_boundary, nnv, boundary_aware, pose, ref, mean, tris, adj_off, adj};
  ProfScope _ps(st, KID_CORRESPOND);
  hipLaunchKernelGGL(k_correspond_model, dim3(cdiv(K, kBlock)), dim3(kBlock), 0, st, c, cp, init);
}

void launch_correspond_target(hipStream_t st, int K, const double* x, const double* tpts, const int* nn_id,
                              const unsigned char* model_boundary, int boundary_aware, const Pose& pose,
                              const double* ref, const double* mean, const int* tris, const int* adj_off,
                              const int* adj, const CorrBuffers& cb, const EntryInit& init) {
  if (K <= 0) return;
  CorrTask c{K, cb, x, tpts, model_boundary, nullptr, boundary_aware, pose, ref, mean, tris, adj_off, adj};
  ProfScope _ps(st, KID_CORRESPOND);
  hipLaunchKernelGGL(k_correspond_target, dim3(cdiv(K, kBlock)), dim3(kBlock), 0, st, c, nn_id, init);
}

int regression_splits(int K) {
  int s = (K + 7) / 8;  // ~8 correspondences per wave: two gather rounds on its dependent chain, many waves to overlap them
  return s < 1 ? 1 : (s > 64 ? 64 : s);
}

int regression_fold(int K, int r, int n_posteriors_in_launch) {
  // (developer switches: ICP_REGRESSION_FOLD_TILES = output tiles from which a launch folds, ICP_REGRESSION_FOLD_K = … or posteriors of at
  // most this many correspondences fold whatever the launch carries)
  static const int min_tiles = dev_env("ICP_REGRESSION_FOLD_TILES") ? std::atoi(dev_env("ICP_REGRESSION_FOLD_TILES")) : 512;
  static const int small_k = dev_env("ICP_REGRESSION_FOLD_K") ? std::atoi(dev_env("ICP_REGRESSION_FOLD_K")) : 0;
  const int S = regression_splits(K);
  if (S <= 1) return 1;
  // femur-size matrices (4 x 4 tiles, 13 leaves) keep their split-K: 64 chains a launch measured 186k it/s folded against 204k split
  // (same box, alternating) — their partials are small, and 16,640 one-leaf waves hide the gathers' latency better than 1,280 thirteen-leaf ones
  static const int min_rank_tiles = dev_env("ICP_REGRESSION_FOLD_RANK_TILES") ? std::atoi(dev_env("ICP_REGRESSION_FOLD_RANK_TILES")) : 6;
  if (((r + 1 + 15) >> 4) < min_rank_tiles && K > small_k) return 1;
  const long tiles = (long)regression_tiles(r) * std::max(n_posteriors_in_launch, 1);
  return (tiles >= min_tiles || K <= small_k) ? S : 1;
}

int regression_macro(int r, int fold) {
  static const int forced = dev_env("ICP_REGRESSION_MACRO") ? std::atoi(dev_env("ICP_REGRESSION_MACRO")) : 0;  // (developer switch: 1, 2)
  if (fold <= 1) return 1;
  const int nt = (r + 1 + 15) >> 4;
  if (forced >= 1 && forced <= 2) return nt >= forced ? forced : 1;
  // (measured, 30 face-model chains a launch — 13 x 13 tiles, K = 400: single tiles 361 µs, 2 x 2 macro tiles 206 µs, 3 x 3 336 µs (few waves,
  // each a long chain of gathers); femur-size matrices (4 x 4 tiles) stay with single tiles: three macro units per posterior are too few waves)
  return nt >= 6 ? 2 : 1;
}
int regression_units(int r, int leaves, int fold, int macro) {
  if (fold > 1 && macro > 1) return regression_macro_tiles(r, macro);
  return regression_tiles(r) * (leaves / std::max(fold, 1));
}

void launch_regression(hipStream_t st, int K, int r, const double* Q, const CorrBuffers& cb, double w_tangent,
                       double kappa, double* Mpart, int* splits_out) {
  const int S = regression_splits(K);
  int kchunk = (K + S - 1) / S;
  if (kchunk < 1) kchunk = 1;
  *splits_out = S;
  { ProfScope _ps(st, KID_REGRESSION);
    hipLaunchKernelGGL(k_regression_mfma, dim3(S, regression_tiles(r)), dim3(64), 0, st, K, kchunk, r, Q, cb, w_tangent, kappa, Mpart); }
}

__global__ void __launch_bounds__(256) k_assemble_posterior_matrix(int r, const double* __restrict__ P, double* __restrict__ M) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= r * r) return;
  const int i = e / r, j = e - i * r;
  const int hi = max(i, j), lo = min(i, j);
  M[e] = P[(size_t)hi * (r + 1) + lo] + (i == j ? 1.0 : 0.0);  // (the values the factor kernels' own assembly writes)
}

void launch_sum_partials(hipStream_t st, int r, double* Mpart, int splits) {
  if (splits <= 1) return;
  PartialSumArgs ra{};
  ra.nn = (r + 1) * (r + 1);
  ra.n = 1;
  ra.Mpart[0] = Mpart;
  ra.splits[0] = splits;
  hipLaunchKernelGGL(k_sum_partials, dim3(cdiv(ra.nn, 256), 1), dim3(256), 0, st, ra);
}
void launch_sum_partials_many(hipStream_t st, int r, int n, double* const* Mpart, const int* splits) {
  PartialSumArgs ra{};
  ra.nn = (r + 1) * (r + 1);
  for (int i = 0; i < n && i < kFactorMax; ++i)
    if (splits[i] > 1) { ra.Mpart[ra.n] = Mpart[i]; ra.splits[ra.n] = splits[i]; ++ra.n; }
  if (ra.n) hipLaunchKernelGGL(k_sum_partials, dim3(cdiv(ra.nn, 256), ra.n), dim3(256), 0, st, ra);
}
void launch_assemble_posterior_matrix(hipStream_t st, int r, const double* Mpart_summed, double* M) {
  hipLaunchKernelGGL(k_assemble_posterior_matrix, dim3(cdiv(r * r, 256)), dim3(256), 0, st, r, Mpart_summed, M);
}

void launch_transition_tails(hipStream_t st, int r, int n, const TransitionTailIO* io, const double* Ginv, double sigma2) {
  TailArgs ta{};
  ta.n = n;
  for (int t = 0; t < n; ++t) {
    ta.alpha[t] = io[t].alpha; ta.M[t] = io[t].M; ta.c_from[t] = io[t].c_from; ta.c_to[t] = io[t].c_to;
    ta.step[t] = io[t].step; ta.out[t] = io[t].out; ta.status[t] = io[t].status;
    ta.relay_in[t] = io[t].relay_in; ta.relay_out[t] = io[t].relay_out;
  }
  const int ld = r | 1;
  const size_t one = (size_t)r * ld;
  const int n_lds = 2 * one <= (size_t)kLdsDoubles - 2560 ? 2 : (one <= (size_t)kLdsDoubles - 2560 ? 1 : 0);
  const size_t shmem = sizeof(double) * one * n_lds;
  ProfScope _ps(st, KID_TAIL);
  if (n_lds == 0) {
    // neither matrix fits LDS (ranks above 134): every product of the iteration streams 8·r² bytes from L2, 1024 threads keep four
    // times the loads in flight (50 -> ≈ 20 µs at rank 200).  Below, 256 threads: the arithmetic of the merged step's own tails.
    hipLaunchKernelGGL(k_transition_tails<1024>, dim3(n), dim3(1024), 0, st, r, ta, Ginv, sigma2, 0, 4);  // (16 lanes per row: 128-byte segments)
  } else {
    set_dyn_lds((const void*)k_transition_tails<256>, shmem);
    hipLaunchKernelGGL(k_transition_tails<256>, dim3(n), dim3(256), shmem, st, r, ta, Ginv, sigma2, n_lds, matvec_tpr_log2(r, 256));
  }
}

void launch_transition_tail_direct(hipStream_t st, int r, const TransitionTailIO& io, const double* G, double sigma2, double* work) {
  const int ld = r | 1;
  const int use_lds = (size_t)(r + 1) * ld <= (size_t)kLdsDoubles - 1200;
  const size_t shmem = use_lds ? sizeof(double) * (size_t)(r + 1) * ld : 0;
  set_dyn_lds((const void*)k_transition_tail_direct, shmem);
  { ProfScope _ps(st, KID_TAIL);
    hipLaunchKernelGGL(k_transition_tail_direct, dim3(1), dim3(1024), shmem, st, r, io.alpha, io.M, G, sigma2, io.c_from, io.c_to,
                       io.step, work, io.out, io.status, use_lds); }
}

void launch_propose(hipStream_t st, int r, const double* alpha, const double* V, const double* S,
                    const double* inv_sqrt_lambda, const double* P, double sigma2, const double* c,
                    const double* z, double step, double* c_out, int root, const int* relay_in, int* relay_out) {
  { ProfScope _ps(st, KID_PROPOSE);
    ProposeIn in{alpha, V, S, inv_sqrt_lambda, P, c, z, sigma2, step, root};
    // (ranks <= 64: 256 threads, the arithmetic of the merged step's own copy of the proposal; above, only this kernel proposes)
    // (ranks above 134 — no matrix of the proposal fits LDS and no merged step exists —: 1,024 threads, 16 lanes per row of the two
    // products with V and P, whose rows come from L2: 30 -> 14 µs at rank 200)
    if (root && r > 64) hipLaunchKernelGGL(k_propose<1024>, dim3(1), dim3(1024), 0, st, r, in, c_out, matvec_tpr_log2(r, 1024), relay_in, relay_out);
    else if (r > 134) hipLaunchKernelGGL(k_propose<1024>, dim3(1), dim3(1024), 0, st, r, in, c_out, 4, relay_in, relay_out);
    else hipLaunchKernelGGL(k_propose<256>, dim3(1), dim3(256), 0, st, r, in, c_out, matvec_tpr_log2(r, 256), relay_in, relay_out); }
}

void launch_gather_points(hipStream_t st, int K, const double* x, const int* ids, double* P) {
  if (K > 0) hipLaunchKernelGGL(k_gather_points, dim3(cdiv(K, kBlock)), dim3(kBlock), 0, st, K, x, ids, P);
}
void launch_correspond_plain(hipStream_t st, int K, const int* ids, const double* pts, const double* ref, const double* mean,
                             const CorrBuffers& cb) {
  if (K > 0) hipLaunchKernelGGL(k_correspond_plain, dim3(cdiv(K, kBlock)), dim3(kBlock), 0, st, K, ids, pts, ref, mean, cb);
}
void launch_mean_step(hipStream_t st, int r, const double* alpha, const double* P, double sigma2, double step, double* c) {
  hipLaunchKernelGGL(k_mean_step, dim3(1), dim3(256), 0, st, r, alpha, P, sigma2, step, c, matvec_tpr_log2(r, 256));
}

}  // namespace icp
