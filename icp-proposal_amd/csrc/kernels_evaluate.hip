// kernels_evaluate.hip — log values of many states under many evaluators side by side (icp_evaluator_log_values_many; the
// reference's logger scores every named evaluator on every logged sample: JSONAcceptRejectLogger.scala:84-106,
// ProductEvaluators.scala:50-54).
//
// Two kernels beside the batched searches of kernels_metrics.hip.  E1 packs the model-side sample points (ids 0..K-1) of the
// instances that share a target into ONE query list: the target's triangles and spheres then stream once per chunk, not once per
// item — a search's winner is the exact lexicographic (d², index) minimum however its queries are grouped, so no bit moves.  E2 runs
// every reduction of a chunk in one launch (job = blockIdx.x, one workgroup per job): each job takes the strides, the summation order
// and the block reductions of its one-item launcher (launch_sum_gauss_logpdf: 256 threads; launch_dist_max: 1024-element blocks;
// launch_dist_stats: 1024 threads above 4,096 distances, else 256).  The workgroup has 1024 threads; a job of 256 leaves the others
// out of its loop, and what they add to the block reductions — 0.0 to a sum that is never -0.0, -inf to a maximum — changes nothing.
#include "icp_kernels.hpp"
#include "icp_dense.hpp"

namespace icp {

namespace {

constexpr int kGatherBlock = 256;
constexpr int kReduceBlock = 1024;

// E1: P[0 .. 3K) = x[0 .. 3K) of every job (job = blockIdx.y)
__global__ void __launch_bounds__(kGatherBlock) k_eval_gather(const EvalGather* __restrict__ jobs) {
  const EvalGather& j = jobs[blockIdx.y];
  const int i = blockIdx.x * kGatherBlock + threadIdx.x;
  if (i < 3 * j.K) j.P[i] = j.x[i];
}

// Σ_k log N(sqrt(d2_k); mean, sigma): sum_gauss_logpdf_body's loop and block sum at a stride of nt threads
__device__ __forceinline__ void eval_gauss(const EvalReduce& j, int nt, double* s_red) {
  const double lognorm = log(sqrt(2.0 * 3.14159265358979323846)) + log(j.sigma);  // Breeze Gaussian.logNormalizer
  double part = 0.0;
  if ((int)threadIdx.x < nt)
    for (int k = threadIdx.x; k < j.K; k += nt) {
      double d = (sqrt(j.d2[k]) - j.mean) / j.sigma;
      part += -d * d / 2.0 - lognorm;
    }
  const double t = block_sum(part, s_red);
  if (threadIdx.x == 0) j.out[0] = t;
}

// k_dist_max: the maximum of every 1024 consecutive squared distances (block_max), the bit patterns of their roots united by an
// unsigned maximum that starts at zero — here by thread 0 instead of a 64-bit atomic (order-free either way)
__device__ __forceinline__ void eval_max(const EvalReduce& j, double* s_red) {
  unsigned long long best = 0ull;
  for (int k0 = 0; k0 < j.K; k0 += kReduceBlock) {
    const int k = k0 + threadIdx.x;
    double mx = k < j.K ? j.d2[k] : 0.0;
    mx = block_max(mx, s_red);
    const unsigned long long b = d2bits(sqrt(mx));
    best = b > best ? b : best;
  }
  if (threadIdx.x == 0) j.out[0] = bits2d(best);
}

// k_dist_stats / k_met_stats: Σ kept distances, their maximum and count at a stride of nt threads
__device__ __forceinline__ void eval_stats(const EvalReduce& j, int nt, double* s_red) {
  double sum = 0.0, mx = -__builtin_inf(), cnt = 0.0;
  if ((int)threadIdx.x < nt)
    for (int k = threadIdx.x; k < j.K; k += nt) {
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

// E2: one workgroup per job (the job's kind is uniform over the workgroup: no barrier is skipped by a part of it)
__global__ void __launch_bounds__(kReduceBlock) k_eval_reduce(const EvalReduce* __restrict__ jobs) {
  __shared__ double s_red[16];
  const EvalReduce& j = jobs[blockIdx.x];
  if (j.kind == kEvalGauss) eval_gauss(j, 256, s_red);
  else if (j.kind == kEvalMax) eval_max(j, s_red);
  else eval_stats(j, j.K > 4096 ? 1024 : 256, s_red);
}

// ---- the one-item reductions

__global__ void __launch_bounds__(kBlock) k_sum_gauss_logpdf(int K, const double* __restrict__ d2, double mean, double sigma,
                                                              double* __restrict__ out) {
  sum_gauss_logpdf_body(K, d2, mean, sigma, out);
}

__global__ void __launch_bounds__(1024) k_dist_stats(int K, const double* __restrict__ d2, const unsigned char* __restrict__ flags,
                                                        const int* __restrict__ idx, int n_flags, double* __restrict__ out) {
  __shared__ double s_red[16];
  double sum = 0.0, mx = -__builtin_inf(), cnt = 0.0;
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    bool drop = false;
    if (flags) {
      int i = idx ? idx[k] : k;
      drop = (i >= 0 && i < n_flags) ? flags[i] != 0 : false;
    }
    if (!drop) {
      double d = sqrt(d2[k]);
      sum += d;
      mx = fmax(mx, d);
      cnt += 1.0;
    }
  }
  sum = block_sum(sum, s_red);
  cnt = block_sum(cnt, s_red);
  mx = block_max(mx, s_red);
  if (threadIdx.x == 0) { out[0] = sum; out[1] = mx; out[2] = cnt; }
}

// the maximum alone (the Hausdorff evaluator needs nothing else of the list): any number of workgroups, the non-negative doubles'
// bit patterns through a 64-bit atomic maximum — order-independent, so exact; `out_max` must be zero (or a distance) beforehand
__global__ void __launch_bounds__(1024) k_dist_max(int K, const double* __restrict__ d2, double* __restrict__ out_max) {
  __shared__ double s_red[16];
  const int k = blockIdx.x * 1024 + threadIdx.x;
  double mx = k < K ? d2[k] : 0.0;
  mx = block_max(mx, s_red);
  if (threadIdx.x == 0) atomicMax((unsigned long long*)out_max, d2bits(sqrt(mx)));
}

}  // namespace

void launch_eval_gather(hipStream_t st, int n, int kmax, const EvalGather* jobs) {
  if (n <= 0 || kmax <= 0) return;
  hipLaunchKernelGGL(k_eval_gather, dim3(cdiv(3 * kmax, kGatherBlock), n), dim3(kGatherBlock), 0, st, jobs);
}

void launch_eval_reduce(hipStream_t st, int n, const EvalReduce* jobs) {
  if (n <= 0) return;
  ProfScope _ps(st, KID_REDUCE);
  hipLaunchKernelGGL(k_eval_reduce, dim3(n), dim3(kReduceBlock), 0, st, jobs);
}

void launch_sum_gauss_logpdf(hipStream_t st, int K, const double* d2, double mean, double sigma, double* out) {
  { ProfScope _ps(st, KID_REDUCE);
    hipLaunchKernelGGL(k_sum_gauss_logpdf, dim3(1), dim3(kBlock), 0, st, K, d2, mean, sigma, out); }
}

void launch_dist_max(hipStream_t st, int K, const double* d2, double* out_max) {
  if (K <= 0) return;  // (an empty list leaves the zero in place: distances are non-negative)
  ProfScope _ps(st, KID_REDUCE);
  hipLaunchKernelGGL(k_dist_max, dim3((K + 1023) / 1024), dim3(1024), 0, st, K, d2, out_max);
}

void launch_dist_stats(hipStream_t st, int K, const double* d2, const unsigned char* flags, const int* idx,
                       int n_flags, double* out) {
  { ProfScope _ps(st, KID_REDUCE);
    // (one workgroup: the sum has one fixed order; four times the threads where the list is a whole mesh — 40 us per call at 28k points)
    hipLaunchKernelGGL(k_dist_stats, dim3(1), dim3(K > 4096 ? 1024 : kBlock), 0, st, K, d2, flags, idx, n_flags, out); }
}

}  // namespace icp
