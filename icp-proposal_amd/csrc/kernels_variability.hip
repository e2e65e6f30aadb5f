// kernels_variability.hip — posterior variability maps of many chains side by side (icp_posterior_variability_many;
// apps/util/PosteriorVariability.scala:30-73 over LogHelper.logSamples2shapes).
//
// The samples of a call pass through one chunk buffer of fixed size, round by round.  Every launch of a round carries all its work
// (sample group, normal job or map segment = blockIdx.y) and reads its record from a device table made once per call:
//   V1 k_instance_many the sample meshes of the round: up to kInstGroup samples of one model from ONE pass over its basis
//                      (kernels_geometry.hip, shared by every batched entry point)
//   V2 k_var_normals   vertex normals of the samples that need them (mode 2) and of the mode-1 reference meshes
//   V3 k_var_sum       lane = vertex: Σ_s x_s in sample order (and Σ_s n_s in mode 2), carried from round to round in the map's own
//                      buffers; the map's last segment applies the 1/S scale
//   V4 k_var_centred   lane = vertex: the centred second moments in sample order, carried likewise; the last segment writes the map
// The operations are those of the one-map path in its order — instance_point's sums and instance_pose, vertex_normal, k_accumulate's
// add-then-scale, k_variability's two sample loops — and a value carried through memory between two segments is the value a register
// would have held: a map's bits depend neither on the other maps of the call nor on how its samples fall into rounds.
#include "icp_kernels.hpp"
#include "icp_search.hpp"

namespace icp {

namespace {

constexpr int kVarBlock = 128;

// V2: k_vertex_normals of one mesh per blockIdx.y
__global__ void __launch_bounds__(kVarBlock) k_var_normals(const VarNormalJob* __restrict__ jobs) {
  const VarNormalJob& jb = jobs[blockIdx.y];
  const int v = blockIdx.x * kVarBlock + threadIdx.x;
  if (v >= jb.N) return;
  const d3 n = vertex_normal(jb.x, jb.tris, jb.adj_off, jb.adj, v);
  jb.out[3 * v] = n.x; jb.out[3 * v + 1] = n.y; jb.out[3 * v + 2] = n.z;
}

// V3: k_variability's first loop (m += x_s, then m *= 1/S) and, in mode 2, the launch_accumulate chain of the sample normals
// (acc = acc + n_s from 0, the last one scaled by the host's 1/S) over the samples of one segment
__global__ void __launch_bounds__(kVarBlock) k_var_sum(const VarSeg* __restrict__ segs) {
  const VarSeg& sg = segs[blockIdx.y];
  const int N = sg.N, n = sg.n;
  const int i = blockIdx.x * kVarBlock + threadIdx.x;
  if (i >= N) return;
  const size_t stride = (size_t)3 * N;
  const global_ptr<double> mean = as_global(sg.mean);
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  if (!sg.first) { m0 = mean[3 * i]; m1 = mean[3 * i + 1]; m2 = mean[3 * i + 2]; }
  {
    global_ptr<const double> x = as_global(sg.x) + 3 * i;
    for (int s = 0; s < n; ++s, x += stride) { m0 += x[0]; m1 += x[1]; m2 += x[2]; }
  }
  if (sg.last) {
    const double inv_n = 1.0 / sg.S;
    m0 *= inv_n; m1 *= inv_n; m2 *= inv_n;
  }
  mean[3 * i] = m0; mean[3 * i + 1] = m1; mean[3 * i + 2] = m2;
  if (sg.mode != 2) return;
  const global_ptr<double> nrm = as_global(sg.nrm);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  if (!sg.first) { a0 = nrm[3 * i]; a1 = nrm[3 * i + 1]; a2 = nrm[3 * i + 2]; }
  global_ptr<const double> ns = as_global(sg.nsm) + 3 * i;
  for (int s = 0; s < n; ++s, ns += stride) { a0 = a0 + ns[0]; a1 = a1 + ns[1]; a2 = a2 + ns[2]; }
  if (sg.last) { a0 *= sg.nscale; a1 *= sg.nscale; a2 *= sg.nscale; }
  nrm[3 * i] = a0; nrm[3 * i + 1] = a1; nrm[3 * i + 2] = a2;
}

// V4: k_variability's second loop over the samples of one segment: trace of the covariance (mode 0, :43) or the variance along the
// map's normal (modes 1 and 2, :69)
__global__ void __launch_bounds__(kVarBlock) k_var_centred(const VarSeg* __restrict__ segs) {
  const VarSeg& sg = segs[blockIdx.y];
  const int N = sg.N, n = sg.n;
  const int i = blockIdx.x * kVarBlock + threadIdx.x;
  if (i >= N) return;
  const size_t stride = (size_t)3 * N;
  const global_ptr<const double> mean = as_global((const double*)sg.mean);
  const double m0 = mean[3 * i], m1 = mean[3 * i + 1], m2 = mean[3 * i + 2];
  const double inv_n1 = 1.0 / (sg.S - 1);
  const global_ptr<double> acc = as_global(sg.acc);
  global_ptr<const double> x = as_global(sg.x) + 3 * i;
  if (sg.mode == 0) {
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    if (!sg.first) { c0 = acc[3 * i]; c1 = acc[3 * i + 1]; c2 = acc[3 * i + 2]; }
    for (int s = 0; s < n; ++s, x += stride) {
      const double v0 = x[0] - m0, v1 = x[1] - m1, v2 = x[2] - m2;
      c0 += v0 * v0; c1 += v1 * v1; c2 += v2 * v2;
    }
    if (sg.last) sg.out[i] = (c0 * inv_n1 + c1 * inv_n1) + c2 * inv_n1;
    else { acc[3 * i] = c0; acc[3 * i + 1] = c1; acc[3 * i + 2] = c2; }
  } else {
    const global_ptr<const double> nrm = as_global((const double*)sg.nrm);
    const double n0 = nrm[3 * i], n1 = nrm[3 * i + 1], n2 = nrm[3 * i + 2];
    double a = sg.first ? 0.0 : acc[i];
    for (int s = 0; s < n; ++s, x += stride) {
      const double p = (n0 * (x[0] - m0) + n1 * (x[1] - m1)) + n2 * (x[2] - m2);
      a += p * p;
    }
    if (sg.last) sg.out[i] = a * inv_n1;
    else acc[i] = a;
  }
}

// ---- the one-map path

__global__ void __launch_bounds__(kBlock) k_accumulate(int n, const double* __restrict__ src, double scale_after, double* __restrict__ acc) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double v = acc[i] + src[i];
  if (scale_after != 0.0) v *= scale_after;
  acc[i] = v;
}

// lane = vertex; the sample loop runs in the reference's order (mean = (Σ s)·(1/n), then the centred second moments)
__global__ void __launch_bounds__(kBlock) k_variability(int N, int S, const double* __restrict__ X, int mode,
                                                         const double* __restrict__ normals, double* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const size_t stride = (size_t)3 * N;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* x = X + (size_t)s * stride + 3 * i;
    m0 += x[0]; m1 += x[1]; m2 += x[2];
  }
  const double inv_n = 1.0 / S, inv_n1 = 1.0 / (S - 1);
  m0 *= inv_n; m1 *= inv_n; m2 *= inv_n;
  if (mode == 0) {
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    for (int s = 0; s < S; ++s) {
      const double* x = X + (size_t)s * stride + 3 * i;
      const double v0 = x[0] - m0, v1 = x[1] - m1, v2 = x[2] - m2;
      c0 += v0 * v0; c1 += v1 * v1; c2 += v2 * v2;
    }
    out[i] = (c0 * inv_n1 + c1 * inv_n1) + c2 * inv_n1;   // trace(cov) (:43)
  } else {
    const double n0 = normals[3 * i], n1 = normals[3 * i + 1], n2 = normals[3 * i + 2];
    double acc = 0.0;
    for (int s = 0; s < S; ++s) {
      const double* x = X + (size_t)s * stride + 3 * i;
      const double p = (n0 * (x[0] - m0) + n1 * (x[1] - m1)) + n2 * (x[2] - m2);
      acc += p * p;                                        // :69
    }
    out[i] = acc * inv_n1;
  }
}

}  // namespace

void launch_var_normals(hipStream_t st, int n_jobs, int Nmax, const VarNormalJob* jobs) {
  if (n_jobs <= 0) return;
  hipLaunchKernelGGL(k_var_normals, dim3(cdiv(Nmax, kVarBlock), n_jobs), dim3(kVarBlock), 0, st, jobs);
}
void launch_var_sum(hipStream_t st, int n_segs, int Nmax, const VarSeg* segs) {
  if (n_segs <= 0) return;
  hipLaunchKernelGGL(k_var_sum, dim3(cdiv(Nmax, kVarBlock), n_segs), dim3(kVarBlock), 0, st, segs);
}
void launch_var_centred(hipStream_t st, int n_segs, int Nmax, const VarSeg* segs) {
  if (n_segs <= 0) return;
  hipLaunchKernelGGL(k_var_centred, dim3(cdiv(Nmax, kVarBlock), n_segs), dim3(kVarBlock), 0, st, segs);
}

void launch_accumulate(hipStream_t st, int n, const double* src, double scale_after, double* acc) {
  hipLaunchKernelGGL(k_accumulate, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, st, n, src, scale_after, acc);
}
void launch_variability(hipStream_t st, int N, int S, const double* X, int mode, const double* normals, double* out) {
  hipLaunchKernelGGL(k_variability, dim3(cdiv(N, kBlock)), dim3(kBlock), 0, st, N, S, X, mode, normals, out);
}

}  // namespace icp
