// kernels_variability.hip — posterior variability maps of many chains side by side (icp_posterior_variability_many;
// apps/util/PosteriorVariability.scala:30-73 over LogHelper.logSamples2shapes).
//
// The samples of a call pass through one chunk buffer of fixed size, round by round.  Every launch of a round carries all its work
// (sample group, normal job or map segment = blockIdx.y) and reads its record from a device table made once per call:
//   V1 k_var_instance  the sample meshes of the round: up to kVarInstGroup samples of one model from ONE pass over its basis
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

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

constexpr int kVarInstBlock = 64;
constexpr int kVarInstU = 8;  // basis columns (× 3 rows) in flight per batch of loads
constexpr int kVarBlock = 128;

// V1.  Thread = model point, blockIdx.y = group.  The sums are instance_point's: the mean, then the basis columns in order with
// separately rounded multiply and add, then instance_pose — every sample's points are the bits of its own k_instance launch.  The
// basis is read once per group instead of once per sample (24·r bytes per point: 137 MB per sample at N = 28,561, r = 200).  The
// coefficients are wave-uniform loads from the samples' device vectors.  The basis pointer comes out of a record: global_ptr keeps
// its loads counted (icp_device.hpp).
__global__ void __launch_bounds__(kVarInstBlock) k_var_instance(const VarGroup* __restrict__ groups, const VarSample* __restrict__ samples) {
  constexpr int G = kVarInstGroup;
  const VarGroup& grp = groups[blockIdx.y];
  const int N = grp.N, r = grp.r, ng = grp.n;
  const int i = blockIdx.x * kVarInstBlock + threadIdx.x;
  if (i >= N) return;
  const VarSample* smp = samples + grp.first;
  global_ptr<const double> cf[G];
#pragma unroll
  for (int g = 0; g < G; ++g) cf[g] = as_global(smp[g < ng ? g : 0].coeffs);
  const global_ptr<const double> mean = as_global(grp.mean);
  double a0[G], a1[G], a2[G];
  const double m0 = mean[3 * i], m1 = mean[3 * i + 1], m2 = mean[3 * i + 2];
#pragma unroll
  for (int g = 0; g < G; ++g) { a0[g] = m0; a1[g] = m1; a2[g] = m2; }
  const global_ptr<const double> q = as_global(grp.Qp) + i;
  int j = 0;
  for (; j + kVarInstU <= r; j += kVarInstU) {
    double v[3 * kVarInstU];
#pragma unroll
    for (int u = 0; u < 3 * kVarInstU; ++u) v[u] = q[(size_t)(3 * j + u) * N];
    __builtin_amdgcn_sched_barrier(0);  // (all loads requested before the first multiply)
#pragma unroll
    for (int u = 0; u < kVarInstU; ++u)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const double c = cf[g][j + u];
        a0[g] = a0[g] + v[3 * u] * c;
        a1[g] = a1[g] + v[3 * u + 1] * c;
        a2[g] = a2[g] + v[3 * u + 2] * c;
      }
  }
  for (; j < r; ++j) {
    const double v0 = q[(size_t)(3 * j) * N], v1 = q[(size_t)(3 * j + 1) * N], v2 = q[(size_t)(3 * j + 2) * N];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const double c = cf[g][j];
      a0[g] = a0[g] + v0 * c;
      a1[g] = a1[g] + v1 * c;
      a2[g] = a2[g] + v2 * c;
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g >= ng) continue;
    const VarSample& s = smp[g];
    const d3 p = instance_pose(i, grp.ref, s.pose, a0[g], a1[g], a2[g]);  // ModelFittingParameters.scala:108-110
    const global_ptr<double> x = as_global(s.x);
    x[3 * i] = p.x; x[3 * i + 1] = p.y; x[3 * i + 2] = p.z;
  }
}

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

}  // namespace

void launch_var_instance(hipStream_t st, int n_groups, int Nmax, const VarGroup* groups, const VarSample* samples) {
  if (n_groups <= 0) return;
  ProfScope _ps(st, KID_INSTANCE);
  hipLaunchKernelGGL(k_var_instance, dim3(cdiv(Nmax, kVarInstBlock), n_groups), dim3(kVarInstBlock), 0, st, groups, samples);
}
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

}  // namespace icp
