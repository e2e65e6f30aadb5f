// kernels_samples.hip — uniform surface samples of many meshes (icp_surface_samples_many; Scalismo's UniformMeshSampler3D as
// IcpBasedSurfaceFitting.scala:51-53 and the two CreateGPModel.scala draw from it) and the mean trace of a kernel at given points
// (icp_kernel_total_variance_many; apps/femur/CreateGPModel.scala:38-46, approxTotalVariance).  DESIGN.md §5.19.
//
// `item` is a grid dimension in every launch; no floating-point atomics, no atomics at all, no device-side waits.  A triangle's weight
// is an INTEGER (its share of the largest triangle's area in units of 2^-32), so that the prefix sums are exact whatever the shape of
// the scan, and every result is a function of the item alone.
//
//   S1  k_smp_areas     workgroup = tile of kScanTile triangles: a2[t] = twice the area, the tile's largest
//   S2  k_smp_weights   workgroup = tile: Amax (every workgroup folds the same tile maxima), q[t], inclusive prefix within the tile, tile total
//   S3  k_smp_offsets   workgroup = item: exclusive prefix of the tile totals, Q, info
//   S4  k_smp_pick      thread = sample: x from the generator, its triangle by binary search, barycentric weights, the point
//   S5  k_smp_nearest   thread = sample: the exact (d², id) minimum over all vertices, the vertices tiled through LDS
//   V1  k_tv_trace      workgroup = 256 consecutive points: the trace of k(x, x), a fixed tree
//   V2  k_tv_finish     one thread per item: the block sums in block order, divided by n
#include "icp_kernels.hpp"
#include "icp_gp_terms.hpp"

#include <climits>

namespace icp {

namespace {

constexpr int kSmpPerThread = kScanTile / kSmpBlock;  // triangles a thread owns in S1 (strided) and S2 (consecutive)
static_assert(kScanTile % kSmpBlock == 0, "a tile is whole threads");
typedef unsigned long long u64;

// orc_rng_uniform's 53-bit integer (oracle/icp_oracle.c; k_met_samples of kernels_metrics.hip): splitmix64 over (seed, step, lane) >> 11
__device__ __forceinline__ u64 smp_splitmix64(u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ u64 smp_h(u64 seed, u64 step, u64 lane) {
  return smp_splitmix64(smp_splitmix64(smp_splitmix64(seed) ^ (step * 0xD1342543DE82EF95ull)) ^ (lane * 0x2545F4914F6CDD1Dull)) >> 11;
}
__device__ __forceinline__ double smp_u(u64 h) { return ((double)h + 0.5) * (1.0 / 9007199254740992.0); }

// the largest of kSmpBlock threads' values, in every thread (a maximum is exact in any order); s: kSmpBlock / 64 doubles
__device__ __forceinline__ double smp_block_max(double x, double* s) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x = fmax(x, __shfl_xor(x, d, 64));
  __syncthreads();  // (s may still be read from an earlier reduction)
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = x;
  __syncthreads();
  double m = s[0];
#pragma unroll
  for (int w = 1; w < kSmpBlock / 64; ++w) m = fmax(m, s[w]);
  return m;
}
// the item's largest a2: every workgroup folds the same tile maxima
__device__ __forceinline__ double smp_amax(const SmpItem& it, double* s) {
  double m = 0.0;
  for (int i = threadIdx.x; i < it.tiles; i += kSmpBlock) m = fmax(m, it.tmax[i]);
  return smp_block_max(m, s);
}

// S1
__global__ void __launch_bounds__(kSmpBlock) k_smp_areas(const SmpItem* __restrict__ items) {
  __shared__ double s[kSmpBlock / 64];
  const SmpItem& it = items[blockIdx.y];
  if ((int)blockIdx.x >= it.tiles) return;  // (uniform)
  const long long base = (long long)blockIdx.x * kScanTile;
  double m = 0.0;
#pragma unroll
  for (int e = 0; e < kSmpPerThread; ++e) {
    const long long t = base + e * kSmpBlock + threadIdx.x;
    if (t >= it.T) continue;
    const int ia = it.tris[3 * t], ib = it.tris[3 * t + 1], ic = it.tris[3 * t + 2];
    const double ax = it.pts[3 * (size_t)ia], ay = it.pts[3 * (size_t)ia + 1], az = it.pts[3 * (size_t)ia + 2];
    const double e1x = it.pts[3 * (size_t)ib] - ax, e1y = it.pts[3 * (size_t)ib + 1] - ay, e1z = it.pts[3 * (size_t)ib + 2] - az;
    const double e2x = it.pts[3 * (size_t)ic] - ax, e2y = it.pts[3 * (size_t)ic + 1] - ay, e2z = it.pts[3 * (size_t)ic + 2] - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    double a2 = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(a2 <= 1.7976931348623157e308)) a2 = 0.0;  // (not finite: within the limits of the entry point this cannot happen)
    it.a2[t] = a2;
    m = fmax(m, a2);
  }
  m = smp_block_max(m, s);
  if (threadIdx.x == 0) it.tmax[blockIdx.x] = m;
}

// S2.  Thread t owns the triangles base + t·kSmpPerThread + e: consecutive, so that its prefix is a running sum
__global__ void __launch_bounds__(kSmpBlock) k_smp_weights(const SmpItem* __restrict__ items) {
  __shared__ double sm[kSmpBlock / 64];
  __shared__ u64 s[kSmpBlock];
  const SmpItem& it = items[blockIdx.y];
  if ((int)blockIdx.x >= it.tiles) return;  // (uniform)
  const double amax = smp_amax(it, sm);
  const long long e0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kSmpPerThread;
  u64 q[kSmpPerThread], sum = 0;
  int positive = 0;
#pragma unroll
  for (int e = 0; e < kSmpPerThread; ++e) {
    q[e] = 0;
    if (e0 + e < it.T && amax > 0.0) q[e] = (u64)trunc((it.a2[e0 + e] / amax) * 4294967296.0);
    sum += q[e];
    positive += q[e] > 0;
  }
  u64 total;
  u64 at = block_exclusive_scan<kSmpBlock, u64>(sum, s, &total);
#pragma unroll
  for (int e = 0; e < kSmpPerThread; ++e) {
    at += q[e];
    if (e0 + e < it.T) it.C[e0 + e] = at;
  }
  // the tile's count of positive weights through the same LDS array
  u64 cnt_total;
  (void)block_exclusive_scan<kSmpBlock, u64>((u64)positive, s, &cnt_total);
  if (threadIdx.x == 0) {
    it.tblk[blockIdx.x] = total;
    it.tcnt[blockIdx.x] = (int)cnt_total;
  }
}

// S3
__global__ void __launch_bounds__(kSmpBlock) k_smp_offsets(const SmpItem* __restrict__ items) {
  __shared__ double sm[kSmpBlock / 64];
  __shared__ u64 s[kSmpBlock];
  const SmpItem& it = items[blockIdx.x];
  const double amax = smp_amax(it, sm);
  u64 carry = 0, count = 0;
  for (int c0 = 0; c0 < it.tiles; c0 += kSmpBlock) {
    const int i = c0 + (int)threadIdx.x;
    const u64 value = i < it.tiles ? it.tblk[i] : 0;
    u64 total, cnt;
    const u64 at = block_exclusive_scan<kSmpBlock, u64>(value, s, &total);
    (void)block_exclusive_scan<kSmpBlock, u64>(i < it.tiles ? (u64)it.tcnt[i] : 0, s, &cnt);
    if (i < it.tiles) it.tblk[i] = carry + at;
    carry += total;
    count += cnt;
  }
  if (threadIdx.x != 0) return;
  it.Q[0] = carry;
  const bool ok = carry > 0;
  const double half = 0.5 * amax;
  it.info[0] = ok ? (double)count : 0.0;
  it.info[1] = ok ? half : 0.0;
  it.info[2] = ok ? half * ((double)carry * (1.0 / 4294967296.0)) : 0.0;
  it.info[3] = 0.0;
}

// S4.  x = (h·Q) >> 53 < Q; the triangle is the first t whose prefix C_t exceeds x, so a zero weight is never chosen
__global__ void __launch_bounds__(kSmpBlock) k_smp_pick(const SmpItem* __restrict__ items) {
  const SmpItem& it = items[blockIdx.y];
  const long long k = (long long)blockIdx.x * kSmpBlock + threadIdx.x;
  if (k >= it.n) return;
  const u64 Q = it.Q[0];
  if (Q == 0) {
    const double nan = __builtin_nan("");
    for (int c = 0; c < 3; ++c) { it.opts[3 * k + c] = nan; it.obary[3 * k + c] = nan; }
    it.ocells[k] = -1;
    it.oids[k] = -1;
    return;
  }
  const u64 x = __umul64hi(smp_h(it.seed, 0, (u64)k) << 11, Q);
  int lo = 0, hi = it.T - 1;  // C_{T-1} = Q > x: the answer lies in [lo, hi]
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (it.C[mid] + it.tblk[mid / kScanTile] > x) hi = mid;
    else lo = mid + 1;
  }
  const int t = lo;
  const double r = sqrt(smp_u(smp_h(it.seed, 1, (u64)k))), v = smp_u(smp_h(it.seed, 2, (u64)k));
  const double w0 = 1.0 - r, w1 = r * (1.0 - v), w2 = r * v;
  const int ia = it.tris[3 * (size_t)t], ib = it.tris[3 * (size_t)t + 1], ic = it.tris[3 * (size_t)t + 2];
  for (int c = 0; c < 3; ++c)
    it.opts[3 * k + c] = (w0 * it.pts[3 * (size_t)ia + c] + w1 * it.pts[3 * (size_t)ib + c]) + w2 * it.pts[3 * (size_t)ic + c];
  it.obary[3 * k] = w0; it.obary[3 * k + 1] = w1; it.obary[3 * k + 2] = w2;
  it.ocells[k] = t;
}

// S5.  Ascending ids and a strict comparison: equal distances go to the lowest id
__global__ void __launch_bounds__(kSmpBlock) k_smp_nearest(const SmpItem* __restrict__ items) {
  __shared__ double sv[3 * kSmpVertexTile];
  const SmpItem& it = items[blockIdx.y];
  if (!it.want_ids || (long long)blockIdx.x * kSmpBlock >= it.n || it.Q[0] == 0) return;  // (uniform)
  const int tid = threadIdx.x;
  const long long k = (long long)blockIdx.x * kSmpBlock + tid;
  const bool ok = k < it.n;
  const long long kc = ok ? k : it.n - 1;
  const double x0 = it.opts[3 * kc], x1 = it.opts[3 * kc + 1], x2 = it.opts[3 * kc + 2];
  double best = INFINITY;
  int best_id = -1;
  for (int v0 = 0; v0 < it.M; v0 += kSmpVertexTile) {
    const int cnt = min(kSmpVertexTile, it.M - v0);
    __syncthreads();  // (the tile may still be read)
    for (int i = tid; i < 3 * cnt; i += kSmpBlock) sv[i] = it.pts[(size_t)3 * v0 + i];
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      const double dx = x0 - sv[3 * i], dy = x1 - sv[3 * i + 1], dz = x2 - sv[3 * i + 2];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 < best) { best = d2; best_id = v0 + i; }
    }
  }
  if (ok) it.oids[k] = best_id;
}

// the diagonal entry [c][c] of the header's term expression at y = x, point i, the terms summed in order
__device__ __forceinline__ double tv_diagonal(const TvItem& it, int i, double x0, double x1, double x2, int c) {
  double acc = 0.0;
  for (int t = 0; t < it.n_terms; ++t) {
    const GpmTerm& tm = it.terms[t];
    double ww = 1.0;
    if (tm.w) ww = tm.w[i] * tm.w[i];
    double val = gpm_base(tm, x0, x1, x2, x0, x1, x2);
    if (tm.gain > 0.0) {
      const double sgn = c == tm.axis ? -1.0 : 1.0;
      const double bm = gpm_base(tm, x0, x1, x2, tm.axis == 0 ? -x0 : x0, tm.axis == 1 ? -x1 : x1, tm.axis == 2 ? -x2 : x2);
      val = val + (tm.gain * sgn) * bm;
    }
    acc = acc + ((tm.scale * ww) * val) * tm.A[3 * c + c];
  }
  return acc;
}

// V1
__global__ void __launch_bounds__(kTvBlock) k_tv_trace(const TvItem* __restrict__ items) {
  __shared__ double tr[kTvBlock];
  const TvItem& it = items[blockIdx.y];
  if ((int)blockIdx.x >= it.nblk) return;  // (uniform)
  const int t = threadIdx.x, i = blockIdx.x * kTvBlock + t;
  double v = 0.0;
  if (i < it.n) {
    const double x0 = it.pts[3 * (size_t)i], x1 = it.pts[3 * (size_t)i + 1], x2 = it.pts[3 * (size_t)i + 2];
    v = (tv_diagonal(it, i, x0, x1, x2, 0) + tv_diagonal(it, i, x0, x1, x2, 1)) + tv_diagonal(it, i, x0, x1, x2, 2);
  }
  tr[t] = v;
  __syncthreads();
  for (int s = kTvBlock / 2; s > 0; s >>= 1) {
    if (t < s) tr[t] = tr[t] + tr[t + s];
    __syncthreads();
  }
  if (t == 0) it.bsum[blockIdx.x] = tr[0];
}

// V2
__global__ void __launch_bounds__(64) k_tv_finish(const TvItem* __restrict__ items, int n_items) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n_items) return;
  const TvItem& it = items[b];
  double sum = 0.0;
  for (int i = 0; i < it.nblk; ++i) sum = sum + it.bsum[i];
  it.out[0] = sum / (double)it.n;
}

}  // namespace

void launch_smp_weights(hipStream_t st, int n_items, int t_max, const SmpItem* items) {
  if (n_items <= 0 || t_max <= 0) return;
  const dim3 per_tile(cdiv(t_max, kScanTile), n_items);
  hipLaunchKernelGGL(k_smp_areas, per_tile, dim3(kSmpBlock), 0, st, items);
  hipLaunchKernelGGL(k_smp_weights, per_tile, dim3(kSmpBlock), 0, st, items);
  hipLaunchKernelGGL(k_smp_offsets, dim3(n_items), dim3(kSmpBlock), 0, st, items);
}
void launch_smp_pick(hipStream_t st, int n_items, int n_max, const SmpItem* items) {
  if (n_items <= 0 || n_max <= 0) return;
  hipLaunchKernelGGL(k_smp_pick, dim3(cdiv(n_max, kSmpBlock), n_items), dim3(kSmpBlock), 0, st, items);
}
void launch_smp_nearest(hipStream_t st, int n_items, int n_max, const SmpItem* items) {
  if (n_items <= 0 || n_max <= 0) return;
  hipLaunchKernelGGL(k_smp_nearest, dim3(cdiv(n_max, kSmpBlock), n_items), dim3(kSmpBlock), 0, st, items);
}
void launch_tv(hipStream_t st, int n_items, int n_max, const TvItem* items) {
  if (n_items <= 0 || n_max <= 0) return;
  hipLaunchKernelGGL(k_tv_trace, dim3(cdiv(n_max, kTvBlock), n_items), dim3(kTvBlock), 0, st, items);
  hipLaunchKernelGGL(k_tv_finish, dim3(cdiv(n_items, 64)), dim3(64), 0, st, items, n_items);
}

}  // namespace icp
