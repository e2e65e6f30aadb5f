// kernels_scan_prep.hip — aligned and partial targets from raw scans (icp_scans_prepare_many).
//
// Per item: the similarity transform of its points and landmarks, the cuts (the cut_count vertices nearest a landmark, smallest in
// (d², id)), the flag bytes, and the compaction of what is left (maskPoints(...).transformedMesh).  Seven launches a round, `item` a
// grid dimension in every one; no floating-point atomics, no device-side waits.  The only atomics are integer additions to LDS
// histograms (k_scan_select): integer addition does not depend on order, so every result is a function of the item alone.
//
//   S1 k_scan_transform   thread = vertex | landmark | mask id: aligned, landmarks_out, the keys (bits of d²) per cut, bit 7 of the flags
//   S2 k_scan_select      workgroup = (cut, item): the exact threshold of the composite key (d² bits, id) by a radix select
//   S3 k_scan_flags       thread = vertex: the cuts' bits
//   S4 k_scan_triangles   thread = triangle: keep[], used[]
//   S5 k_scan_block       workgroup = tile of kScanTile elements of used[] or keep[]: exclusive prefix within the tile, tile total
//   S6 k_scan_totals      workgroup = (array, item): exclusive prefix of the tile totals, the counts
//   S7 k_scan_scatter     thread = vertex and triangle: partial points, renumbered triangles, kept ids (adds the tile's prefix)
#include "icp_kernels.hpp"

namespace icp {

namespace {

constexpr int kScanBlock = 256;      // threads of the per-element launches
constexpr int kScanSelBlock = 1024;  // threads of the selection's workgroup
constexpr int kScanPerThread = kScanTile / kScanBlock;  // consecutive elements a thread of the block scan owns
static_assert(kScanTile % kScanBlock == 0, "a tile is whole threads");

// A(x): q = s·x, u = q − c, y_i = ((R_i0·u_0 + R_i1·u_1) + R_i2·u_2) + o_i — every operation rounded separately (-ffp-contract=off).
// Vertices and landmarks go through this one function: a cut's centre has the bits the caller gets back
__device__ __forceinline__ void scan_apply(const ScanItem& it, const double* __restrict__ x, double y[3]) {
  const double u0 = it.s * x[0] - it.c[0], u1 = it.s * x[1] - it.c[1], u2 = it.s * x[2] - it.c[2];
  y[0] = ((it.R[0] * u0 + it.R[1] * u1) + it.R[2] * u2) + it.o[0];
  y[1] = ((it.R[3] * u0 + it.R[4] * u1) + it.R[5] * u2) + it.o[1];
  y[2] = ((it.R[6] * u0 + it.R[7] * u1) + it.R[8] * u2) + it.o[2];
}

// S1
__global__ void __launch_bounds__(kScanBlock) k_scan_transform(const ScanItem* __restrict__ items) {
  const ScanItem& it = items[blockIdx.y];
  const long long i = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  if (i < it.M) {
    double y[3];
    scan_apply(it, it.pts + 3 * i, y);
    it.aligned[3 * i] = y[0]; it.aligned[3 * i + 1] = y[1]; it.aligned[3 * i + 2] = y[2];
    for (int j = 0; j < it.n_cuts; ++j) {
      double z[3];
      scan_apply(it, it.lms + 3 * (size_t)it.cut_landmark[j], z);
      const double dx = y[0] - z[0], dy = y[1] - z[1], dz = y[2] - z[2];
      const double d2 = (dx * dx + dy * dy) + dz * dz;  // >= +0, finite or +inf: its bit pattern orders as the value does
      it.keys[(size_t)j * it.M + i] = (unsigned long long)__double_as_longlong(d2);
    }
  } else if (i < (long long)it.M + it.L) {
    const long long l = i - it.M;
    double y[3];
    scan_apply(it, it.lms + 3 * l, y);
    it.lm_out[3 * l] = y[0]; it.lm_out[3 * l + 1] = y[1]; it.lm_out[3 * l + 2] = y[2];
  } else if (i < (long long)it.M + it.L + it.n_mask) {
    // (the flags were zeroed in front of the round and nobody else writes them in this launch; a repeated id stores the same byte
    // twice: benign)
    const int id = it.mask[i - it.M - it.L];
    if (id < it.M) it.flags[id] = 0x80;
  }
}

// the histogram of one radix pass: a thread adds runs of equal digits at once (the leading bytes of the keys of one scan are nearly
// all equal: one LDS atomic per run instead of one per key)
struct DigitRun {
  int digit = -1;
  unsigned n = 0;
  __device__ __forceinline__ void add(unsigned* hist, int d) {
    if (d == digit) { ++n; return; }
    if (n) atomicAdd(&hist[digit], n);
    digit = d; n = 1;
  }
  __device__ __forceinline__ void flush(unsigned* hist) {
    if (n) atomicAdd(&hist[digit], n);
  }
};

// the bin of a 256-bin histogram that holds the want-th (1-based) smallest candidate -> s_pick = {bin, rank within the bin, the bin's
// count}; called by every thread of the workgroup, histogram complete
__device__ __forceinline__ void scan_pick_bin(const unsigned* hist, unsigned want, unsigned* s_pick) {
  const int d = threadIdx.x;
  if (d < 256) {
    unsigned below = 0;
    for (int i = 0; i < d; ++i) below += hist[i];
    const unsigned mine = hist[d];
    if (below < want && want <= below + mine) { s_pick[0] = (unsigned)d; s_pick[1] = want - below; s_pick[2] = mine; }
  }
}

// S2: the cut set of (item, cut) is {v : (key[v], v) <= (K*, id*)} lexicographically, |set| = cut_count.  Twelve passes of eight bits
// at most, most significant first: eight over the keys, then — only if the last key's equals do not all fit — four over the ids of
// the vertices whose key is K* (equal distances go to the lowest ids)
__global__ void __launch_bounds__(kScanSelBlock) k_scan_select(const ScanItem* __restrict__ items) {
  const ScanItem& it = items[blockIdx.y];
  const int j = blockIdx.x;
  if (j >= it.n_cuts) return;
  const int M = it.M, tid = threadIdx.x;
  const unsigned k = (unsigned)it.cut_count[j];
  unsigned long long* thr = it.thr + 2 * j;
  if (k == 0 || k >= (unsigned)M) {  // nobody, everybody
    if (tid == 0) {
      thr[0] = k == 0 ? 0ull : ~0ull;
      thr[1] = (unsigned long long)(k == 0 ? -1ll : (long long)0x7fffffff);
    }
    return;
  }
  __shared__ unsigned hist[256];
  __shared__ unsigned s_pick[3];
  const unsigned long long* __restrict__ keys = it.keys + (size_t)j * M;
  unsigned long long prefix = 0;
  unsigned want = k, cnt = 0;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    DigitRun run;
    for (int v = tid; v < M; v += kScanSelBlock) {
      const unsigned long long key = keys[v];
      if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) run.add(hist, (int)((key >> shift) & 255));
    }
    run.flush(hist);
    __syncthreads();
    scan_pick_bin(hist, want, s_pick);
    __syncthreads();
    prefix |= (unsigned long long)s_pick[0] << shift;
    want = s_pick[1]; cnt = s_pick[2];
    __syncthreads();
  }
  // prefix = K*; cnt vertices have it, the `want` lowest ids of them belong to the set
  unsigned id_prefix = 0x7fffffffu;
  if (want < cnt) {
    id_prefix = 0;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      DigitRun run;
      for (int v = tid; v < M; v += kScanSelBlock) {
        if (keys[v] != prefix) continue;
        const unsigned id = (unsigned)v;
        if (pass == 0 || (id >> (shift + 8)) == (id_prefix >> (shift + 8))) run.add(hist, (int)((id >> shift) & 255));
      }
      run.flush(hist);
      __syncthreads();
      scan_pick_bin(hist, want, s_pick);
      __syncthreads();
      id_prefix |= s_pick[0] << shift;
      want = s_pick[1];
      __syncthreads();
    }
  }
  if (tid == 0) {
    thr[0] = prefix;
    thr[1] = (unsigned long long)(long long)(int)id_prefix;
  }
}

// S3
__global__ void __launch_bounds__(kScanBlock) k_scan_flags(const ScanItem* __restrict__ items) {
  const ScanItem& it = items[blockIdx.y];
  const long long v = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  if (v >= it.M || it.n_cuts == 0) return;
  unsigned f = it.flags[v];  // bit 7, from S1
  for (int j = 0; j < it.n_cuts; ++j) {
    const unsigned long long key = it.keys[(size_t)j * it.M + v], K = it.thr[2 * j];
    const long long id = (long long)it.thr[2 * j + 1];
    if (key < K || (key == K && v <= id)) f |= 1u << j;
  }
  it.flags[v] = (unsigned char)f;
}

// S4: a triangle is kept iff none of its vertices is dropped; a vertex is used iff a kept triangle has it
__global__ void __launch_bounds__(kScanBlock) k_scan_triangles(const ScanItem* __restrict__ items) {
  const ScanItem& it = items[blockIdx.y];
  const long long t = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  if (t >= it.T) return;
  const int a = it.tris[3 * t], b = it.tris[3 * t + 1], c = it.tris[3 * t + 2];
  const bool keep = (it.flags[a] | it.flags[b] | it.flags[c]) == 0;
  it.keep[t] = keep ? 1 : 0;
  if (keep) {
    // (the triangles around a vertex all store the same byte, 1, into used[] — zeroed in front of the round —: the order of the
    // stores does not matter, and nothing reads used[] in this launch)
    it.used[a] = 1; it.used[b] = 1; it.used[c] = 1;
  }
}

// S5: blockIdx.z = 0: used[M]; 1: keep[T]
__global__ void __launch_bounds__(kScanBlock) k_scan_block(const ScanItem* __restrict__ items) {
  const ScanItem& it = items[blockIdx.y];
  const bool tri = blockIdx.z != 0;
  const int n = tri ? it.T : it.M;
  const long long base = (long long)blockIdx.x * kScanTile;
  if (base >= n) return;
  const unsigned char* __restrict__ src = tri ? it.keep : it.used;
  int* __restrict__ pre = tri ? it.tpre : it.vpre;
  __shared__ int s[kScanBlock];
  const long long e0 = base + (long long)threadIdx.x * kScanPerThread;
  int b[kScanPerThread], sum = 0;
#pragma unroll
  for (int e = 0; e < kScanPerThread; ++e) {
    b[e] = e0 + e < n ? (int)src[e0 + e] : 0;
    sum += b[e];
  }
  int total;
  int at = block_exclusive_scan<kScanBlock>(sum, s, &total);
#pragma unroll
  for (int e = 0; e < kScanPerThread; ++e) {
    if (e0 + e < n) pre[e0 + e] = at;
    at += b[e];
  }
  if (threadIdx.x == 0) (tri ? it.tblk : it.vblk)[blockIdx.x] = total;
}

// S6: blockIdx.x = 0: the vertices' tile totals; 1: the triangles'
__global__ void __launch_bounds__(kScanBlock) k_scan_totals(const ScanItem* __restrict__ items) {
  const ScanItem& it = items[blockIdx.y];
  const bool tri = blockIdx.x != 0;
  const int n = tri ? it.T : it.M;
  const int tiles = cdiv(n, kScanTile);
  int* __restrict__ blk = tri ? it.tblk : it.vblk;
  __shared__ int s[kScanBlock];
  int carry = 0;
  for (int c0 = 0; c0 < tiles; c0 += kScanBlock) {
    const int i = c0 + (int)threadIdx.x;
    const int value = i < tiles ? blk[i] : 0;
    int total;
    const int at = block_exclusive_scan<kScanBlock>(value, s, &total);
    if (i < tiles) blk[i] = carry + at;
    carry += total;
  }
  if (threadIdx.x == 0) it.counts[tri ? 1 : 0] = carry;
}

__device__ __forceinline__ int scan_new_vertex(const ScanItem& it, long long v) { return it.vpre[v] + it.vblk[v / kScanTile]; }

// S7
__global__ void __launch_bounds__(kScanBlock) k_scan_scatter(const ScanItem* __restrict__ items) {
  const ScanItem& it = items[blockIdx.y];
  const long long i = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  if (i < it.M && it.used[i]) {
    const size_t nv = (size_t)scan_new_vertex(it, i);
    it.ppts[3 * nv] = it.aligned[3 * i]; it.ppts[3 * nv + 1] = it.aligned[3 * i + 1]; it.ppts[3 * nv + 2] = it.aligned[3 * i + 2];
    it.kept[nv] = (int)i;
  }
  if (i < it.T && it.keep[i]) {
    const size_t nt = (size_t)(it.tpre[i] + it.tblk[i / kScanTile]);
    for (int e = 0; e < 3; ++e) it.ptris[3 * nt + e] = scan_new_vertex(it, it.tris[3 * i + e]);
  }
}

}  // namespace

void launch_scan_transform(hipStream_t st, int n_items, long long work_max, const ScanItem* items) {
  if (n_items <= 0 || work_max <= 0) return;
  hipLaunchKernelGGL(k_scan_transform, dim3((unsigned)((work_max + kScanBlock - 1) / kScanBlock), n_items), dim3(kScanBlock), 0, st, items);
}
void launch_scan_select(hipStream_t st, int n_items, const ScanItem* items) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(k_scan_select, dim3(kScanMaxCuts, n_items), dim3(kScanSelBlock), 0, st, items);
}
void launch_scan_flags(hipStream_t st, int n_items, int m_max, const ScanItem* items) {
  if (n_items <= 0 || m_max <= 0) return;
  hipLaunchKernelGGL(k_scan_flags, dim3(cdiv(m_max, kScanBlock), n_items), dim3(kScanBlock), 0, st, items);
}
void launch_scan_triangles(hipStream_t st, int n_items, int t_max, const ScanItem* items) {
  if (n_items <= 0 || t_max <= 0) return;
  hipLaunchKernelGGL(k_scan_triangles, dim3(cdiv(t_max, kScanBlock), n_items), dim3(kScanBlock), 0, st, items);
}
void launch_scan_prefix(hipStream_t st, int n_items, int n_max, const ScanItem* items) {
  if (n_items <= 0) return;
  if (n_max > 0) hipLaunchKernelGGL(k_scan_block, dim3(cdiv(n_max, kScanTile), n_items, 2), dim3(kScanBlock), 0, st, items);
  hipLaunchKernelGGL(k_scan_totals, dim3(2, n_items), dim3(kScanBlock), 0, st, items);
}
void launch_scan_scatter(hipStream_t st, int n_items, int n_max, const ScanItem* items) {
  if (n_items <= 0 || n_max <= 0) return;
  hipLaunchKernelGGL(k_scan_scatter, dim3(cdiv(n_max, kScanBlock), n_items), dim3(kScanBlock), 0, st, items);
}

}  // namespace icp
