// kernels_decimate.hip — mesh decimation to a vertex subset (icp_decimate_many).
//
// Per item: farthest-point samples (Euclidean, f64), the sample nearest every vertex along mesh edges (synchronous min-plus sweeps on
// 64-bit keys: f32 distance bits, label), and the dual triangles of those cells without duplicates.  `item` is a grid dimension in
// every launch; no floating-point atomics, no device-side waits.  The atomics are integer minima and one integer count: neither
// depends on order, so every result is a function of the item alone.
//
//   D1  k_dec_select_step    blockIdx = (block of vertices, item), one launch per sample: folds the last launch's partials, updates D
//   D1' k_dec_select_group   workgroup = item (M <= kDecGroupVertices): all the steps in one launch, coordinates and D in registers
//   D2  k_dec_clear/_seed    thread = vertex | sample: both key buffers all ones, then the samples' keys (0, j)
//   D3  k_dec_sweep          thread = half-edge, one launch per sweep: next = min(cur, cur[u] + len), integer atomicMin
//   D4  k_dec_candidates     thread = vertex and triangle: labels, the canonical triple key of a candidate, the candidates' count
//   D5  k_dec_insert         thread = triangle: its key into the open-addressing table, the lowest index per key
//   D6  k_dec_keep           thread = triangle: keep[t] = the lowest index of my key is t
//   D7  k_dec_block          workgroup = tile of kScanTile triangles: exclusive prefix of keep[] within the tile, tile total
//   D8  k_dec_totals         workgroup = item: exclusive prefix of the tile totals, T_out
//   D9  k_dec_scatter        thread = triangle: the kept triples, in the order of their original index
#include "icp_kernels.hpp"

#include <climits>

namespace icp {

namespace {

constexpr unsigned long long kDecNone = ~0ull;
constexpr int kDecPerThread = kScanTile / kDecBlock;  // consecutive triangles a thread of the block scan owns
static_assert(kScanTile % kDecBlock == 0, "a tile is whole threads");

struct DecBest {
  double v;
  int i;
};
// the larger value; equal values go to the lowest id
__device__ __forceinline__ void dec_fold(DecBest& x, double v, int i) {
  if (v > x.v || (v == x.v && i < x.i)) x = DecBest{v, i};
}
// d²(u, v) = ((dx·dx + dy·dy) + dz·dz), every operation rounded separately (-ffp-contract=off)
__device__ __forceinline__ double dec_d2(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// the best of kDecBlock threads, in every thread
__device__ __forceinline__ DecBest dec_block_reduce(DecBest x, double* sv, int* si) {
  const int t = threadIdx.x;
  sv[t] = x.v; si[t] = x.i;
  __syncthreads();
  for (int d = kDecBlock / 2; d > 0; d >>= 1) {
    if (t < d) {
      DecBest a{sv[t], si[t]};
      dec_fold(a, sv[t + d], si[t + d]);
      sv[t] = a.v; si[t] = a.i;
    }
    __syncthreads();
  }
  const DecBest b{sv[0], si[0]};
  __syncthreads();
  return b;
}

// D1.  `step` = j in 0 .. kk: launch j names sample j (j < kk) and the covering radius after j samples (j >= 1).  Reads the partials'
// half j & 1, writes the other one.  Every workgroup folds the same partials, so all agree on the sample without a device-side wait.
__global__ void __launch_bounds__(kDecBlock) k_dec_select_step(const DecItem* __restrict__ items, int step) {
  __shared__ double sv[kDecBlock];
  __shared__ int si[kDecBlock];
  const DecItem& it = items[blockIdx.y];
  if (it.group || (int)blockIdx.x >= it.nblk || step > it.kk) return;
  const int t = threadIdx.x, nblk = it.nblk;
  const int prev = (step & 1) * nblk, cur = ((step + 1) & 1) * nblk;
  const bool lead = blockIdx.x == 0 && t == 0;
  int p = it.start;
  if (step == 0) {
    if (lead) { it.counts[0] = it.kk; it.counts[1] = 0; it.counts[2] = 0; it.counts[3] = 0; }
  } else {
    DecBest x{-1.0, INT_MAX};
    for (int b = t; b < nblk; b += kDecBlock) dec_fold(x, it.pmax[prev + b], it.pidx[prev + b]);
    const DecBest best = dec_block_reduce(x, sv, si);
    // (counts[0] is kk until the selection stops at some step s < kk, and s from then on: nothing is written behind the stop)
    if (lead && it.counts[0] >= step) {
      it.cover2[step - 1] = best.v;
      if (step < it.kk && best.v == 0.0) it.counts[0] = step;
    }
    if (step == it.kk) return;
    if (best.v == 0.0) {  // every vertex coincides with a sample: the partial is handed on unchanged, every later launch decides the same
      if (t == 0) { it.pmax[cur + blockIdx.x] = it.pmax[prev + blockIdx.x]; it.pidx[cur + blockIdx.x] = it.pidx[prev + blockIdx.x]; }
      return;
    }
    p = best.i;
  }
  const double px = it.pts[3 * (size_t)p], py = it.pts[3 * (size_t)p + 1], pz = it.pts[3 * (size_t)p + 2];
  if (lead) {
    it.ids[step] = p;
    it.spts[3 * step] = px; it.spts[3 * step + 1] = py; it.spts[3 * step + 2] = pz;
  }
  const int v = blockIdx.x * kDecBlock + t;
  DecBest x{-1.0, INT_MAX};
  if (v < it.M) {
    double d = dec_d2(it.pts[3 * (size_t)v], it.pts[3 * (size_t)v + 1], it.pts[3 * (size_t)v + 2], px, py, pz);
    if (step > 0) {
      const double old = it.D[v];
      d = d < old ? d : old;
    }
    it.D[v] = d;
    x = DecBest{d, v};
  }
  const DecBest b = dec_block_reduce(x, sv, si);
  if (t == 0) { it.pmax[cur + blockIdx.x] = b.v; it.pidx[cur + blockIdx.x] = b.i; }
}

// D1'.  Thread t owns the vertices t + kDecGroupThreads·e; the argmax goes through the waves' shuffles and one LDS row per wave.  The
// same expressions and the same tie rule as D1: the same bits.
__global__ void __launch_bounds__(kDecGroupThreads) k_dec_select_group(const DecItem* __restrict__ items) {
  constexpr int kWaves = kDecGroupThreads / 64;
  __shared__ double sv[kWaves];
  __shared__ int si[kWaves];
  const DecItem& it = items[blockIdx.x];
  if (!it.group) return;
  const int t = threadIdx.x, M = it.M, kk = it.kk;
  double x[kDecGroupPerThread], y[kDecGroupPerThread], z[kDecGroupPerThread], D[kDecGroupPerThread];
#pragma unroll
  for (int e = 0; e < kDecGroupPerThread; ++e) {
    const int v = t + kDecGroupThreads * e;
    const bool ok = v < M;
    x[e] = ok ? it.pts[3 * (size_t)v] : 0.0;
    y[e] = ok ? it.pts[3 * (size_t)v + 1] : 0.0;
    z[e] = ok ? it.pts[3 * (size_t)v + 2] : 0.0;
    D[e] = -1.0;  // (a vertex past M keeps it: below every real D)
  }
  if (t == 0) { it.counts[1] = 0; it.counts[2] = 0; it.counts[3] = 0; }
  int p = it.start, k_eff = kk;
  for (int step = 0; step <= kk; ++step) {
    if (step > 0) {
      DecBest b{-1.0, INT_MAX};
#pragma unroll
      for (int e = 0; e < kDecGroupPerThread; ++e) dec_fold(b, D[e], t + kDecGroupThreads * e);
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const double ov = __shfl_xor(b.v, d, 64);
        const int oi = __shfl_xor(b.i, d, 64);
        dec_fold(b, ov, oi);
      }
      if ((t & 63) == 0) { sv[t >> 6] = b.v; si[t >> 6] = b.i; }
      __syncthreads();
      b = DecBest{-1.0, INT_MAX};
#pragma unroll
      for (int w = 0; w < kWaves; ++w) dec_fold(b, sv[w], si[w]);
      __syncthreads();
      if (t == 0) it.cover2[step - 1] = b.v;
      if (step == kk) break;
      if (b.v == 0.0) { k_eff = step; break; }
      p = b.i;
    }
    const double px = it.pts[3 * (size_t)p], py = it.pts[3 * (size_t)p + 1], pz = it.pts[3 * (size_t)p + 2];
    if (t == 0) {
      it.ids[step] = p;
      it.spts[3 * step] = px; it.spts[3 * step + 1] = py; it.spts[3 * step + 2] = pz;
    }
#pragma unroll
    for (int e = 0; e < kDecGroupPerThread; ++e) {
      if (t + kDecGroupThreads * e < M) {
        const double d = dec_d2(x[e], y[e], z[e], px, py, pz);
        D[e] = (step == 0 || d < D[e]) ? d : D[e];
      }
    }
  }
  if (t == 0) it.counts[0] = k_eff;
}

// D2
__global__ void __launch_bounds__(kDecBlock) k_dec_clear(const DecItem* __restrict__ items) {
  const DecItem& it = items[blockIdx.y];
  const long long v = (long long)blockIdx.x * kDecBlock + threadIdx.x;
  if (v >= it.M) return;
  it.key[0][v] = kDecNone;
  it.key[1][v] = kDecNone;
}
__global__ void __launch_bounds__(kDecBlock) k_dec_seed(const DecItem* __restrict__ items) {
  const DecItem& it = items[blockIdx.y];
  const int j = blockIdx.x * kDecBlock + threadIdx.x;
  if (j >= it.counts[0]) return;  // k_eff, from the selection
  const int v = it.ids[j];        // (the samples are distinct vertices: one store per key)
  it.key[0][v] = (unsigned long long)j;
  it.key[1][v] = (unsigned long long)j;
}

// D3.  Half-edge e of triangle (a, b, c): a→b, b→a, b→c, c→b, c→a, a→c.  The thread also lowers next[u] to cur[u]: next held the keys
// of the sweep before, which are nowhere below cur's, so that next ends as min(cur, candidates) whatever the order.  A vertex without
// an edge never changes in either buffer.
__global__ void __launch_bounds__(kDecBlock) k_dec_sweep(const DecItem* __restrict__ items, int slot, int parity) {
  const DecItem& it = items[blockIdx.y];
  const long long i = (long long)blockIdx.x * kDecBlock + threadIdx.x;
  if (i >= 6ll * it.T) return;
  const long long tr = i / 6;
  const int e = (int)(i - 6 * tr);
  const int from = (e + 1) / 2 % 3, to = e == 0 ? 1 : e == 1 ? 0 : e == 2 ? 2 : e == 3 ? 1 : e == 4 ? 0 : 2;
  const int u = it.tris[3 * tr + from], v = it.tris[3 * tr + to];
  const unsigned long long* __restrict__ cur = it.key[parity];
  unsigned long long* next = it.key[parity ^ 1];
  const unsigned long long ku = cur[u];
  atomicMin(&next[u], ku);
  if (u == v || ku == kDecNone) return;
  const double d2 = dec_d2(it.pts[3 * (size_t)u], it.pts[3 * (size_t)u + 1], it.pts[3 * (size_t)u + 2], it.pts[3 * (size_t)v],
                           it.pts[3 * (size_t)v + 1], it.pts[3 * (size_t)v + 2]);
  const float len = (float)sqrt(d2);  // the f64 square root, then one rounding to f32
  const float dist = __uint_as_float((unsigned)(ku >> 32)) + len;
  const unsigned long long cand = ((unsigned long long)__float_as_uint(dist) << 32) | (ku & 0xffffffffull);
  if (cand < cur[v]) {  // (otherwise next[v] <= cur[v] <= cand already)
    atomicMin(&next[v], cand);
    it.flags[slot] = 1;
  }
}

// D4.  `parity`: the buffer that holds the final keys
__global__ void __launch_bounds__(kDecBlock) k_dec_candidates(const DecItem* __restrict__ items, int parity) {
  const DecItem& it = items[blockIdx.y];
  const long long i = (long long)blockIdx.x * kDecBlock + threadIdx.x;
  const unsigned long long* __restrict__ key = it.key[parity];
  if (i < it.M) it.labels[i] = key[i] == kDecNone ? -1 : (int)(unsigned)key[i];
  if (i >= it.T) return;
  const unsigned long long ka = key[it.tris[3 * i]], kb = key[it.tris[3 * i + 1]], kc = key[it.tris[3 * i + 2]];
  unsigned long long out = kDecNone;
  const unsigned a = (unsigned)ka, b = (unsigned)kb, c = (unsigned)kc;
  if (ka != kDecNone && kb != kDecNone && kc != kDecNone && a != b && b != c && a != c) {
    // the rotation that puts the smallest label first; the orientation is kept
    unsigned p = a, q = b, r = c;
    if (b < a && b < c) { p = b; q = c; r = a; }
    else if (c < a && c < b) { p = c; q = a; r = b; }
    out = ((unsigned long long)p << 32) | ((unsigned long long)q << 16) | r;
    atomicAdd(&it.counts[3], 1);
  }
  it.tkey[i] = out;
}

__device__ __forceinline__ unsigned dec_hash(unsigned long long key) { return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32); }

// D5.  At most half the slots are ever taken (size >= 2·candidates), so a probe ends at the key or at an empty slot; the walk is
// bounded by the table's size all the same.  Which slot a key takes depends on the order; nothing that leaves the table does.
__global__ void __launch_bounds__(kDecBlock) k_dec_insert(const DecItem* __restrict__ items, const DecTable* __restrict__ tables) {
  const DecItem& it = items[blockIdx.y];
  const DecTable& tb = tables[blockIdx.y];
  const long long t = (long long)blockIdx.x * kDecBlock + threadIdx.x;
  if (t >= it.T) return;
  const unsigned long long key = it.tkey[t];
  if (key == kDecNone) return;
  unsigned h = dec_hash(key) & tb.mask;
  for (unsigned n = 0; n <= tb.mask; ++n, h = (h + 1) & tb.mask) {
    const unsigned long long old = atomicCAS(&tb.slots[h], kDecNone, key);
    if (old == kDecNone || old == key) {
      atomicMin(&tb.lowest[h], (unsigned)t);
      return;
    }
  }
}

// D6
__global__ void __launch_bounds__(kDecBlock) k_dec_keep(const DecItem* __restrict__ items, const DecTable* __restrict__ tables) {
  const DecItem& it = items[blockIdx.y];
  const DecTable& tb = tables[blockIdx.y];
  const long long t = (long long)blockIdx.x * kDecBlock + threadIdx.x;
  if (t >= it.T) return;
  const unsigned long long key = it.tkey[t];
  unsigned char keep = 0;
  if (key != kDecNone) {
    unsigned h = dec_hash(key) & tb.mask;
    for (unsigned n = 0; n <= tb.mask; ++n, h = (h + 1) & tb.mask) {
      const unsigned long long s = tb.slots[h];
      if (s == key) { keep = tb.lowest[h] == (unsigned)t; break; }
      if (s == kDecNone) break;
    }
  }
  it.keep[t] = keep;
}

// D7 (the block scan of kernels_scan_prep.hip S5, over keep[T])
__global__ void __launch_bounds__(kDecBlock) k_dec_block(const DecItem* __restrict__ items) {
  const DecItem& it = items[blockIdx.y];
  const int n = it.T;
  const long long base = (long long)blockIdx.x * kScanTile;
  if (base >= n) return;
  __shared__ int s[kDecBlock];
  const long long e0 = base + (long long)threadIdx.x * kDecPerThread;
  int b[kDecPerThread], sum = 0;
#pragma unroll
  for (int e = 0; e < kDecPerThread; ++e) {
    b[e] = e0 + e < n ? (int)it.keep[e0 + e] : 0;
    sum += b[e];
  }
  int total;
  int at = block_exclusive_scan<kDecBlock>(sum, s, &total);
#pragma unroll
  for (int e = 0; e < kDecPerThread; ++e) {
    if (e0 + e < n) it.tpre[e0 + e] = at;
    at += b[e];
  }
  if (threadIdx.x == 0) it.tblk[blockIdx.x] = total;
}

// D8
__global__ void __launch_bounds__(kDecBlock) k_dec_totals(const DecItem* __restrict__ items, const DecTable* __restrict__ tables) {
  const DecItem& it = items[blockIdx.x];
  const int tiles = cdiv(it.T, kScanTile);
  __shared__ int s[kDecBlock];
  int carry = 0;
  for (int c0 = 0; c0 < tiles; c0 += kDecBlock) {
    const int i = c0 + (int)threadIdx.x;
    const int value = i < tiles ? it.tblk[i] : 0;
    int total;
    const int at = block_exclusive_scan<kDecBlock>(value, s, &total);
    if (i < tiles) it.tblk[i] = carry + at;
    carry += total;
  }
  if (threadIdx.x == 0) tables[blockIdx.x].t_out[0] = carry;
}

// D9
__global__ void __launch_bounds__(kDecBlock) k_dec_scatter(const DecItem* __restrict__ items, const DecTable* __restrict__ tables) {
  const DecItem& it = items[blockIdx.y];
  const long long t = (long long)blockIdx.x * kDecBlock + threadIdx.x;
  if (t >= it.T || !it.keep[t]) return;
  const size_t row = (size_t)(it.tpre[t] + it.tblk[t / kScanTile]);  // < candidates: a kept triangle is a candidate
  const unsigned long long key = it.tkey[t];
  if (row >= (size_t)tables[blockIdx.y].cap) return;  // (cannot happen: the host sized `cells` from the candidates' count)
  int* __restrict__ out = tables[blockIdx.y].cells + 3 * row;
  out[0] = (int)(key >> 32); out[1] = (int)((key >> 16) & 0xffff); out[2] = (int)(key & 0xffff);
}

}  // namespace

void launch_dec_select(hipStream_t st, int n_items, int nblk_max, int kk_max, bool any_group, const DecItem* items) {
  if (n_items <= 0) return;
  if (any_group) hipLaunchKernelGGL(k_dec_select_group, dim3(n_items), dim3(kDecGroupThreads), 0, st, items);
  if (nblk_max <= 0) return;
  for (int step = 0; step <= kk_max; ++step)
    hipLaunchKernelGGL(k_dec_select_step, dim3(nblk_max, n_items), dim3(kDecBlock), 0, st, items, step);
}
void launch_dec_seed(hipStream_t st, int n_items, int m_max, int kk_max, const DecItem* items) {
  if (n_items <= 0 || m_max <= 0) return;
  hipLaunchKernelGGL(k_dec_clear, dim3(cdiv(m_max, kDecBlock), n_items), dim3(kDecBlock), 0, st, items);
  hipLaunchKernelGGL(k_dec_seed, dim3(cdiv(kk_max, kDecBlock), n_items), dim3(kDecBlock), 0, st, items);
}
void launch_dec_sweep(hipStream_t st, int n_items, int t_max, int slot, int parity, const DecItem* items) {
  if (n_items <= 0 || t_max <= 0) return;
  const long long blocks = (6ll * t_max + kDecBlock - 1) / kDecBlock;
  hipLaunchKernelGGL(k_dec_sweep, dim3((unsigned)blocks, n_items), dim3(kDecBlock), 0, st, items, slot, parity);
}
void launch_dec_candidates(hipStream_t st, int n_items, int n_max, int parity, const DecItem* items) {
  if (n_items <= 0 || n_max <= 0) return;
  hipLaunchKernelGGL(k_dec_candidates, dim3(cdiv(n_max, kDecBlock), n_items), dim3(kDecBlock), 0, st, items, parity);
}
void launch_dec_triangles(hipStream_t st, int n_items, int t_max, const DecItem* items, const DecTable* tables) {
  if (n_items <= 0) return;
  if (t_max > 0) {
    const dim3 per_triangle(cdiv(t_max, kDecBlock), n_items);
    hipLaunchKernelGGL(k_dec_insert, per_triangle, dim3(kDecBlock), 0, st, items, tables);
    hipLaunchKernelGGL(k_dec_keep, per_triangle, dim3(kDecBlock), 0, st, items, tables);
    hipLaunchKernelGGL(k_dec_block, dim3(cdiv(t_max, kScanTile), n_items), dim3(kDecBlock), 0, st, items);
  }
  hipLaunchKernelGGL(k_dec_totals, dim3(n_items), dim3(kDecBlock), 0, st, items, tables);
  if (t_max > 0) hipLaunchKernelGGL(k_dec_scatter, dim3(cdiv(t_max, kDecBlock), n_items), dim3(kDecBlock), 0, st, items, tables);
}

}  // namespace icp
