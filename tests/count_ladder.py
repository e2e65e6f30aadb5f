"""The counts at which the library takes another path — K queries or correspondences, N model vertices, V searched vertices, T searched
triangles —, the meshes, models and query sets of those counts: the inputs of tests/test_gpu_counts.py, pinned without a GPU by
tests/test_count_ladder_cpu.py.  The rank ladders (tests/small_rank_ladder.py, tests/large_rank_ladder.py) cover the other dimension.

DISPATCH restates, in Python, every decision of the native code behind the per-method searches, the posterior's regression and the
merged step that depends on one of the counts (the file and function each one comes from is named beside it).  A decision is written
as what of it selects code — one workgroup or several, a loop that runs or does not, a list or a scan — not as a trip count: an edge
is a count at which a decision gives another answer for count + 1, and a ladder holds both sides of every edge of its count, and 1, 2
and 3 besides.  Where a decision hangs on two counts the pair is named in PAIRS.  The CPU test derives the edges from DISPATCH and
compares: a change of the dispatch code that moves an edge has to move the restatement here, and then the ladder.

Out of scope: what belongs to the `*_many` entry points alone (metrics, registration maps, projection slabs, gp models, batched fits:
met_cand / eval_cand, filter_grid_blocks over many items, regression_fold and regression_macro, which fold only when a launch carries
many posteriors).  tests/batched_count_ladder.py ladders that family.

Readings of the code that differ from the obvious one:
 * the stride of a candidate list does NOT depend on a context's history.  query_scratch only grows the scratch, but it grows it to
   `want` = (K + 4)·min(n, 4096) ints (at most kMaxCandidates) for the call at hand, and cand_stride_for caps capacity / (K + 4) at 4096
   and at n: a larger scratch left by an earlier call gives the same stride, and once `want` is capped (K > 16,380 at n >= 4096) a
   fresh context's scratch is the largest there is.  The same holds for query_batch (stride_after shows both; the GPU test runs it).
 * the stride starts to shrink at K = 16,380 | 16,381 (capacity / (K + 4) with capacity 64 Mi), not at 16,376 | 16,377.
 * `count.surface_exact_tests` cannot tell a listed query from an overflowed one without a hint: an unhinted query lists all T
   triangles, and surface_resolve adds n (= T) for a list and T for a scan.  Under a finite bound it does: Σn is far below K·T.
 * launch 1 of the merged step sizes its vertex part by Kpad, max(Kpad of the TargetSampling proposal, Kpad of the evaluator's reverse
   direction), not by K_t — the edge is 256 | 257 either way.
 * a leaf of the regression is walked four correspondences at a time and then one at a time (regression_tile): with a single leaf
   (K <= 8) that gives the edges 3 | 4, 4 | 5 and 7 | 8 besides regression_splits' own."""
import numpy as np

import designed_spectra as DS

# ---------------------------------------------------------------- constants of the native code

K_QU = 4                    # kQU (icp_search.hpp): queries per unrolled filter iteration; Kpad is a multiple
K_BLOCK = 256               # kBlock = kSearchBlock = kStepBlock: threads of a workgroup
SPHERES_PER_LANE = 2        # kSpheresPerLane: 128 triangles a wave, 512 a workgroup
FILTER_TILE = 128           # kFilterTile: queries of the vertex filter's LDS tile
SURFACE_TILE = 512          # kSurfaceTile
SURFACE_CHUNK = 256         # split_surface_queries: queries per surface workgroup of a lone chain
CAND_STRIDE = 512           # kCandStride
CAND_STRIDE_MAX = 4096      # kCandStrideMax
MAX_CANDIDATES = 64 << 20   # kMaxCandidates (abi_types.inl)
FILTER_WAVES = 4096         # split_queries: target_waves of one chain
STEP_BEGIN_POINTS = 128     # kStepBeginPoints
STEP_REDUCE_SPLITS = 32     # kStepReduceSplits
SMALL = 600                 # the small ladders end below this; the large shapes are PAIRS


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------- the dispatch, restated

def query_kpad(K):
    """kernels_fit.hip, query_kpad; make_surface_task / make_vertex_task (kernels_geometry.hip)"""
    return cdiv(K, K_QU) * K_QU


def cand_stride(n):
    """icp_kernels.hpp, cand_stride"""
    return (n if n > 0 else 1) if n < CAND_STRIDE else CAND_STRIDE


def cand_stride_for(n, K, capacity):
    """icp_kernels.hpp, cand_stride_for: entries per query of a batch of K queries given `capacity` ints"""
    s = capacity // (K + 4 if K + 4 > 0 else 1)
    s = min(s, CAND_STRIDE_MAX)
    s = max(s, CAND_STRIDE)
    return min(s, n if n > 0 else 1)


def scratch_want(K, n):
    """abi_types.inl, icp_ctx::query_scratch: the candidate ints a call of K queries against n elements asks for"""
    return min(MAX_CANDIDATES, max((K + 4) * min(max(n, 1), CAND_STRIDE_MAX), 1))


def query_batch(K, n, capacity):
    """kernels_geometry.hip, query_batch: queries per batch"""
    kb = capacity // cand_stride(n)
    if kb > 4:
        kb -= 4
    return min(max(kb, 1), K)


def search_plan(K, n, capacity=0):
    """launch_surface_query / launch_vertex_query on a context whose scratch holds `capacity` ints already -> [(queries, stride,
    listed without a hint)] per batch"""
    cap = max(capacity, scratch_want(K, n))
    kb = query_batch(K, n, cap)
    out = []
    for b0 in range(0, K, kb):
        k = min(kb, K - b0)
        s = cand_stride_for(n, k, cap)
        out.append((k, s, n <= s))
    return out


def stride_after(K, n, earlier=()):
    """the plan of a call after the calls `earlier` = [(K, n), ...] on the same context"""
    cap = 0
    for k, m in earlier:
        cap = max(cap, scratch_want(k, m))
    return search_plan(K, n, cap)


def split_surface_queries(Kpad, chains=1):
    """kernels_geometry.hip, split_surface_queries -> (ksplit, kchunk)"""
    tile = SURFACE_TILE if chains >= 16 else SURFACE_CHUNK
    kc = max(cdiv(min(Kpad, tile), K_QU) * K_QU, K_QU)
    return cdiv(Kpad, kc), kc


def split_queries(vblocks, Kpad, chains=1):
    """kernels_geometry.hip, split_queries -> (ksplit, kchunk)"""
    target = max(FILTER_WAVES // max(chains, 1), 1)
    s = max(cdiv(target, vblocks * (K_BLOCK // 64)), 1)
    s = max(min(s, cdiv(Kpad, 8)), 1)
    s = min(s, 65535)
    kc = cdiv(cdiv(Kpad, s), K_QU) * K_QU
    return cdiv(Kpad, kc), kc


def vertex_chunk_shape(V, K):
    """icp_search.hpp, vertex_filter: (LDS tiles a chunk takes, capped at 2 — the kt loop and its second barrier run from 2 on;
    groups of 64 queries in a tile, capped at 2)"""
    _, kc = split_queries(vblocks(V), query_kpad(K))
    return min(cdiv(kc, FILTER_TILE), 2), min(cdiv(min(kc, FILTER_TILE), 64), 2)


def tblocks(T):
    """make_surface_task: workgroups over the triangles"""
    return cdiv(T if T > 0 else 1, K_BLOCK * SPHERES_PER_LANE)


def vblocks(V):
    """make_vertex_task"""
    return cdiv(V if V > 0 else 1, K_BLOCK)


def live_waves(n, per_wave):
    """waves of the LAST workgroup that hold any element (surface_filter: wave_live, 128 triangles a wave; vertex_filter: 64)"""
    per_block = 4 * per_wave
    return cdiv((n - 1) % per_block + 1, per_wave)


def regression_splits(K):
    """kernels_posterior.hip, regression_splits"""
    return min(max(cdiv(K, 8), 1), 64)


def regression_kchunk(K):
    """launch_regression, chain_step_front (abi_step.inl)"""
    return max(cdiv(K, regression_splits(K)), 1)


def empty_leaves(K):
    """leaves whose slice [split·kchunk, …) starts at or past K: regression_tile writes zeros for them"""
    return regression_splits(K) - cdiv(K, regression_kchunk(K))


def regression_shape(K):
    """what of the regression's split selects code: one leaf or several (launch_sum_partials returns at once with one), the merged
    step's summing launch (kStepReduceSplits), kchunk <= 8 or above (the 64-leaf clamp at work), empty leaves or none"""
    S = regression_splits(K)
    return S == 1, S >= STEP_REDUCE_SPLITS, regression_kchunk(K) <= 8, empty_leaves(K) > 0


def single_leaf_loops(K):
    """icp_dense.hpp, regression_tile with one leaf (K <= 8): (the loop of four runs, the loop of one runs)"""
    return (K // 4 > 0, K % 4 > 0) if K <= 8 else None


def step_begin_grid(N, Kt_pad):
    """kernels_step.hip, launch_step_begin: ⌈N / 128⌉ workgroups of the instance + ⌈Kpad / 256⌉ of the vertex part"""
    return cdiv(N, STEP_BEGIN_POINTS) + cdiv(Kt_pad, K_BLOCK)


K_DISPATCH = {  # name -> (decision(K), first K, last K looked at)
    "query_kpad: sentinel slots": (lambda K: query_kpad(K) > K, 1, 8),
    "split_surface_queries, lone chain: one workgroup a block of spheres / several": (lambda K: min(split_surface_queries(query_kpad(K))[0], 2), 1, SMALL),
    "split_surface_queries, 16 chains or more": (lambda K: min(split_surface_queries(query_kpad(K), 16)[0], 2), 1, SMALL),
    "surface_filter: groups of 64 queries in a chunk": (lambda K: min(cdiv(split_surface_queries(query_kpad(K))[1], 64), 2), 1, SMALL),
    "cdiv(Kpad, kBlock): k_surface_init, k_vertex_init, launch 1's vertex part": (lambda K: min(cdiv(query_kpad(K), K_BLOCK), 2), 1, SMALL),
    "cdiv(K, kBlock): k_correspond_*, k_gather_points": (lambda K: min(cdiv(K, K_BLOCK), 2), 1, SMALL),
    "regression_splits, kchunk, empty leaves, kStepReduceSplits": (regression_shape, 1, SMALL),
    "regression_tile: loops of a single leaf": (single_leaf_loops, 1, 8),
}
T_DISPATCH = {
    "surface_filter: a lane with one sphere (odd T)": (lambda T: T % 2, 1, 4),
    "surface_filter: live waves of the last workgroup; coherent_triangle_order: kd_runs above 128": (lambda T: live_waves(T, 128), 1, 512),
    "tblocks": (lambda T: min(tblocks(T), 2), 1, SMALL),
    "cand_stride: all of them / kCandStride": (lambda T: T < CAND_STRIDE, 1, SMALL),
    "cand_stride_for without a hint: listed / overflowed (kCandStrideMax)": (lambda T: search_plan(5, T)[0][2], 1, 4200),
}
V_DISPATCH = {
    "vertex_filter: live waves of the last workgroup": (lambda V: live_waves(V, 64), 1, 256),
    "vblocks": (lambda V: min(vblocks(V), 2), 1, SMALL),
    "cand_stride: all of them / kCandStride": (lambda V: V < CAND_STRIDE, 1, SMALL),
    "cand_stride_for without a hint: listed / overflowed (kCandStrideMax)": (lambda V: search_plan(5, V)[0][2], 1, 4200),
}
N_DISPATCH = {
    "launch 1: waves of the last workgroup that carry a point (two of four)": (lambda N: live_waves(N, 64) if N <= 128 else 2, 1, 128),
    "launch 1: cdiv(N, kStepBeginPoints)": (lambda N: min(cdiv(N, STEP_BEGIN_POINTS), 2), 1, SMALL),
    "cdiv(N, kBlock): k_instance*, k_vertex_normals": (lambda N: min(cdiv(N, K_BLOCK), 2), 1, SMALL),
}
DISPATCH = {"K": K_DISPATCH, "T": T_DISPATCH, "V": V_DISPATCH, "N": N_DISPATCH}


def edges(decision, lo, hi):
    """the counts c in lo..hi-1 with decision(c) != decision(c + 1)"""
    return [c for c in range(lo, hi) if decision(c) != decision(c + 1)]


def derived_ladder(table):
    out = {1, 2, 3}
    for fn, lo, hi in table.values():
        for c in edges(fn, lo, hi):
            out.update((c, c + 1))
    return tuple(sorted(out))


def stands_for(count, table):
    """the edges a count is a side of (DESIGN.md §9.4 is written from this)"""
    return [f"{name} {c} | {c + 1}" for name, (fn, lo, hi) in table.items() for c in edges(fn, lo, hi) if count in (c, c + 1)]


K_LADDER = (1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 248, 249, 256, 257, 512, 513, 567, 568, 576, 577)
T_LADDER = (1, 2, 3, 4, 128, 129, 256, 257, 384, 385, 511, 512, 513, 4096, 4097)
V_LADDER = (1, 2, 3, 64, 65, 128, 129, 192, 193, 256, 257, 511, 512, 4096, 4097)
N_LADDER = (1, 2, 3, 64, 65, 128, 129, 256, 257)

# decisions on two counts: name -> (kind, the fixed count, decision(K), first K, last K) and the K on both sides of their edges
PAIR_DISPATCH = {
    "stride shrinks once (K + 4)·4096 passes kMaxCandidates (K, T >= 4097)": ("surface", 4097, lambda K: search_plan(K, 4097)[0][1] == CAND_STRIDE_MAX, 16000, 16800),
    "query_batch: a second batch (K, T >= 512)": ("surface", 520, lambda K: min(len(search_plan(K, 520)), 2), 130900, 131200),
    "vertex_filter: groups of 64 in a tile, LDS tiles a chunk (V = 2,560, K)": ("vertex", 2560, lambda K: vertex_chunk_shape(2560, K), 6000, 13600),
}
PAIRS = (  # (kind, n elements, K): the smallest shapes that reach those edges
    ("surface", 4097, 16380), ("surface", 4097, 16381),
    ("surface", 520, 131068), ("surface", 520, 131069),
    ("vertex", 2560, 6592), ("vertex", 2560, 6593), ("vertex", 2560, 13184), ("vertex", 2560, 13185),
)


def derived_pairs():
    out = []
    for kind, n, fn, lo, hi in PAIR_DISPATCH.values():
        for K in edges(fn, lo, hi):
            out += [(kind, n, K), (kind, n, K + 1)]
    return tuple(out)


REGRESSION_KS = (1, 7, 8, 9, 16, 17, 248, 249, 511, 512, 513, 567, 568, 576, 577)  # and N: (d) of tests/test_gpu_counts.py
MERGED_NS = (127, 128, 129, 255, 256, 257, 600)                                       # (e); 600: several workgroups of every launch
MERGED_KS = (255, 256, 257)
HINTED_KS = tuple(K for K in K_LADDER if K <= 520)                                    # (c)
RANKS = (12, 40)  # one 16 × 16 regression tile; three tile rows (small_rank_ladder.regression_tiles: 1 and 6 tiles)


# ---------------------------------------------------------------- the meshes, all made from counts

def _grid_points(a, b, flat):
    i, j = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    if flat:
        return np.stack([i, j, 0 * i], axis=-1).reshape(-1, 3).astype(np.float64)
    return np.stack([10.0 * i, 10.0 * j, 4.0 * np.sin(0.5 * i) * np.cos(0.4 * j)], axis=-1).reshape(-1, 3).astype(np.float64)


def curved_grid(a, b):
    """designed_spectra.grid_mesh((a, b)): 10 mm between neighbours, gently curved; the cells (p, q, s) of every square first, then
    the cells (q, t, s)"""
    return DS.grid_mesh((a, b))


def flat_grid(a, b):
    """the same triangulation on integer coordinates (i, j, 0): distances and ties are exact in floating point"""
    return _grid_points(a, b, True), DS.grid_mesh((a, b))[1]


def cut_mesh(V=None, T=None, cols=16):
    """a gently curved grid of `cols` columns cut to exactly T triangles and V vertices.  The triangles go square by square (both
    triangles of a square together, as a mesh file lists neighbours together), the vertices in the order the triangles first use
    them, then the rest of the grid row by row; the first T triangles and the first V vertices are kept.  T = None: every triangle
    whose corners are among the V vertices; V = None: the vertices the T triangles use."""
    assert V is not None or T is not None
    need_v = V if V is not None else 0
    need_t = T if T is not None else 0
    rows = max(2, cdiv(need_v, cols) + 1, cdiv(cdiv(need_t, 2), cols - 1) + 1)
    pts = _grid_points(rows, cols, False)
    idx = np.arange(rows * cols).reshape(rows, cols)
    p, q, s, t = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    cells = np.stack([np.stack([p, q, s], axis=1), np.stack([q, t, s], axis=1)], axis=1).reshape(-1, 3)
    if T is not None:
        cells = cells[:T]
    _, first = np.unique(cells.ravel(), return_index=True)
    used = cells.ravel()[np.sort(first)]
    rest = np.setdiff1d(np.arange(rows * cols), used)
    order = np.concatenate([used, rest])
    if V is None:
        V = used.shape[0]
    order = order[:V]
    new_id = -np.ones(rows * cols, dtype=np.int64)
    new_id[order] = np.arange(V)
    cells = new_id[cells]
    cells = cells[(cells >= 0).all(axis=1)]
    assert order.shape[0] == V and (T is None or cells.shape[0] == T), (V, T, order.shape, cells.shape)
    return pts[order].copy(), cells.astype(np.int32)


def torus_mesh(a, b, extra=0, R=40.0, r0=15.0):
    """closed: a × b vertices on a torus, 2ab triangles square by square; `extra` more vertices, each put at the centroid of a
    triangle of its own, which it splits into three (N = ab + extra, T = 2N: closed for every N, primes included)"""
    assert a >= 3 and b >= 3 and 0 <= extra <= a * b // 4
    i, j = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    u, v = 2.0 * np.pi * i / a, 2.0 * np.pi * j / b
    pts = np.stack([(R + r0 * np.cos(u)) * np.cos(v), (R + r0 * np.cos(u)) * np.sin(v), r0 * np.sin(u)], axis=-1).reshape(-1, 3)
    idx = np.arange(a * b).reshape(a, b)
    p, q, s, t = idx, np.roll(idx, -1, axis=0), np.roll(idx, -1, axis=1), np.roll(np.roll(idx, -1, axis=0), -1, axis=1)
    cells = np.stack([np.stack([p.ravel(), q.ravel(), s.ravel()], axis=1), np.stack([q.ravel(), t.ravel(), s.ravel()], axis=1)], axis=1).reshape(-1, 3)
    cells, pts = [tuple(c) for c in cells], list(pts)
    for k in range(extra):
        c = 8 * k + 3
        x, y, z = cells[c]
        m = len(pts)
        pts.append((pts[x] + pts[y] + pts[z]) / 3.0)
        cells[c] = (x, y, m)
        cells += [(y, z, m), (z, x, m)]
    return np.array(pts, dtype=np.float64), np.array(cells, dtype=np.int32)


def closed_mesh(N, R=40.0, r0=15.0):
    """torus_mesh of exactly N vertices: the largest a·b <= N with a, b >= 3 and a as near √N as it goes, the rest as split triangles"""
    best = None
    for a in range(3, int(np.sqrt(N)) + 1):
        b = N // a
        if b >= 3 and (best is None or a * b >= best[0] * best[1]):
            best = (a, b)
    assert best is not None, N
    return torus_mesh(best[0], best[1], N - best[0] * best[1], R, r0)


def with_degenerates(mesh):
    """three triangles inserted at the lowest indices: (v, v, w) with a repeated corner — a segment whose Ericson form is the corner v
    or NaN —, (u, u, u), a point, and three vertices of one grid column (collinear on a flat grid, a sliver on a curved one); v is the
    vertex nearest the mesh's centroid, u = v + 3"""
    pts, cells = mesh
    m = int(np.argmin(((pts - pts.mean(axis=0)) ** 2).sum(axis=1)))
    deg = np.array([[m, m, m + 1], [m + 3, m + 3, m + 3], [m - 3, m - 2, m - 1]], dtype=np.int32)
    return pts, np.concatenate([deg, cells], axis=0).astype(np.int32)


def tiny_mesh(V):
    """V = 1: one vertex and the point triangle (0, 0, 0); V = 2: two vertices and the segment (0, 0, 1)"""
    assert V in (1, 2)
    pts = np.array([[3.0, -1.0, 2.0], [11.0, 4.0, -2.0]])[:V]
    return pts.copy(), np.array([[0, 0, V - 1]], dtype=np.int32)


def ladder_mesh(count, n):
    """the mesh of one entry of T_LADDER / V_LADDER"""
    if count == "T":
        return cut_mesh(T=n)
    return tiny_mesh(n) if n < 3 else cut_mesh(V=n)


def model_on(pkg, mesh, r, seed, variance=None):
    """designed_spectra.orthonormal_model on a mesh of this module: an orthonormal basis, variances 400 .. 25 mm² (a unit coefficient
    moves the mesh by √(λ / 3N) a coordinate: a fraction of the 10 mm between neighbours)"""
    pts, cells = mesh
    n = pts.shape[0]
    assert 3 * n >= r
    rng = np.random.default_rng(seed)
    lam = np.geomspace(400.0, 25.0, r) if variance is None else np.asarray(variance, dtype=np.float64)
    return pkg.data.StatisticalMeshModel(pts.copy(), cells.copy(), np.zeros_like(pts), DS.random_orthonormal(rng, 3 * n, r), lam)


def as_target(pkg, mesh):
    return pkg.data.TriangleMesh(mesh[0].copy(), mesh[1].copy())


# ---------------------------------------------------------------- query sets

def random_queries(mesh, K, seed, sd=6.0):
    """`random`: vertices of the mesh drawn with replacement, moved by a Gaussian of sd (mm) a coordinate"""
    rng = np.random.default_rng(seed)
    pts = mesh[0]
    return pts[rng.integers(0, pts.shape[0], size=K)] + sd * rng.normal(size=(K, 3))


TIED = {  # `tied`, on flat_grid: name -> offset from an interior vertex (i, j, 0)
    "above a vertex shared by six triangles": (0.0, 0.0, 0.5),
    "above an edge midpoint": (0.5, 0.0, 0.5),
    "above a cell centre, on the diagonal, equidistant from four vertices": (0.5, 0.5, 0.5),
    "in the plane, on a vertex": (0.0, 0.0, 0.0),
}
# offsets that have ONE winner, the highest-indexed member of the tie the placement of the same name makes: the states of a hinted
# sequence that come before the tied one.  Triangles: of the six around (i, j) the highest is (q, t, s) of the square (i, j − 1), with
# corners (i + 1, j − 1), (i + 1, j), (i, j); (0.5, −0.25) lies inside it.  Vertices: of the four around a cell centre the highest is
# (i + 1, j + 1).
BEFORE_TIE = {"triangles": (0.5, -0.25, 0.5), "vertices": (0.75, 0.75, 0.5)}


def interior_vertices(a, b):
    idx = np.arange(a * b).reshape(a, b)
    return idx[1:-1, 1:-1].ravel()


def tied_queries(a, b, offset):
    """the interior vertices of flat_grid(a, b), each moved by `offset`"""
    return flat_grid(a, b)[0][interior_vertices(a, b)] + np.asarray(offset, dtype=np.float64)[None, :]


FAR_SHIFTS = tuple(float(2 ** e) * np.array([1.0, -0.75, 0.5]) for e in (13, 20, 26))
SCALES = (2.0 ** -10, 2.0 ** 10)


# ---------------------------------------------------------------- references in numpy, independent of the oracle

def closest_point_triangle_np(p, a, b, c):
    """Ericson's closest point on a triangle (Real-Time Collision Detection §5.1.5), vectorised over leading axes, with separately
    rounded multiplies and adds in the order of icp_oracle.c -> points; NaN where the form divides 0 by 0"""
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        e_ab = a + (d1 / (d1 - d3))[..., None] * ab
        e_ac = a + (d2 / (d2 - d6))[..., None] * ac
        e_bc = b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b)
        den = 1.0 / ((va + vb) + vc)
        inner = (a + ab * (vb * den)[..., None]) + ac * (vc * den)[..., None]
    conds = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), (d6 >= 0.0) & (d5 <= d6),
             (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0)]
    picks = [np.broadcast_to(a, inner.shape), np.broadcast_to(b, inner.shape), e_ab, np.broadcast_to(c, inner.shape), e_ac, e_bc]
    out = inner
    for cond, pick in zip(reversed(conds), reversed(picks)):
        out = np.where(cond[..., None], pick, out)
    return out


def lexmin(d2):
    """per row: the lexicographic (d², index) minimum, NaN never winning -> (index, d², how many share the minimum)"""
    d = np.where(np.isnan(d2), np.inf, d2)
    best = d.min(axis=1)
    return d.argmin(axis=1).astype(np.int32), best, (d == best[:, None]).sum(axis=1)


def surface_reference(q, mesh, chunk=256):
    """-> (triangle, d², multiplicity, closest point) of every query"""
    pts, cells = mesh
    a, b, c = pts[cells[:, 0]][None], pts[cells[:, 1]][None], pts[cells[:, 2]][None]
    tri, d2, mult, cp = [], [], [], []
    for k0 in range(0, q.shape[0], chunk):
        p = q[k0:k0 + chunk, None, :]
        o = closest_point_triangle_np(p, a, b, c)
        d = p - o
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i, best, m = lexmin(dd)
        tri.append(i), d2.append(best), mult.append(m), cp.append(o[np.arange(o.shape[0]), i])
    return np.concatenate(tri), np.concatenate(d2), np.concatenate(mult), np.concatenate(cp)


def vertex_reference(q, pts):
    d = q[:, None, :] - pts[None, :, :]
    return lexmin((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


# ---------------------------------------------------------------- hinted sequences: scenes of (c)

STEP, SIGMA_T, SIGMA_N = 0.1, 10.0, 5.0  # the parity configuration
DIRECTIONS = ("ModelSampling", "TargetSampling")


class Scene:
    """a model mesh, a target mesh, target-side sample points and a sequence of states; `scale` multiplies every length of it
    (a power of two: exact), `shift` moves target, sample points and the states' translation alike"""

    def __init__(self, name, model_mesh, target_mesh, tp, states, r, scale=1.0, shift=None, flat=False, states_t=None):
        shift = np.zeros(3) if shift is None else np.asarray(shift, dtype=np.float64)
        self.name, self.r, self.scale, self.flat = name, r, scale, flat
        self.model_mesh = (model_mesh[0] * scale, model_mesh[1])
        self.target_mesh = ((target_mesh[0] + shift) * scale, target_mesh[1])
        self.tp = (np.asarray(tp, dtype=np.float64) + shift) * scale
        self.shift = shift
        self.states = states      # [(translation, coefficients)] before shift and scale
        self.states_t = states_t  # the TargetSampling side's, where they differ

    def model(self, pkg):
        lam = np.geomspace(400.0, 25.0, self.r) * self.scale ** 2
        m = model_on(pkg, self.model_mesh, self.r, 11, variance=lam)
        return m

    def noise(self):
        return SIGMA_T * self.scale, SIGMA_N * self.scale

    def states_of(self, direction):
        return self.states_t if direction == "TargetSampling" and self.states_t is not None else self.states

    def theta(self, s, bump=0.0, direction="ModelSampling"):
        """state s; `bump` (a multiple of 2⁻¹⁰) moves it along x so that no two calls of a context see the same θ"""
        t, c = self.states_of(direction)[s]
        theta = np.zeros(10 + self.r)
        theta[0] = 1.0
        theta[1:4] = (np.asarray(t, dtype=np.float64) + self.shift + np.array([bump, 0.0, 0.0])) * self.scale
        theta[10:] = c
        return theta


def curved_scene(r=12, scale=1.0, shift=None, degenerate=False, name="curved grid"):
    """a 24 × 25 model grid (N = 600) over a 30 × 31 target grid with another phase; four states half a cell of integer or half-integer
    translation and a small shape move apart"""
    model_mesh = curved_grid(24, 25)
    tp_, tc = curved_grid(30, 31)
    tp_ = tp_ + np.array([-28.0, -31.0, 1.5])
    tp_[:, 2] += 1.5 * np.cos(0.07 * tp_[:, 0]) * np.sin(0.05 * tp_[:, 1])
    target_mesh = (tp_, tc)
    if degenerate:
        target_mesh = with_degenerates(target_mesh)
    rng = np.random.default_rng(31)
    samples = tp_[rng.permutation(tp_.shape[0])[:SMALL]] + 0.0
    c0 = 0.4 * rng.normal(size=r)
    states = [((3.0, -2.0, 1.5), c0), ((8.5, -2.0, 2.0), c0 + 0.05 * rng.normal(size=r)), ((8.5, 4.0, 2.0), c0 + 0.1 * rng.normal(size=r)),
              ((2.0, -1.0, 0.5), c0 + 0.1 * rng.normal(size=r))]
    if degenerate:
        # on a smooth surface no query has a vertex as its closest point: the point triangle's vertex and the segment's corner are
        # drawn into spikes whose tips lie 0.5 mm from the model vertex nearest in state 1, on the target's side of it along z — every
        # edge of the spike leads away from that vertex, so the tip is its closest point: the point (the corner) ties the triangles
        # around it and is listed before them
        t1, c1 = states[1]
        basis = DS.random_orthonormal(np.random.default_rng(11), 3 * model_mesh[0].shape[0], r)   # model_on(…, seed 11)
        x1 = model_mesh[0] + ((basis * np.sqrt(np.geomspace(400.0, 25.0, r))[None, :]) @ c1).reshape(-1, 3) + np.asarray(t1)
        pts, cells = target_mesh
        pts = pts.copy()
        for w in (cells[0, 0], cells[1, 0]):
            j = int(np.argmin(((x1 - pts[w]) ** 2).sum(axis=1)))
            pts[w] = x1[j] + np.array([0.0, 0.0, 0.5 if pts[w][2] > x1[j][2] else -0.5])
        target_mesh = (pts, cells)
    return Scene(name, model_mesh, target_mesh, samples, states, r, scale, shift)


FLAT = (13, 17)  # the flat grids of the tied scenes: 221 vertices, 384 triangles


def tied_scene(r=12):
    """model and target the same flat grid, coefficients zero, pure translations: every model vertex keeps the offset of the state from
    its target vertex.  States: one winner each (the highest-indexed triangle of the six), then above the vertex (six tied, the
    hint the highest), above an edge midpoint, above the cell centre (two triangles tied; the surface point is equidistant from four
    vertices), in the plane on the vertex.  The sample points of the other direction are the cell centres of the model at rest: the
    states before the last put the model's vertex (i + 1, j + 1) nearest, the tied ones all four."""
    a, b = FLAT
    mesh = flat_grid(a, b)
    centres = flat_grid(a, b)[0].reshape(a, b, 3)[:-1, :-1].reshape(-1, 3) + np.array([0.5, 0.5, 0.5])
    z = np.zeros(r)
    states = [(BEFORE_TIE["triangles"], z), (TIED["above a vertex shared by six triangles"], z), (TIED["above an edge midpoint"], z),
              (TIED["above a cell centre, on the diagonal, equidistant from four vertices"], z), (TIED["in the plane, on a vertex"], z)]
    return Scene("flat grid, tied", mesh, mesh, centres, states, r, flat=True, states_t=[(t, z) for t in tied_vertex_states()])


def tied_vertex_states():
    """translations of the model for the TargetSampling side of the tied scene: sample point k sits 0.5 above cell centre k of the
    model at rest.  First the model moved so that vertex (i + 1, j + 1) alone is nearest, then at rest: four vertices tied, the
    hint the highest of them."""
    return [(-0.25, -0.25, 0.0), (0.0, 0.0, 0.0), (-0.25, -0.25, 0.25), (0.0, 0.0, 0.25)]


def hinted_scenes():
    out = {"curved": curved_scene(), "degenerate": curved_scene(degenerate=True, name="target with degenerate triangles"), "tied": tied_scene()}
    for e, sh in zip((13, 20, 26), FAR_SHIFTS):
        out[f"far 2^{e}"] = curved_scene(shift=sh, name=f"shifted by 2^{e}·(1, −0.75, 0.5)")
    for sc in SCALES:
        out[f"scaled {sc:g}"] = curved_scene(scale=sc, name=f"scaled by {sc:g}")
    return out


# ---------------------------------------------------------------- the long form of a proposal's regression

def regression_long_form(model, theta, corr_id, corr_pt, keep, normals, sigma_t=SIGMA_T, sigma_n=SIGMA_N):
    """M and α of posterior_long_form.long_form for the kept correspondences of an unrotated state: observations y = point − t (model
    space), precision (1/σt²)·I + (1/σn² − 1/σt²)·n nᵀ with n the unit vertex normal of the instance at the correspondence's vertex"""
    import posterior_long_form as LF
    assert not theta[4:7].any() and theta[0] == 1.0
    k = np.flatnonzero(keep)
    n = normals[corr_id[k]]
    wt = 1.0 / sigma_t ** 2
    prec = wt * np.eye(3)[None] + (1.0 / sigma_n ** 2 - wt) * n[:, :, None] * n[:, None, :]
    lf = LF.long_form(model, corr_id[k], corr_pt[k] - theta[1:4][None, :], covariances=np.linalg.inv(prec))
    return lf["M"], lf["alpha"]


class RegressionCase:
    """(d): the 24 × 25 curved grid as a model of rank r (N = 600, open: its rim is boundary) over the 30 × 31 target of curved_scene,
    one unrotated state.  ModelSampling keeps every correspondence (the target reaches past the model on every side).  TargetSampling's
    sample points are made from the state's instance: point k sits 0.5 mm beside a vertex of the rim — dropped, boundary aware — where k
    is the first or the last correspondence of an even-numbered leaf or the last of all, and beside an interior vertex otherwise."""

    def __init__(self, pkg, r):
        sc = curved_scene(r)
        self.r, self.model, self.target_mesh = r, sc.model(pkg), sc.target_mesh
        self.theta = sc.theta(0)
        self.x = self.model.instance(self.theta[10:]) + self.theta[1:4][None, :]
        idx = np.arange(600).reshape(24, 25)
        self.interior = idx[2:-2, 2:-2].ravel()
        self.rim = np.concatenate([idx[0, :], idx[-1, :], idx[1:-1, 0], idx[1:-1, -1]])

    def drop_pattern(self, K):
        kc = regression_kchunk(K)
        k = np.arange(K)
        drop = ((k % kc == 0) | (k % kc == kc - 1)) & ((k // kc) % 2 == 0)
        drop |= k == K - 1
        return drop & (K > 1)

    def samples(self, K):
        rng = np.random.default_rng(1000 + K)
        drop = self.drop_pattern(K)
        v = np.where(drop, self.rim[rng.integers(0, self.rim.shape[0], size=K)], self.interior[rng.integers(0, self.interior.shape[0], size=K)])
        return self.x[v] + 0.5 * rng.normal(size=(K, 3)), (~drop).astype(np.uint8)

    def params(self, oracle, direction, K):
        """-> (the oracle's proposal parameters, the keep flags the design asks for or None: all kept, the sample points or None)"""
        if direction == "ModelSampling":
            return oracle.proposal_params(STEP, SIGMA_T, SIGMA_N, oracle.MODEL_SAMPLING, True, n_model_ids=K), None, None
        tp, keep = self.samples(K)
        return oracle.proposal_params(STEP, SIGMA_T, SIGMA_N, oracle.TARGET_SAMPLING, True, target_pts=tp), keep, tp


_regression_cases = {}


def regression_case(pkg, r):
    if r not in _regression_cases:
        _regression_cases[r] = RegressionCase(pkg, r)
    return _regression_cases[r]
