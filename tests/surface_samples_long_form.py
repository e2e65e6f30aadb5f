"""The rules of icp_surface_samples_many and icp_kernel_total_variance_many (include/icp_proposal.h) in numpy and
Python integers: the long form the GPU tests compare with, bit for bit.

    weights   A2_t = sqrt((nx nx + ny ny) + nz nz) of the cross product of e1 = b - a, e2 = c - a; Amax = max A2;
              q_t = (uint64) trunc((A2_t / Amax) 2^32); C = the inclusive prefix of q in integers, Q = C[T - 1]
    draws     h(seed, step, lane) = splitmix64(splitmix64(splitmix64(seed) ^ step K1) ^ lane K2) >> 11, u = (h + 0.5) 2^-53
              x = (h(seed, 0, k) Q) >> 53; the triangle is the first t with C_t > x; r = sqrt(u(seed, 1, k)), v = u(seed, 2, k)
              w = (1 - r, r (1 - v), r v); p = (w0 a + w1 b) + w2 c
    nearest   the first minimum of d2 = (dx dx + dy dy) + dz dz over all vertices (np.argmin: the lowest id of equal minima)
    trace     per point (entry 0 + entry 1) + entry 2 of the term expression at y = x, the terms summed in order; blocks of 256
              consecutive points, tr[i] += tr[i + s] for s = 128 .. 1, the block sums in block order, divided by n
"""
import numpy as np

import face_kernel_long_form as FK

K0, KA, KB = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
K1, K2 = 0xD1342543DE82EF95, 0x2545F4914F6CDD1D
MASK = (1 << 64) - 1
SCAN_TILE = 2048     # kScanTile: triangles of one workgroup of the device's prefix scan (the tests' edges; the long form has no tiles)
BLOCK = 256          # kSmpBlock: samples of one workgroup
VERTEX_TILE = 1024   # kSmpVertexTile: vertices of one LDS tile of the nearest-vertex search
NO_AREA = -3         # ICP_ERR_NOT_FINITE


def splitmix64(x):
    """over a uint64 array, the arithmetic modulo 2^64"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + np.uint64(K0)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(KA)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(KB)
        return x ^ (x >> np.uint64(31))


def h(seed, step, lanes):
    """the 53-bit integers of (seed, step, lane) for an array of lanes -> uint64"""
    lanes = np.atleast_1d(np.asarray(lanes, dtype=np.uint64))
    with np.errstate(over="ignore"):
        inner = splitmix64(np.uint64(seed & MASK)) ^ np.uint64((step * K1) & MASK)
        return splitmix64(splitmix64(inner) ^ (lanes * np.uint64(K2))) >> np.uint64(11)


def u_of(hh):
    return (hh.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def u(seed, step, lanes):
    return u_of(h(seed, step, lanes))


def double_areas(points, cells):
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    a, e1, e2 = p[c[:, 0]], p[c[:, 1]] - p[c[:, 0]], p[c[:, 2]] - p[c[:, 0]]
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    with np.errstate(over="ignore", invalid="ignore"):
        a2 = np.sqrt((nx * nx + ny * ny) + nz * nz)
    return np.where(np.isfinite(a2), a2, 0.0)


def weights(points, cells):
    """-> (q [T] uint64, C [T] uint64 inclusive prefix, Q int, Amax)"""
    a2 = double_areas(points, cells)
    amax = float(a2.max())
    if not amax > 0.0:
        z = np.zeros(a2.shape[0], dtype=np.uint64)
        return z, z, 0, 0.0
    q = np.trunc((a2 / amax) * 4294967296.0).astype(np.uint64)
    C = np.cumsum(q, dtype=np.uint64)
    Q = sum(int(v) for v in q) if q.shape[0] <= 4096 else int(C[-1])
    assert Q == int(C[-1]) and Q < 1 << 58
    return q, C, Q, amax


def picks(seed, n, Q):
    """x of samples 0 .. n-1 in Python integers -> uint64 [n]"""
    return np.array([(int(v) * Q) >> 53 for v in h(seed, 0, np.arange(n))], dtype=np.uint64)


def nearest_vertices(points, samples, chunk=64):
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    s = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 3)
    out = np.empty(s.shape[0], dtype=np.int32)
    px, py, pz = (np.ascontiguousarray(p[:, j]) for j in range(3))
    for k0 in range(0, s.shape[0], chunk):
        dx, dy, dz = s[k0:k0 + chunk, 0:1] - px[None, :], s[k0:k0 + chunk, 1:2] - py[None, :], s[k0:k0 + chunk, 2:3] - pz[None, :]
        d2 = (dx * dx + dy * dy) + dz * dz
        out[k0:k0 + chunk] = np.argmin(d2, axis=1)  # (the first of equal minima: the lowest id)
    return out


def squared_distance(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def long_form(points, cells, n, seed, vertex_ids=True, ids_for=None):
    """-> dict: points [n, 3], cells [n] int32, bary [n, 3], vertex_ids [n] int32 (or None; with ids_for only the first ids_for
    samples' ids), info [4], status"""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    q, C, Q, amax = weights(p, c)
    if Q == 0:
        return {"points": np.full((n, 3), np.nan), "cells": np.full(n, -1, dtype=np.int32), "bary": np.full((n, 3), np.nan),
                "vertex_ids": np.full(n, -1, dtype=np.int32) if vertex_ids else None, "info": np.zeros(4), "status": NO_AREA}
    x = picks(seed, n, Q)
    assert int(x.max()) < Q
    t = np.searchsorted(C, x, side="right")
    assert np.all(q[t] > 0)
    lanes = np.arange(n)
    r, v = np.sqrt(u(seed, 1, lanes)), u(seed, 2, lanes)
    w = np.stack([1.0 - r, r * (1.0 - v), r * v], axis=1)
    pts = (w[:, 0:1] * p[c[t, 0]] + w[:, 1:2] * p[c[t, 1]]) + w[:, 2:3] * p[c[t, 2]]
    ids = None
    if vertex_ids:
        ids = nearest_vertices(p, pts if ids_for is None else pts[:ids_for])
    half = 0.5 * amax
    info = np.array([float((q > 0).sum()), half, half * (float(Q) * (1.0 / 4294967296.0)), 0.0])
    return {"points": pts, "cells": t.astype(np.int32), "bary": w, "vertex_ids": ids, "info": info, "status": 0}


# ---------------------------------------------------------------- the mean trace of a kernel

def base_at(term, x, y):
    """b(x_i, y_i), elementwise over [n, 3] arrays"""
    if FK.is_gaussian(term):
        return np.exp(-(squared_distance(x, y) / (term.sigma * term.sigma)))
    c = 2.0 ** term.level
    return (FK.spline_sum(x[:, 0] * c, y[:, 0] * c) * FK.spline_sum(x[:, 1] * c, y[:, 1] * c)) * FK.spline_sum(x[:, 2] * c, y[:, 2] * c)


def traces(points, terms, point_weights=None):
    """trace k(x, x) per point [n]: (entry 0 + entry 1) + entry 2, every entry the terms summed in order"""
    x = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    d = np.zeros((x.shape[0], 3))
    for t, term in enumerate(terms):
        val = np.repeat(base_at(term, x, x)[:, None], 3, axis=1)
        if term.mirror_gain > 0.0:
            sgn = np.ones(3)
            sgn[term.mirror_axis] = -1.0
            xm = x.copy()
            xm[:, term.mirror_axis] = -xm[:, term.mirror_axis]
            val = val + (term.mirror_gain * sgn)[None, :] * base_at(term, x, xm)[:, None]
        w = None if point_weights is None else point_weights[t]
        ww = np.ones(x.shape[0]) if w is None else np.asarray(w, dtype=np.float64) * np.asarray(w, dtype=np.float64)
        d = d + ((term.scale * ww)[:, None] * val) * np.diag(np.asarray(term.A, dtype=np.float64))[None, :]
    return (d[:, 0] + d[:, 1]) + d[:, 2]


def tree_mean(tr):
    """the fixed shape of the device's sum"""
    tr = np.asarray(tr, dtype=np.float64)
    n = tr.shape[0]
    nblk = (n + BLOCK - 1) // BLOCK
    pad = np.zeros(nblk * BLOCK)
    pad[:n] = tr
    pad = pad.reshape(nblk, BLOCK)
    s = BLOCK // 2
    while s >= 1:
        pad[:, :s] = pad[:, :s] + pad[:, s:2 * s]
        s //= 2
    total = 0.0
    for v in pad[:, 0]:
        total = total + float(v)
    return total / float(n)


def total_variance(points, terms, point_weights=None):
    return tree_mean(traces(points, terms, point_weights))


# ---------------------------------------------------------------- the tests' meshes

def strip(T, growth=1.0):
    """a strip of T triangles over a 2 x (T/2 + 2) grid of points; column j is growth·j(j+1)/2 wide apart, so the areas grow along it"""
    cols = T // 2 + 2
    j = np.arange(cols, dtype=np.float64)
    xs = j + growth * 0.001 * j * (j + 1.0) / 2.0
    pts = np.concatenate([np.stack([xs, 0 * xs, 0 * xs], axis=1), np.stack([xs, 1.0 + 0 * xs, 0.25 * np.sin(j)], axis=1)])
    a = np.arange(cols - 1)
    lower, upper = np.stack([a, a + 1, a + cols], axis=1), np.stack([a + 1, a + cols + 1, a + cols], axis=1)
    cells = np.stack([lower, upper], axis=1).reshape(-1, 3)[:T]
    assert cells.shape[0] == T
    return pts, cells.astype(np.int32)


# ---------------------------------------------------------------- the tests' calls straight through the C ABI

OUTPUTS = ("points", "cells", "bary", "vertex_ids", "info")
CANARY, ICANARY, TAIL = -12345.0, -7, 5


def make(points, cells, n, seed=0):
    return {"points": np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3),
            "cells": np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3), "n": int(n), "seed": int(seed)}


def raw_call(pkg, items, nulls=None, whole_null=(), n_items=None, counts=None, status=True, expect=(0,)):
    """items through icp_surface_samples_many with canary-filled arrays that are TAIL rows longer than the call may write; nulls[b]:
    the outputs item b passes as NULL; whole_null: the output arguments passed as NULL altogether; counts: (M, T, n) overrides per
    item -> (rc, one dict per item: the arrays as the call left them without their tails, "tails_ok", "status")"""
    nat, lib = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    n = len(items)
    nulls = nulls or [()] * n
    i32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    sizes = [(i["points"].shape[0], i["cells"].shape[0], i["n"]) for i in items] if counts is None else counts
    n_pts, n_tri, ks = i32([s[0] for s in sizes]), i32([s[1] for s in sizes]), i32([s[2] for s in sizes])
    seeds = np.array([i["seed"] for i in items], dtype=np.uint64)
    out = []
    for i in items:
        k = i["n"] + TAIL
        out.append({"points": np.full((k, 3), CANARY), "cells": np.full(k, ICANARY, dtype=np.int32), "bary": np.full((k, 3), CANARY),
                    "vertex_ids": np.full(k, ICANARY, dtype=np.int32), "info": np.full(4 + TAIL, CANARY)})
    ptrs = lambda arrays, t: (t * n)(*[None if a is None else a.ctypes.data_as(t) for a in arrays])  # noqa: E731

    def given(name, t):
        if name in whole_null:
            return None
        return ptrs([None if name in nulls[b] else out[b][name] for b in range(n)], t)

    st = np.full(n, 99, dtype=np.int32)
    rc = lib.icp_surface_samples_many(n if n_items is None else n_items, 0, n_pts.ctypes.data_as(ip), ptrs([i["points"] for i in items], dp),
                                      n_tri.ctypes.data_as(ip), ptrs([i["cells"] for i in items], ip), ks.ctypes.data_as(ip),
                                      seeds.ctypes.data_as(nat.c_uint64_p), given("points", dp), given("cells", ip), given("bary", dp),
                                      given("vertex_ids", ip), given("info", dp), st.ctypes.data_as(ip) if status else None)
    assert rc in expect, (rc, lib.icp_last_error())
    res = []
    for b, i in enumerate(items):
        k = i["n"]
        d = {"status": int(st[b]), "tails_ok": True}
        for name in OUTPUTS:
            a, rows = out[b][name], (4 if name == "info" else k)
            canary = ICANARY if a.dtype == np.int32 else CANARY
            d["tails_ok"] = d["tails_ok"] and bool(np.all(a[rows:] == canary))
            absent = name in nulls[b] or name in whole_null
            if absent:
                d["tails_ok"] = d["tails_ok"] and bool(np.all(a == canary))
            d[name] = None if absent else a[:rows]
        res.append(d)
    return rc, res


def untouched(got):
    """every array the call was given still holds its canary"""
    return got["tails_ok"] and all(got[k] is None or np.all(got[k] == (ICANARY if got[k].dtype == np.int32 else CANARY)) for k in OUTPUTS)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_item(got, lf, what, ids_for=None):
    """what the call left is the long form's, to the bit (NaN included); an output passed as NULL is not compared"""
    assert got["status"] == lf["status"], (what, got["status"])
    assert got["tails_ok"], (what, "a row behind the item's was written")
    for name in OUTPUTS:
        if got[name] is None or lf[name] is None:
            continue
        a, b = got[name], lf[name]
        if name == "vertex_ids" and ids_for is not None:
            a, b = a[:ids_for], b[:ids_for]
        assert same(a, b), (what, name)
