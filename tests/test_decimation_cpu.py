"""CPU: mesh decimation (icp_decimate_many, api.decimated_meshes, data.decimate, data.mesh_edge_census) — the numpy long form the GPU
tests compare with (tests/decimation_long_form.py) against a brute-force loop in plain Python, literal statements of the lattice's
ties, the femur facts of DESIGN.md §5.18, the prefix property, the ABI surface, the Python-side argument checks with the native
library stubbed out, and the real library's refusal of every bad argument before it touches a device."""
import ctypes
import os
import struct

import numpy as np
import pytest

import decimation_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def brute_force(points, cells, k, start=0):
    """the rules once more, without numpy: loops over vertices for the selection, dicts of (distance, label) tuples for the sweeps
    (the sum of two f32 is exact in a Python float: one rounding to f32), a set for the triples seen
    -> (ids, cover2, labels, triangles, sweeps)"""
    pts = [tuple(float(x) for x in p) for p in points]
    M = len(pts)

    def d2(a, b):
        dx, dy, dz = pts[a][0] - pts[b][0], pts[a][1] - pts[b][1], pts[a][2] - pts[b][2]
        return (dx * dx + dy * dy) + dz * dz

    ids, cover2 = [start], []
    D = [d2(v, start) for v in range(M)]
    while True:
        best = 0
        for v in range(1, M):
            if D[v] > D[best]:
                best = v
        cover2.append(D[best])
        if len(ids) == min(k, M) or D[best] == 0.0:
            break
        ids.append(best)
        D = [min(D[v], d2(v, best)) for v in range(M)]
    edges = set()
    for c in cells:
        c = [int(x) for x in c]
        for a in range(3):
            for b in range(3):
                if c[a] != c[b]:
                    edges.add((c[a], c[b]))
    key = {v: None for v in range(M)}
    for j, v in enumerate(ids):
        key[v] = (0.0, j)
    sweeps = 0
    while True:
        nxt = dict(key)
        for u, v in edges:
            if key[u] is None:
                continue
            cand = (f32(key[u][0] + f32(d2(u, v) ** 0.5)), key[u][1])
            if nxt[v] is None or cand < nxt[v]:
                nxt[v] = cand
        if nxt == key:
            break
        key = nxt
        sweeps += 1
    labels = [-1 if key[v] is None else key[v][1] for v in range(M)]
    seen, tris = set(), []
    for c in cells:
        l = [labels[int(x)] for x in c]
        if min(l) < 0 or len(set(l)) < 3:
            continue
        at = l.index(min(l))
        canon = (l[at], l[(at + 1) % 3], l[(at + 2) % 3])
        if canon not in seen:
            seen.add(canon)
            tris.append(list(canon))
    return ids, cover2, labels, tris, sweeps


def _compare(points, cells, k, start=0):
    lf = LF.long_form(points, cells, k, start)
    ids, cover2, labels, tris, sweeps = brute_force(points, cells, k, start)
    assert lf["ids"].tolist() == ids and lf["cover2"].tolist() == cover2
    assert lf["labels"].tolist() == labels and lf["cells"].tolist() == tris
    assert lf["counts"] == (len(ids), len(tris), sweeps)
    assert np.array_equal(lf["points"], np.asarray(points, dtype=np.float64)[ids])
    return lf


@pytest.mark.parametrize("k,start", [(1, 0), (2, 0), (5, 0), (9, 0), (13, 40), (30, 7), (80, 3), (81, 0), (86, 80)])
def test_long_form_against_a_brute_force_loop(k, start):
    pts, cells = LF.lattice(81)
    assert pts.shape == (81, 3) and cells.shape == (128, 3) and np.array_equal(pts[9 * 4 + 7], [4.0, 7.0, 0.0])
    lf = _compare(pts, cells, k, start)
    assert lf["counts"][0] == min(k, 81) and np.all(np.diff(lf["cover2"]) <= 0)
    if k >= 81:
        assert sorted(lf["ids"].tolist()) == list(range(81)) and lf["cover2"][-1] == 0.0 and lf["counts"][1] == 128 and lf["counts"][2] == 0
    # … with a second component, a loose vertex, a repeated triangle, a flipped one and a degenerate one
    more = np.concatenate([pts, [[20.0, 20.0, 1.0], [21.0, 20.0, 1.0], [20.0, 21.0, 1.0], [-5.0, -5.0, 2.0]]])
    extra = np.array([[81, 82, 83], [3, 4, 12], [12, 4, 3], [3, 4, 12], [5, 5, 6]], dtype=np.int32)
    _compare(more, np.concatenate([cells, extra]), k, start)


def test_literal_statements_of_the_ties():
    pts, cells = LF.lattice(81)
    assert LF.select(pts, 9)[0].tolist() == [0, 80, 8, 72, 40, 4, 36, 44, 76]
    lf = LF.long_form(pts, cells, 5)
    assert lf["labels"][:9].tolist() == [0, 0, 0, 0, 0, 2, 2, 2, 2]  # vertex 4 is two edges from samples 0 and 2: the lowest label
    assert lf["cells"].tolist() == [[0, 4, 2], [1, 2, 4], [0, 3, 4], [1, 4, 3]]
    x = np.repeat(np.arange(4.0), 3)
    lf = LF.long_form(np.stack([x, 0 * x, 0 * x], axis=1), np.zeros((0, 3), dtype=np.int32), 10)
    assert lf["ids"].tolist() == [0, 9, 3, 6] and lf["cover2"].tolist() == [9.0, 1.0, 1.0, 0.0] and lf["counts"] == (4, 0, 0)
    assert lf["labels"].tolist() == [0, -1, -1, 2, -1, -1, 3, -1, -1, 1, -1, -1]  # (no edges: only the samples have a label)
    # two components with k = 1: the other component's labels are −1
    two = np.concatenate([pts[:9], pts[:9] + [0.0, 0.0, 5.0]])
    lf = LF.long_form(two, np.array([[0, 1, 2], [9, 10, 11]]), 1)
    assert lf["labels"].tolist() == [0, 0, 0] + [-1] * 15 and lf["counts"] == (1, 0, 1)


@pytest.fixture(scope="module")
def femur_meshes(pkg):
    reference, _, _ = pkg.data.load_femur_mesh("femur_reference")
    _, target = pkg.data.load_femur_model_and_target(50)
    assert reference.n_points == 1622 and target.n_points == 1622
    return {"reference": reference, "target": target}


@pytest.fixture(scope="module")
def femur_ladders(femur_meshes):
    """one selection at the largest count per mesh: every smaller count is its prefix"""
    return {name: LF.select(mesh.points, 1200) for name, mesh in femur_meshes.items()}


@pytest.mark.parametrize("name", ["reference", "target"])
@pytest.mark.parametrize("k", [102, 400, 1200])
def test_femur_decimations_are_closed_manifolds(pkg, femur_meshes, femur_ladders, name, k):
    mesh = femur_meshes[name]
    ids = femur_ladders[name][0][:k]
    labels, sweeps = LF.label(mesh.points, mesh.cells, ids)
    tri = LF.dual_triangles(labels, mesh.cells)
    assert labels.min() == 0 and labels.max() == k - 1 and 1 <= sweeps <= 26
    assert tri.shape[0] == 2 * k - 4
    assert LF.edge_census(tri, k) == (0, 3 * k - 6, 0, 2)
    census = pkg.data.mesh_edge_census(pkg.data.TriangleMesh(mesh.points[ids], tri))
    assert census == {"boundary": 0, "interior": 3 * k - 6, "non_manifold": 0, "euler": 2}


def test_the_result_need_not_be_a_manifold(femur_meshes, femur_ladders):
    """the femur reference at k = 204: one edge in three triangles — why the caller gets a census"""
    mesh = femur_meshes["reference"]
    ids = femur_ladders["reference"][0][:204]
    tri = LF.dual_triangles(LF.label(mesh.points, mesh.cells, ids)[0], mesh.cells)
    assert LF.edge_census(tri, 204)[2] == 1


def test_open_mesh_census(pkg):
    face = pkg.data.synthetic_face_model(grid=41, rank=1).reference_mesh
    for k, triangles, boundary in ((102, 169, 33), (400, 730, 68)):
        lf = LF.long_form(face.points, face.cells, k)
        b, _, bad, _ = LF.edge_census(lf["cells"], k)
        assert (lf["counts"][1], b, bad) == (triangles, boundary, 0)
    assert pkg.data.mesh_edge_census(face) == {"boundary": 160, "interior": 4720, "non_manifold": 0, "euler": 1}


def test_any_prefix_is_the_decimation_to_that_count(femur_meshes, femur_ladders):
    mesh = femur_meshes["target"]
    ids, cover2 = femur_ladders["target"]
    assert np.all(np.diff(cover2) <= 0) and np.all(np.isfinite(cover2)) and cover2[-1] > 0
    for k in (1, 2, 102, 399):
        small_ids, small_cover2 = LF.select(mesh.points, k)
        assert np.array_equal(small_ids, ids[:k]) and np.array_equal(small_cover2, cover2[:k])
    # cover2[j] is the squared covering radius after j + 1 samples
    for j in (0, 57, 1199):
        d2 = np.min([LF.squared_distances(mesh.points, mesh.points[i]) for i in ids[:j + 1]], axis=0)
        assert d2.max() == cover2[j]


def test_symbol_header_and_signature(pkg):
    nat = pkg._native
    assert hasattr(nat.lib(), "icp_decimate_many")
    header = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    for word in ("icp_decimate_many(", "ICP_DECIMATE_MAX_POINTS 65535", "ICP_DECIMATE_ROUND_BYTES", "EQUAL\n *               VALUES GO TO THE LOWEST ID",
                 "ANY PREFIX OF ids", "VTK's quadric decimation", "No floating-point\n * atomics"):
        assert word in header, word
    res, args = nat.SIGNATURES["icp_decimate_many"]
    # (the entry point's declaration has 15 parameters, n_items .. status)
    assert res is ctypes.c_int and len(args) == 15 and args[1] is ctypes.c_int
    for fn in (pkg.decimated_meshes, pkg.decimated_mesh, pkg.data.decimate, pkg.data.mesh_edge_census, pkg.data.StatisticalMeshModel.decimate):
        assert callable(fn)


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def test_decimated_meshes_validates_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    Mesh = pkg.data.TriangleMesh
    pts, cells = LF.lattice(9)
    mesh = Mesh(pts, cells)

    def moved(value):
        p = pts.copy()
        p[3, 1] = value
        return Mesh(p, cells)

    bad_cells, neg_cells = cells.copy(), cells.copy()
    bad_cells[0, 1], neg_cells[1, 2] = 9, -1
    bad = [dict(meshes=[], counts=3), dict(meshes=[Mesh(np.zeros((0, 3)), np.zeros((0, 3)))], counts=3),   # no item; M = 0
           dict(meshes=[pts], counts=3),                                                                    # not a TriangleMesh
           dict(meshes=[mesh], counts=0), dict(meshes=[mesh], counts=-1), dict(meshes=[mesh], counts=65536), dict(meshes=[mesh], counts=2.0),
           dict(meshes=[mesh], counts=True), dict(meshes=[mesh], counts=None),
           dict(meshes=[mesh], counts=3, starts=-1), dict(meshes=[mesh], counts=3, starts=9), dict(meshes=[mesh], counts=3, starts=1.0),
           dict(meshes=[moved(np.inf)], counts=3), dict(meshes=[moved(np.nan)], counts=3), dict(meshes=[moved(-2.0 ** 61)], counts=3),
           dict(meshes=[Mesh(pts, bad_cells)], counts=3), dict(meshes=[Mesh(pts, neg_cells)], counts=3),
           dict(meshes=[mesh, mesh], counts=[3]), dict(meshes=[mesh, mesh], counts=3, starts=[0, 1, 2]),
           dict(meshes=[mesh], counts=3, want=("ids", "nonsense")), dict(meshes=[mesh], counts=3, want=())]
    for kw in bad:
        with pytest.raises(ValueError):
            pkg.decimated_meshes(**kw)
    good = [dict(meshes=mesh, counts=3), dict(meshes=[mesh, mesh], counts=[1, 65535], starts=[8, 0]), dict(meshes=[mesh, mesh], counts=4, starts=2),
            dict(meshes=[moved(2.0 ** 60)], counts=np.int32(100)), dict(meshes=[Mesh(pts, np.zeros((0, 3)))], counts=3, want=("ids",))]
    for kw in good:
        with pytest.raises(AssertionError, match="icp_decimate_many reached"):
            pkg.decimated_meshes(**kw)
    with pytest.raises(AssertionError, match="icp_decimate_many reached"):
        pkg.decimated_mesh(mesh, 3, start=1)
    with pytest.raises(AssertionError, match="icp_decimate_many reached"):
        pkg.data.decimate(mesh, 3)


CANARY = 7.0


def _native_call(pkg, n_items=2, M=None, T=None, points=None, cells=None, k=4, start=0, status=True, starts_null=False, outputs=True):
    """the same item n_items times, straight through ctypes, every output canary-filled -> (rc, status, the output arrays)"""
    nat, lib = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    pts0, cells0 = LF.lattice(9)
    pts = np.ascontiguousarray(pts0 if points is None else points, dtype=np.float64)
    cl = np.ascontiguousarray(cells0 if cells is None else cells, dtype=np.int32)
    n = max(n_items, 1)
    i32 = lambda v: np.full(n, v, dtype=np.int32)  # noqa: E731
    n_pts, n_tri, ks, ss = i32(pts.shape[0] if M is None else M), i32(cl.shape[0] if T is None else T), i32(k), i32(start)
    outs = {"ids": np.full(9, 7, dtype=np.int32), "points": np.full((9, 3), CANARY), "cover2": np.full(9, CANARY),
            "labels": np.full(9, 7, dtype=np.int32), "cells": np.full((8, 3), 7, dtype=np.int32), "counts": np.full(3 * n, 7, dtype=np.int32)}
    st = np.full(n, 99, dtype=np.int32)
    rep = lambda a, t: (t * n)(*[a.ctypes.data_as(t)] * n) if outputs else None  # noqa: E731
    rc = lib.icp_decimate_many(n_items, 0, n_pts.ctypes.data_as(ip), (dp * n)(*[pts.ctypes.data_as(dp)] * n), n_tri.ctypes.data_as(ip),
                               (ip * n)(*[cl.ctypes.data_as(ip)] * n), ks.ctypes.data_as(ip), None if starts_null else ss.ctypes.data_as(ip),
                               outs["counts"].ctypes.data_as(ip) if outputs else None, rep(outs["ids"], ip), rep(outs["points"], dp),
                               rep(outs["cover2"], dp), rep(outs["labels"], ip), rep(outs["cells"], ip), st.ctypes.data_as(ip) if status else None)
    return rc, st, outs


def _untouched(outs):
    return all(np.all(a == 7) for a in outs.values())


def test_the_library_refuses_bad_arguments_before_touching_a_device(pkg):
    """ICP_ERR_INVALID_ARG for every item, nothing written — also on a machine without a GPU, where touching the device would be
    ICP_ERR_DEVICE instead"""
    pts, cells = LF.lattice(9)

    def moved(value, i=5, j=1):
        p = pts.copy()
        p[i, j] = value
        return p

    def tri(value):
        c = cells.copy()
        c[3, 2] = value
        return c

    cases = [dict(points=moved(np.inf)), dict(points=moved(-np.inf)), dict(points=moved(np.nan)), dict(points=moved(2.0 ** 61)),
             dict(points=moved(-2.0 ** 60 * (1 + 2.0 ** -52), 8, 2)),
             dict(cells=tri(9)), dict(cells=tri(-1)),
             dict(M=0), dict(M=-1), dict(M=(1 << 24) + 1), dict(T=-1), dict(T=(1 << 26) + 1),
             dict(k=0), dict(k=-4), dict(k=65536), dict(start=-1), dict(start=9), dict(start=2 ** 31 - 1)]
    for kw in cases:
        rc, st, outs = _native_call(pkg, **kw)
        assert rc == -1 and np.all(st == -1), kw
        assert _untouched(outs), kw
    assert b"outside the limits" in pkg._native.lib().icp_last_error()
    for kw in (dict(n_items=0), dict(n_items=-3), dict(n_items=65536), dict(status=False), dict(outputs=False)):
        rc, st, outs = _native_call(pkg, **kw)
        assert rc == -1 and np.all(st == 99) and _untouched(outs), kw
    assert b"null argument" in pkg._native.lib().icp_last_error()
