"""GPU: mesh decimation (icp_decimate_many, api.decimated_meshes, data.decimate, StatisticalMeshModel.decimate) — every comparison is
bit equality (doubles viewed as uint64) against the numpy long form (tests/decimation_long_form.py).

The ladder's device results come from ONE decimated_meshes call (every vertex count, sample count and start side by side); the long
forms are made once per item and shared."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import decimation_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "icp-proposal_amd", "csrc")


def source_constant(name, file):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, file)).read())
    assert m, (name, file)
    return int(m.group(1))


# the sizes the kernels define: threads of the per-element launches (= vertices of one selection partial), threads of the one-workgroup
# selection, the vertices it holds, triangles of a tile of the prefix sums
BLOCK, GROUP_THREADS, GROUP_VERTICES, TILE = (source_constant(n, "icp_kernels.hpp") for n in ("kDecBlock", "kDecGroupThreads", "kDecGroupVertices", "kScanTile"))
LADDER = tuple(sorted({1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025} | {e + d for e in (BLOCK, GROUP_THREADS, GROUP_VERTICES, TILE) for d in (-1, 0, 1)}))
FULL_COUNTS_UP_TO = 1025  # every k of {1, 2, M − 1, M, M + 5} up to here; above, the long form's k·M selection decides the counts


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def make(points, cells, k, start=0):
    return dict(points=np.ascontiguousarray(points, dtype=np.float64), cells=np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3), k=int(k),
                start=int(start))


def ladder_items():
    """the exact lattice (ties in the selection at every step, in the sweeps at every vertex) at every M of the ladder, with the counts
    1, 2, M − 1, M, M + 5 and a start that is not 0"""
    items = []
    for M in LADDER:
        pts, cells = LF.lattice(M, spacing=4.0)
        if M <= FULL_COUNTS_UP_TO:
            ks = sorted({k for k in (1, 2, M - 1, M, M + 5) if k >= 1})
        else:
            ks = [1, 2, 37] + ([M + 5] if M in (GROUP_VERTICES, GROUP_VERTICES + 1) else [])
        for n, k in enumerate(ks):
            items.append(make(pts, cells, k, (M // 3) if n % 2 else 0))
    # the tile of the triangles' prefix sums: one below, at and one above it, and two tiles and one
    pts, cells = LF.lattice(2300, spacing=4.0)
    for T in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        items.append(make(pts, cells[:T], 300, 11))
    return items


@functools.lru_cache(maxsize=None)
def _ladder():
    return ladder_items()


def long_form_of(it):
    return LF.long_form(it["points"], it["cells"], it["k"], it["start"])


def assert_item(got, lf, what):
    assert got["counts"] == lf["counts"], (what, got["counts"], lf["counts"])
    for name in ("ids", "points", "cover2", "labels", "cells"):
        assert same(got[name], lf[name]), (what, name)


def run(pkg, items, **kw):
    Mesh = pkg.data.TriangleMesh
    return pkg.decimated_meshes([Mesh(i["points"], i["cells"]) for i in items], [i["k"] for i in items], [i["start"] for i in items], **kw)


@pytest.mark.gpu
def test_count_ladder_against_the_long_form(pkg):
    items = _ladder()
    got = run(pkg, items)
    assert len(got) == len(items)
    tied = 0
    for it, g in zip(items, got):
        lf = long_form_of(it)
        assert_item(g, lf, (it["points"].shape[0], it["k"], it["start"]))
        tied += int(lf["cover2"].shape[0] > 2 and np.any(np.diff(lf["cover2"]) == 0))
    assert tied >= len(LADDER)  # equal maxima met in the selection of most items: the lowest ids took the places


@pytest.mark.gpu
def test_the_femur_on_the_device(pkg):
    """the femur reference and the aligned target at k = 102, 400 and 1,200, and the jittered target: the long form's bits; closed
    manifolds with T = 2k − 4; any prefix of the ids is the decimation to that count"""
    reference, _, _ = pkg.data.load_femur_mesh("femur_reference")
    _, target = pkg.data.load_femur_model_and_target(50)
    rng = np.random.default_rng(11)
    jittered = target.points + rng.normal(0.0, 0.05, size=target.points.shape)
    items = [make(m.points, m.cells, k) for m in (reference, target) for k in (102, 400, 1200)]
    items += [make(jittered, target.cells, 400, 1000), make(reference.points, reference.cells, 204)]
    got = run(pkg, items)
    for q, (it, g) in enumerate(zip(items, got)):
        lf = long_form_of(it)
        assert_item(g, lf, ("femur", q))
    for q in range(6):
        k = items[q]["k"]
        assert got[q]["counts"][:2] == (k, 2 * k - 4)
        census = pkg.data.mesh_edge_census(pkg.data.TriangleMesh(got[q]["points"], got[q]["cells"]))
        assert census == {"boundary": 0, "interior": 3 * k - 6, "non_manifold": 0, "euler": 2}
    for base in (0, 3):
        for q in (base, base + 1):
            k = items[q]["k"]
            assert same(got[q]["ids"], got[base + 2]["ids"][:k]) and same(got[q]["cover2"], got[base + 2]["cover2"][:k])
    assert pkg.data.mesh_edge_census(pkg.data.TriangleMesh(got[7]["points"], got[7]["cells"]))["non_manifold"] == 1


@pytest.mark.gpu
def test_the_subdivided_target_at_1200(pkg):
    _, big = pkg.data.synthetic_femur_target()
    assert big.n_points == 58322
    it = make(big.points, big.cells, 1200)
    got = run(pkg, [it])[0]
    assert_item(got, long_form_of(it), "58,322 vertices")
    assert got["counts"][:2] == (1200, 2396)
    assert pkg.data.mesh_edge_census(pkg.data.TriangleMesh(got["points"], got["cells"])) == {"boundary": 0, "interior": 3594, "non_manifold": 0,
                                                                                           "euler": 2}


@pytest.mark.gpu
def test_a_carry_of_the_tile_totals(pkg):
    """more than kDecBlock tiles of triangles (the scan of the tile totals walks them kDecBlock at a time): the 32 × 32 lattice's
    triangles over and over — duplicates of the first copy —, then every one of them flipped — other triples, kept, behind the carry"""
    pts, cells = LF.lattice(1024, spacing=4.0)
    copies = -(-(BLOCK * TILE + 1) // cells.shape[0])
    it = make(pts, np.concatenate([np.tile(cells, (copies, 1)), cells[:, ::-1]]), 256, 5)
    assert it["cells"].shape[0] > BLOCK * TILE + cells.shape[0]
    got = run(pkg, [it])[0]
    lf = long_form_of(it)
    assert_item(got, lf, "carry")
    once = LF.dual_triangles(lf["labels"], cells)
    assert same(got["cells"][:once.shape[0]], once) and got["counts"][1] > once.shape[0]  # the rows behind: flipped triangles, past the carry


# ---------------------------------------------------------------- straight through the C ABI: NULL outputs, canaries

OUTPUTS = ("ids", "points", "cover2", "labels", "cells")
CANARY = -12345.0


def raw_call(pkg, items, nulls=None, counts_null=False):
    """items through icp_decimate_many with caller-sized, canary-filled arrays; nulls[b]: names of the outputs item b passes as NULL
    -> one dict per item: the arrays as the call left them, "counts", "status" """
    nat, lib = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    n = len(items)
    nulls = nulls or [()] * n
    i32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    n_pts, n_tri = i32([i["points"].shape[0] for i in items]), i32([i["cells"].shape[0] for i in items])
    ks, ss = i32([i["k"] for i in items]), i32([i["start"] for i in items])
    out = []
    for b, i in enumerate(items):
        M, T, k = int(n_pts[b]), int(n_tri[b]), i["k"]
        out.append({"ids": np.full(k, -7, dtype=np.int32), "points": np.full((k, 3), CANARY), "cover2": np.full(k, CANARY),
                    "labels": np.full(M, -7, dtype=np.int32), "cells": np.full((T, 3), -7, dtype=np.int32)})
    ptrs = lambda arrays, t: (t * n)(*[None if a is None else a.ctypes.data_as(t) for a in arrays])  # noqa: E731
    given = lambda name: [None if name in nulls[b] else out[b][name] for b in range(n)]  # noqa: E731
    counts = np.full(3 * n, -7, dtype=np.int32)
    status = np.full(n, 99, dtype=np.int32)
    rc = lib.icp_decimate_many(n, 0, n_pts.ctypes.data_as(ip), ptrs([i["points"] for i in items], dp), n_tri.ctypes.data_as(ip),
                               ptrs([i["cells"] for i in items], ip), ks.ctypes.data_as(ip), ss.ctypes.data_as(ip),
                               None if counts_null else counts.ctypes.data_as(ip), ptrs(given("ids"), ip), ptrs(given("points"), dp),
                               ptrs(given("cover2"), dp), ptrs(given("labels"), ip), ptrs(given("cells"), ip), status.ctypes.data_as(ip))
    assert rc == 0, (rc, lib.icp_last_error())
    for b in range(n):
        out[b]["counts"], out[b]["status"] = tuple(int(x) for x in counts[3 * b:3 * b + 3]), int(status[b])
        for name in nulls[b]:
            out[b][name] = None
    return out


def assert_raw(got, lf, what, counts=True):
    """the rows the counts name are the long form's, the rows behind them keep their canary"""
    assert got["status"] == 0, what
    if counts:
        assert got["counts"] == lf["counts"], (what, got["counts"], lf["counts"])
    ke, to, _ = lf["counts"]
    if got["ids"] is not None:
        assert same(got["ids"][:ke], lf["ids"]) and np.all(got["ids"][ke:] == -7), (what, "ids")
    if got["points"] is not None:
        assert same(got["points"][:ke], lf["points"]) and np.all(got["points"][ke:] == CANARY), (what, "points")
    if got["cover2"] is not None:
        assert same(got["cover2"][:ke], lf["cover2"]) and np.all(got["cover2"][ke:] == CANARY), (what, "cover2")
    if got["labels"] is not None:
        assert same(got["labels"], lf["labels"]), (what, "labels")
    if got["cells"] is not None:
        assert same(got["cells"][:to], lf["cells"]) and np.all(got["cells"][to:] == -7), (what, "cells")


def edge_items(pkg):
    lat, lat_cells = LF.lattice(300, spacing=4.0)
    face = pkg.data.synthetic_face_model(grid=41, rank=1).reference_mesh
    x = np.repeat(np.arange(4.0), 3)
    repeated = np.stack([x, 0 * x, 0 * x], axis=1)
    far = lat + [0.0, 0.0, 500.0]
    two = np.concatenate([lat, far]), np.concatenate([lat_cells, lat_cells + 300])
    loose = np.concatenate([lat, [[-9.0, -9.0, 3.0], [2000.0, 2.0, 1.0], [4.0, 4.0, 0.25]]])
    messy = np.concatenate([lat_cells, lat_cells[::3], lat_cells[::5, ::-1], [[5, 5, 6], [9, 9, 9]], lat_cells[:40, [1, 2, 0]]])
    return [make(repeated, np.zeros((0, 3)), 10),                           # four distinct points three times each: the early stop; T = 0
            make(np.repeat(lat, 2, axis=0), np.repeat(lat_cells, 1, axis=0) * 2, 700, 3),   # every point twice, one copy meshed: k_eff = 300
            make(face.points, face.cells, 102), make(face.points, face.cells, 400),        # an open mesh
            make(two[0], two[1], 1, 17), make(two[0], two[1], 2), make(two[0], two[1], 60, 450),   # two components: labels −1 with k = 1
            make(loose, lat_cells, 50), make(loose, lat_cells, 303),        # loose vertices: samples that no triangle uses, labels −1
            make(lat, np.zeros((0, 3)), 25, 299),                           # T = 0
            make(lat, messy, 40, 1),                                        # repeats, both orientations, rotations, degenerate triangles
            make(lat[:1], np.zeros((0, 3)), 3), make(lat[:3], [[0, 1, 2]], 3), make(lat[:3], [[0, 1, 2]], 2, 2)]


@pytest.mark.gpu
def test_edge_cases_and_canaries(pkg):
    items = edge_items(pkg)
    got = raw_call(pkg, items)
    lfs = [long_form_of(it) for it in items]
    for b, (g, lf) in enumerate(zip(got, lfs)):
        assert_raw(g, lf, b)
    assert got[0]["counts"] == (4, 0, 0) and got[0]["ids"][:4].tolist() == [0, 9, 3, 6] and got[0]["cover2"][3] == 0.0
    assert got[1]["counts"][0] == 300 and got[1]["cover2"][299] == 0.0
    face_census = [LF.edge_census(got[q]["cells"][:got[q]["counts"][1]], items[q]["k"]) for q in (2, 3)]
    assert [(got[q]["counts"][1],) + c[:1] + c[2:3] for q, c in zip((2, 3), face_census)] == [(169, 33, 0), (730, 68, 0)]
    assert (got[4]["labels"] == -1).sum() == 300 and got[4]["labels"][17] == 0 and got[4]["counts"][1] == 0
    assert (got[5]["labels"] == -1).sum() == 0  # (the second sample is the farthest vertex: in the other component)
    assert got[7]["labels"][302] == -1 and np.all(got[8]["labels"][300:] >= 0)  # (a quarter above a lattice vertex: among the last samples)
    assert got[9]["counts"][1:] == (0, 0) and (got[9]["labels"] >= 0).sum() == 25
    assert got[11]["counts"] == (1, 0, 0) and got[12]["counts"] == (3, 1, 0) and got[12]["cells"][0].tolist() == [0, 2, 1]
    # NULL outputs: what is asked for is the same whatever else is; without counts, labels and cells the sweeps are skipped altogether
    names = set(OUTPUTS)
    for nulls, counts_null in (([("ids",)] * len(items), False), ([("labels", "cells")] * len(items), True),
                               ([tuple(names - {"labels"})] * len(items), True), ([tuple(names - {"cells"})] * len(items), True),
                               ([tuple(names - {OUTPUTS[b % 5]}) for b in range(len(items))], True), ([tuple(names)] * len(items), False)):
        again = raw_call(pkg, items, nulls, counts_null)
        for b, (a, lf) in enumerate(zip(again, lfs)):
            assert_raw(a, lf, ("nulls", nulls[b], b), counts=not counts_null)
            assert counts_null == (a["counts"] == (-7, -7, -7))


@pytest.mark.gpu
def test_decimated_points_in_an_evaluator_and_a_decimated_model(pkg, femur50):
    model, target = femur50
    dec = pkg.data.decimate(target, 400)
    lf = LF.long_form(target.points, target.cells, 400)
    assert same(dec.points, lf["points"]) and same(dec.cells, lf["cells"])
    ctx = pkg.IcpContext(model, target, device=0)
    theta = pkg.initial_parameters(model)
    values = []
    for tp in (dec.points, lf["points"]):
        ev = pkg.CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator(ctx, 0.0, 2.0, 1.0, pkg.SymmetricEvaluation, 400, decimatedTargetPoints=tp)
        values.append(ev.logValue(theta))
        ev.close()
    ctx.close()
    assert np.isfinite(values[0]) and values[0] == values[1]
    small = model.decimate(300, start=5)
    ref = LF.long_form(model.ref_points, model.cells, 300, 5)
    ids = ref["ids"].astype(np.int64)
    assert same(small.ref_points, ref["points"]) and same(small.cells, ref["cells"]) and same(small.variance, model.variance)
    assert same(small.mean_def, model.mean_def[ids]) and same(small.basis, model.basis.reshape(-1, 3, model.rank)[ids].reshape(-1, model.rank))
    c = np.linspace(-1.0, 1.0, model.rank)
    assert same(small.instance(c), small.instance(c)) and np.abs(small.instance(c) - model.instance(c)[ids]).max() <= 1e-9


# ---------------------------------------------------------------- determinism: alone, mixed, reversed, small rounds, both routes

def mixed_items(pkg):
    """different M, T and k, both selection routes at the default threshold; MIXED_NULLS: some output pointers NULL"""
    edge = edge_items(pkg)
    big, big_cells = LF.lattice(GROUP_VERTICES + 1, spacing=4.0)
    rng = np.random.default_rng(3)
    jitter, jitter_cells = LF.lattice(2049)
    return [make(big, big_cells, 130, 77), edge[10], make(jitter + rng.normal(0.0, 0.2, size=jitter.shape), jitter_cells, 500, 2048), edge[1], edge[6],
            edge[11]]


MIXED_NULLS = [(), ("ids",), ("labels", "cover2"), ("cells",), (), ("points", "cells", "labels")]


def same_item(a, b):
    return a["counts"] == b["counts"] and all(a[k] is None or b[k] is None or same(a[k], b[k]) for k in OUTPUTS)


def chunk_check():
    """one item alone == the same item inside a call of 6 mixed items == that call reversed == with the round's buffer forced to the
    smallest allowed (every item a round of its own) and to a size a few small items share == with sweep groups of one == with the
    general selection forced on every item == with the one-workgroup selection's limit moved: every output array equal as bits, and
    the rows behind the counts keep their canaries"""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    hooks = ("ICP_TEST_DECIMATE_CHUNK_DOUBLES", "ICP_TEST_DECIMATE_GROUP_VERTICES", "ICP_TEST_DECIMATE_SWEEP_GROUP")
    for h in hooks:
        os.environ.pop(h, None)
    items = mixed_items(pkg)
    lfs = [long_form_of(it) for it in items]
    whole = raw_call(pkg, items, MIXED_NULLS)
    for q, it in enumerate(items):
        assert_raw(whole[q], lfs[q], ("mixed", q))
        assert same_item(raw_call(pkg, [it])[0], whole[q]), ("alone", q)
    rev = raw_call(pkg, items[::-1], MIXED_NULLS[::-1])[::-1]
    assert all(same_item(a, b) for a, b in zip(whole, rev)), "reversed"
    ladder = [it for it in ladder_items() if it["points"].shape[0] in (1, 3, BLOCK - 1, BLOCK, BLOCK + 1, 1025)]
    ladder_lfs = [long_form_of(it) for it in ladder]
    for env in ({hooks[0]: "1"}, {hooks[0]: "60000"}, {hooks[2]: "1"}, {hooks[1]: "0"}, {hooks[1]: "300"}, {hooks[1]: "0", hooks[2]: "1", hooks[0]: "60000"}):
        os.environ.update(env)
        other = raw_call(pkg, items, MIXED_NULLS)
        assert all(same_item(a, b) for a, b in zip(whole, other)), env
        for q in range(len(items)):
            assert_raw(other[q], lfs[q], (env, q))
        if hooks[1] in env:  # the ladder's small sizes through the general selection
            for q, g in enumerate(raw_call(pkg, ladder)):
                assert_raw(g, ladder_lfs[q], (env, "ladder", q))
        for h in env:
            os.environ.pop(h)
    print("chunk check ok")


@pytest.mark.gpu
def test_an_items_bits_do_not_depend_on_the_batch_the_rounds_or_the_route():
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=300,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "chunk check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    chunk_check()
