"""GPU: aligned and partial targets from raw scans (icp_scans_prepare_many, api.prepare_scans, data.aligned_and_partial_targets) —
every comparison is bit equality (doubles viewed as uint64) against the numpy long form (tests/scan_preparation_long_form.py).

The ladder's device results come from ONE prepare_scans call (every count, cut and transform side by side); the long forms are made
once per item and shared."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scan_preparation_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "icp-proposal_amd", "csrc")


def source_constant(name, file):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, file)).read())
    assert m, (name, file)
    return int(m.group(1))


# the block and tile sizes the kernels define: threads of the per-element launches, threads of the selection's workgroup, elements of
# a tile of the prefix sums (two tiles: 4,096 | 4,097 is in the list already)
EDGES = (source_constant("kScanBlock", "kernels_scan_prep.hip"), source_constant("kScanSelBlock", "kernels_scan_prep.hip"),
         source_constant("kScanTile", "icp_kernels.hpp"))
LADDER = tuple(sorted({1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097} | {e + d for e in EDGES for d in (-1, 0, 1)}))
# the scan of the tile totals walks them kScanBlock at a time: one count past kScanBlock tiles (a carry between two chunks)
LARGE = EDGES[0] * EDGES[2] + 1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def general_transform(pkg):
    """s = 1/1000, a Kabsch rotation, c != 0"""
    a, b = LF.kabsch_rotation()
    rot, t = pkg.data.rigid_landmark_transform(a, b)
    return pkg.data.ScanTransform(1.0 / 1000.0, rot, [0.25, -1.5, 2.0], t)


def exact_transform(pkg):
    """no rounding anywhere on a lattice of multiples of 4: s = 1/2, a quarter turn, integer c and t — every tie of the lattice stays"""
    return pkg.data.ScanTransform(0.5, [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], [1.0, 2.0, 3.0], [-7.0, 4.0, 11.0])


def tie_count(d2):
    """a count that splits the tie class nearest the middle of the sorted distances (None: no two are equal)"""
    s = np.sort(d2)
    eq = np.flatnonzero(s[1:] == s[:-1])  # s[i] == s[i + 1]: a count of i + 1 takes one of the two
    if eq.size == 0:
        return None
    return int(eq[np.argmin(np.abs(eq - s.shape[0] // 2))]) + 1


def ladder_items(pkg):
    """per M and transform: the counts 0, 1, M − 1, M, M + 5 and one in the middle of a tie class, two cuts at once around landmarks
    0 (the scan's middle vertex) and 1 (its vertex 0), a mask list with a repeat and ids >= M"""
    items = []
    for M in LADDER + (LARGE,):
        pts, cells = LF.lattice(M, spacing=4.0)
        lms = np.stack([pts[M // 2], pts[0], pts[M - 1] + 1.0])
        mask = np.array([M // 3, M // 3, M + 2, 10 ** 9, (2 * M) // 3], dtype=np.int64)
        for kind, tf in (("general", general_transform(pkg)), ("exact", exact_transform(pkg))):
            if M == LARGE and kind == "general":
                continue
            al = LF.transform(pts, tf.pre_scale, tf.rotation, tf.centre, tf.translation)
            z = LF.transform(lms, tf.pre_scale, tf.rotation, tf.centre, tf.translation)
            tie = tie_count(LF.squared_distances(al, z[0]))
            if kind == "exact" and M >= 4:
                assert tie is not None, M
            counts = [0, 1, M - 1, M, M + 5, tie if tie is not None else M // 2]
            if M == LARGE:
                counts = [tie]
            for k, c in enumerate(counts):
                items.append(dict(M=M, kind=kind, points=pts, cells=cells, tf=tf, landmarks=lms, cuts=[(0, c), (1, counts[(k + 2) % len(counts)])],
                                  mask=mask))
    return items


def long_form_of(it):
    tf = it["tf"]
    return LF.long_form(it["points"], it["cells"], tf.pre_scale, tf.rotation, tf.centre, tf.translation, it["landmarks"], it["cuts"], it["mask"])


def assert_item(got, lf, what):
    assert same(got["aligned"].points, lf["aligned"]), (what, "aligned")
    assert same(got["landmarks"], lf["landmarks"]), (what, "landmarks")
    assert same(got["cut_flags"], lf["cut_flags"]), (what, "cut_flags", np.flatnonzero(got["cut_flags"] != lf["cut_flags"])[:8])
    assert same(got["kept_ids"], lf["kept_ids"]), (what, "kept_ids")
    assert same(got["partial"].points, lf["partial_points"]), (what, "partial points")
    assert same(got["partial"].cells, lf["partial_cells"]), (what, "partial cells")


@pytest.mark.gpu
def test_count_ladder_against_the_long_form(pkg):
    items = ladder_items(pkg)
    Mesh = pkg.data.TriangleMesh
    got = pkg.prepare_scans([Mesh(i["points"], i["cells"]) for i in items], [i["tf"] for i in items], [i["landmarks"] for i in items],
                            [i["cuts"] for i in items], [i["mask"] for i in items])
    assert len(got) == len(items)
    tied = 0
    for it, g in zip(items, got):
        lf = long_form_of(it)
        assert_item(g, lf, (it["M"], it["kind"], it["cuts"]))
        d2 = np.sort(LF.squared_distances(lf["aligned"], lf["landmarks"][0]))
        c = it["cuts"][0][1]
        tied += int(0 < c < it["M"] and d2[c - 1] == d2[c])
    assert tied >= len(LADDER) - 3  # the threshold fell inside a tie class at (nearly) every count: the lowest ids took the places


@pytest.mark.gpu
def test_the_references_shape_is_a_usable_target(pkg, femur50):
    """apps/bfm/AlignShapes.scala:88-92 on a face-sized patch: 1,000 vertices around the highest one cut away"""
    face = pkg.data.synthetic_face_model(grid=41, rank=1)
    rng = np.random.default_rng(41)
    pts = face.ref_points + rng.normal(0.0, 0.02, size=face.ref_points.shape)  # (no ties)
    assert pts.shape == (1681, 3)
    tip = int(np.argmax(pts[:, 2]))
    # the patch stood up along the femur's length, twice its size, centred on the femur: a third of the femur's vertices then have an
    # interior vertex of the patch's remaining frame nearest (the boundary-aware evaluator drops the others)
    model, _ = femur50
    rot = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    t = (model.ref_points + model.mean_def).mean(axis=0) - LF.transform(pts, 2.0, rot).mean(axis=0)
    tf = pkg.data.ScanTransform(2.0, rot, np.zeros(3), t)
    got = pkg.prepare_scans(pkg.data.TriangleMesh(pts, face.cells), tf, pts[tip:tip + 1].copy(), [(0, 1000)])[0]
    lf = LF.long_form(pts, face.cells, 2.0, rot, None, t, landmarks=pts[tip:tip + 1], cuts=[(0, 1000)])
    assert_item(got, lf, "face")
    assert int((got["cut_flags"] == 1).sum()) == 1000 and got["partial"].n_points < 681 + 1 and got["partial"].n_cells > 0
    flags = pkg.data.boundary_vertex_flags(got["partial"])
    rim = np.zeros((41, 41), dtype=bool)
    rim[0, :] = rim[-1, :] = rim[:, 0] = rim[:, -1] = True
    inner = flags.astype(bool) & ~rim.ravel()[got["kept_ids"]]
    assert inner.sum() > 0  # an inner boundary, around the hole
    ctx = pkg.IcpContext(model, got["partial"], device=0)
    ev = pkg.CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator(ctx, 0.0, 2.0, 1.0, pkg.SymmetricEvaluation, 200)
    value = ev.logValue(pkg.initial_parameters(model))
    ev.close()
    ctx.close()
    assert np.isfinite(value)


# ---------------------------------------------------------------- straight through the C ABI: NULL outputs, canaries

OUTPUTS = ("aligned", "landmarks", "cut_flags", "partial_points", "partial_cells", "kept_ids")
CANARY = -12345.0


def raw_call(pkg, items, nulls=None, counts_null=False):
    """items through icp_scans_prepare_many with caller-sized, canary-filled arrays; nulls[b]: names of the outputs item b passes as
    NULL -> one dict per item: the arrays as the call left them, "counts", "status" """
    nat, lib = pkg._native, pkg._native.lib()
    dp, ip, up = nat.c_double_p, nat.c_int_p, nat.c_ubyte_p
    n = len(items)
    nulls = nulls or [()] * n
    hold = []

    def keep(a):
        hold.append(a)
        return a

    pts = [keep(np.ascontiguousarray(i["points"], dtype=np.float64)) for i in items]
    cells = [keep(np.ascontiguousarray(i["cells"], dtype=np.int32).reshape(-1, 3)) for i in items]
    lms = [keep(np.ascontiguousarray(i["landmarks"] if i["landmarks"] is not None else np.zeros((0, 3)), dtype=np.float64).reshape(-1, 3)) for i in items]
    cl = [keep(np.array([c[0] for c in i["cuts"]], dtype=np.int32)) for i in items]
    cc = [keep(np.array([c[1] for c in i["cuts"]], dtype=np.int32)) for i in items]
    mk = [keep(np.ascontiguousarray(i["mask"], dtype=np.int32).reshape(-1)) for i in items]
    tfs = (nat.ScanTransform * n)()
    for b, i in enumerate(items):
        tf = i["tf"]
        tfs[b].struct_size, tfs[b].pre_scale = ctypes.sizeof(nat.ScanTransform), tf.pre_scale
        tfs[b].rotation[:] = tf.rotation.reshape(-1).tolist()
        tfs[b].centre[:] = tf.centre.tolist()
        tfs[b].translation[:] = tf.translation.tolist()
    i32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    n_pts, n_tri, n_lm = i32([p.shape[0] for p in pts]), i32([c.shape[0] for c in cells]), i32([a.shape[0] for a in lms])
    n_ct, n_mk = i32([a.shape[0] for a in cl]), i32([a.shape[0] for a in mk])
    out = []
    for b in range(n):
        M, T, L = int(n_pts[b]), int(n_tri[b]), int(n_lm[b])
        out.append({"aligned": np.full((M, 3), CANARY), "landmarks": np.full((L, 3), CANARY), "cut_flags": np.full(M, 0x55, dtype=np.uint8),
                    "partial_points": np.full((M, 3), CANARY), "partial_cells": np.full((T, 3), -7, dtype=np.int32),
                    "kept_ids": np.full(M, -7, dtype=np.int32)})
    ptrs = lambda arrays, t: (t * n)(*[None if a is None else a.ctypes.data_as(t) for a in arrays])  # noqa: E731
    given = lambda name: [None if name in nulls[b] else out[b][name] for b in range(n)]  # noqa: E731
    counts = np.full(2 * n, -7, dtype=np.int32)
    status = np.full(n, 99, dtype=np.int32)
    rc = lib.icp_scans_prepare_many(n, 0, n_pts.ctypes.data_as(ip), ptrs(pts, dp), n_tri.ctypes.data_as(ip), ptrs(cells, ip), tfs,
                                    n_lm.ctypes.data_as(ip), ptrs(lms, dp), n_ct.ctypes.data_as(ip), ptrs(cl, ip), ptrs(cc, ip),
                                    n_mk.ctypes.data_as(ip), ptrs(mk, ip), ptrs(given("aligned"), dp), ptrs(given("landmarks"), dp),
                                    ptrs(given("cut_flags"), up), ptrs(given("partial_points"), dp), ptrs(given("partial_cells"), ip),
                                    ptrs(given("kept_ids"), ip), None if counts_null else counts.ctypes.data_as(ip), status.ctypes.data_as(ip))
    assert rc == 0, (rc, lib.icp_last_error())
    for b in range(n):
        out[b]["counts"], out[b]["status"] = (int(counts[2 * b]), int(counts[2 * b + 1])), int(status[b])
        for name in nulls[b]:
            out[b][name] = None
    return out


def assert_raw(got, lf, what):
    """the rows the counts name are the long form's, the rows behind them keep their canary"""
    assert got["status"] == 0 and got["counts"] == lf["counts"], (what, got["counts"], lf["counts"])
    nk, tk = lf["counts"]
    for name in ("aligned", "landmarks", "cut_flags"):
        if got[name] is not None:
            assert same(got[name], lf[name]), (what, name)
    if got["partial_points"] is not None:
        assert same(got["partial_points"][:nk], lf["partial_points"]) and np.all(got["partial_points"][nk:] == CANARY), (what, "partial points")
    if got["partial_cells"] is not None:
        assert same(got["partial_cells"][:tk], lf["partial_cells"]) and np.all(got["partial_cells"][tk:] == -7), (what, "partial cells")
    if got["kept_ids"] is not None:
        assert same(got["kept_ids"][:nk], lf["kept_ids"]) and np.all(got["kept_ids"][nk:] == -7), (what, "kept ids")


def item(pkg, M, tf=None, cells=True, landmarks=2, cuts=(), mask=(), jitter=None, extra_vertices=0):
    pts, cl = LF.lattice(M, spacing=4.0)
    if jitter is not None:
        pts = pts + np.random.default_rng(jitter).normal(0.0, 0.3, size=pts.shape)
    if extra_vertices:
        pts = np.concatenate([pts, 4.0 * np.arange(3.0 * extra_vertices).reshape(-1, 3) + 1.0])
    lms = np.stack([pts[M // 2], pts[0], pts[M - 1] + 1.0, pts[M // 3]])[:landmarks] if landmarks else None
    return dict(points=pts, cells=cl if cells else np.zeros((0, 3), dtype=np.int32), tf=tf if tf is not None else general_transform(pkg),
                landmarks=lms, cuts=list(cuts), mask=np.array(mask, dtype=np.int64))


@pytest.mark.gpu
def test_edge_cases_and_canaries(pkg):
    items = [item(pkg, 300, cells=False, cuts=[(0, 40)], mask=[5]),                                  # T = 0
             item(pkg, 257, cuts=[(1, 257)]),                                                          # every vertex cut
             item(pkg, 257, cuts=[(0, 100), (1, 200)], mask=list(range(0, 257, 2))),                   # … by two cuts and the mask together
             item(pkg, 100, cuts=[(0, 7)], extra_vertices=3),                                          # vertices no triangle references
             item(pkg, 100, cuts=[], mask=[100, 101, 10 ** 9, 2 ** 31 - 1]),                           # mask ids >= M alone: nothing is cut
             item(pkg, 100, landmarks=0, cuts=[], mask=[]),                                            # L = 0, n_cuts = 0
             item(pkg, 100, landmarks=0, cuts=[], mask=[3, 3, 50]),
             item(pkg, 1, cuts=[(0, 0)]), item(pkg, 2, cuts=[(0, 1)]),
             item(pkg, 600, tf=exact_transform(pkg), landmarks=4, cuts=[(k % 4, 30 * k) for k in range(7)], mask=[599, 0])]  # seven cuts
    got = raw_call(pkg, items)
    for b, (it, g) in enumerate(zip(items, got)):
        assert_raw(g, long_form_of(it), b)
    assert got[0]["counts"] == (0, 0) and got[1]["counts"] == (0, 0) and got[2]["counts"] == (0, 0)
    assert got[3]["counts"][0] < 100 and not np.any(got[3]["cut_flags"][100:])  # the three loose vertices: not cut, and gone
    assert got[4]["counts"] == (100, len(items[4]["cells"])) and not got[4]["cut_flags"].any()
    assert got[5]["counts"] == (100, len(items[5]["cells"]))
    assert set(np.flatnonzero(got[9]["cut_flags"] & 0x7f)) and np.any(got[9]["cut_flags"] & 0x40)
    again = raw_call(pkg, items[:3], counts_null=True)  # counts_out = NULL: the arrays all the same
    for a, g in zip(again, got):
        assert all(same(a[k], g[k]) for k in OUTPUTS)


@pytest.mark.gpu
def test_aligned_and_partial_targets_on_the_femur_target(pkg):
    _, ref_ids, ref_lms = pkg.data.load_femur_mesh("femur_reference")
    target, tgt_ids, tgt_lms = pkg.data.load_femur_mesh("femur_target")
    scan_lms = dict(zip(tgt_ids, np.asarray(tgt_lms, dtype=np.float64)))
    model_lms = dict(zip(ref_ids, np.asarray(ref_lms, dtype=np.float64)))
    name = tgt_ids[2]
    mask = [10, 11, 12, 1621, 1622, 5000]
    aligned, partial, lms, partial_lms = pkg.data.aligned_and_partial_targets([target, target], [scan_lms, scan_lms], model_lms, cut_landmark=name,
                                                                              cut_count=300, mask_ids=mask, drop_landmarks=(name,))
    tf = pkg.data.landmark_alignment(scan_lms, model_lms)
    lm_in = np.asarray([scan_lms[k] for k in scan_lms])
    lf = LF.long_form(target.points, target.cells, tf.pre_scale, tf.rotation, tf.centre, tf.translation, lm_in, [(2, 300)], mask)
    for b in range(2):
        assert same(aligned[b].points, lf["aligned"]) and same(aligned[b].cells, target.cells)
        assert list(lms[b]) == list(scan_lms) and all(same(lms[b][k], lf["landmarks"][i]) for i, k in enumerate(scan_lms))
        assert list(partial_lms[b]) == [k for k in scan_lms if k != name]
        assert same(partial[b].points, lf["partial_points"]) and same(partial[b].cells, lf["partial_cells"])
    assert 0 < partial[0].n_points <= 1622 - 300
    _, want = pkg.data.load_femur_model_and_target(50)
    assert np.abs(aligned[0].points - want.points).max() <= 1e-12  # load_femur_model_and_target's target, to rounding


# ---------------------------------------------------------------- determinism: alone, mixed, reversed, small rounds

def mixed_items(pkg):
    """different M, T, L and n_cuts; MIXED_NULLS: some output pointers NULL"""
    return [item(pkg, 4097, cuts=[(0, 1000), (1, 37)], mask=[5, 5, 4096, 4097]),
            item(pkg, 257, cells=False, landmarks=1, cuts=[(0, 100)]),
            item(pkg, 1025, landmarks=0, mask=[0, 7, 1024]),
            item(pkg, 65, tf=exact_transform(pkg), landmarks=3, cuts=[(k % 3, 9 * k) for k in range(7)]),
            item(pkg, 2049, cuts=[(1, 1024)], jitter=3, extra_vertices=2),
            item(pkg, 1, landmarks=1, cuts=[(0, 5)])]


MIXED_NULLS = [(), ("aligned",), ("partial_points", "kept_ids"), ("cut_flags", "landmarks"), (), ("partial_points", "partial_cells", "kept_ids")]


def same_item(a, b):
    return a["counts"] == b["counts"] and all(a[k] is None or b[k] is None or same(a[k], b[k]) for k in OUTPUTS)


def chunk_check():
    """one item alone == the same item inside a call of 6 mixed items == that call reversed == with the round's buffer forced to the
    smallest allowed (every item a round of its own) and to about a ninth of the largest item (the small items share rounds) == with
    the array-by-array copies of large items forced on the small ones: every output array equal as bits, and the rows behind the counts
    keep their canaries whichever way the copies go"""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    os.environ.pop("ICP_TEST_SCAN_PREP_CHUNK_DOUBLES", None)
    items = mixed_items(pkg)
    whole = raw_call(pkg, items, MIXED_NULLS)
    for q, it in enumerate(items):
        assert_raw(whole[q], long_form_of(it), ("mixed", q))
        assert same_item(raw_call(pkg, [it])[0], whole[q]), ("alone", q)
    rev = raw_call(pkg, items[::-1], MIXED_NULLS[::-1])[::-1]
    assert all(same_item(a, b) for a, b in zip(whole, rev)), "reversed"
    for doubles in (1, 10000):
        os.environ["ICP_TEST_SCAN_PREP_CHUNK_DOUBLES"] = str(doubles)
        small = raw_call(pkg, items, MIXED_NULLS)
        assert all(same_item(a, b) for a, b in zip(whole, small)), doubles
        for q, it in enumerate(items):
            assert_raw(small[q], long_form_of(it), ("small rounds", doubles, q))
    os.environ["ICP_TEST_SCAN_PREP_DIRECT_COPIES"] = "1"  # the copies of large items (array by array), at the last forced size too
    for doubles in (None, 10000):
        if doubles is None:
            os.environ.pop("ICP_TEST_SCAN_PREP_CHUNK_DOUBLES", None)
        direct = raw_call(pkg, items, MIXED_NULLS)
        assert all(same_item(a, b) for a, b in zip(whole, direct)), ("direct copies", doubles)
        os.environ["ICP_TEST_SCAN_PREP_CHUNK_DOUBLES"] = "10000"
    os.environ.pop("ICP_TEST_SCAN_PREP_DIRECT_COPIES", None)
    os.environ.pop("ICP_TEST_SCAN_PREP_CHUNK_DOUBLES", None)
    print("chunk check ok")


@pytest.mark.gpu
def test_an_items_bits_do_not_depend_on_the_batch_or_the_rounds():
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=300,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "chunk check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    chunk_check()
