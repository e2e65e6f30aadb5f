"""CPU: target preparation (icp_scans_prepare_many, api.prepare_scans, data.landmark_alignment) — the numpy long form the GPU tests
compare with (tests/scan_preparation_long_form.py) against a brute-force loop in plain Python, hand-checked cut sets on tied lattices,
the femur alignment against load_femur_model_and_target, the ABI surface, the Python-side argument checks with the native library
stubbed out, and the real library's refusal of every bad argument before it touches a device."""
import ctypes
import os

import numpy as np
import pytest

import scan_preparation_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 2, 3, 5, 6, 9, 81, 100)


def brute_force(points, cells, landmark, count, mask_ids=()):
    """the rules once more, without numpy's sorting or masks: a sort of (d², id) tuples, set membership, a dict for the new ids
    (identity transform) -> (cut ids, dropped ids, kept triangles renumbered, kept old ids)"""
    pts = [tuple(float(x) for x in p) for p in points]
    z = tuple(float(x) for x in landmark)
    keyed = []
    for v, p in enumerate(pts):
        dx, dy, dz = p[0] - z[0], p[1] - z[1], p[2] - z[2]
        keyed.append(((dx * dx + dy * dy) + dz * dz, v))
    keyed.sort()
    cut = {v for _, v in keyed[:min(count, len(pts))]}
    dropped = cut | {int(m) for m in mask_ids if int(m) < len(pts)}
    kept_cells = [tuple(int(v) for v in c) for c in cells if not any(int(v) in dropped for v in c)]
    kept_ids = sorted({v for c in kept_cells for v in c})
    new = {old: k for k, old in enumerate(kept_ids)}
    return cut, dropped, [tuple(new[v] for v in c) for c in kept_cells], kept_ids


def _compare(points, cells, count, mask_ids=()):
    lf = LF.long_form(points, cells, landmarks=points[40:41], cuts=[(0, count)], mask_ids=mask_ids)
    cut, dropped, kept_cells, kept_ids = brute_force(points, cells, points[40], count, mask_ids)
    assert set(np.flatnonzero(lf["cut_flags"] & 1).tolist()) == cut
    assert set(np.flatnonzero(lf["cut_flags"]).tolist()) == dropped
    assert set(np.flatnonzero(lf["cut_flags"] & 0x80).tolist()) == {int(m) for m in mask_ids if int(m) < len(points)}
    assert lf["kept_ids"].tolist() == kept_ids and [tuple(c) for c in lf["partial_cells"].tolist()] == kept_cells
    assert np.array_equal(lf["partial_points"], points[kept_ids]) and lf["counts"] == (len(kept_ids), len(kept_cells))
    assert np.array_equal(lf["aligned"], points)  # the identity transform returns the bits it was given
    return lf


@pytest.mark.parametrize("count", COUNTS)
def test_long_form_against_a_brute_force_loop(count):
    pts, cells = LF.lattice(81)
    assert pts.shape == (81, 3) and cells.shape == (128, 3) and np.array_equal(pts[40], [4.0, 4.0, 0.0])
    lf = _compare(pts, cells, count)
    if count >= 81:
        assert lf["counts"] == (0, 0) and lf["partial_points"].shape == (0, 3) and lf["partial_cells"].shape == (0, 3)
    # … plus a vertex that no triangle references: it leaves the partial mesh even when it is not cut
    more = np.concatenate([pts, [[40.0, 40.0, 1.0]]])
    lf = _compare(more, cells, count)
    assert 81 not in lf["kept_ids"].tolist() and (lf["cut_flags"][81] != 0) == (count >= 82)
    # … and a mask list with a duplicate, the id M and an id far beyond M
    _compare(pts, cells, count, mask_ids=[7, 12, 7, 81, 10 ** 9, 80])


def test_hand_checked_cut_sets(pkg):
    pts, cells = LF.lattice(81)
    cut = lambda p, n: set(LF.cut_set(p, p[40], n).tolist())  # noqa: E731
    assert cut(pts, 1) == {40}
    assert cut(pts, 2) == {31, 40}          # the four edge neighbours 31, 39, 41, 49 tie exactly: the lowest ids
    assert cut(pts, 3) == {31, 39, 40}
    assert cut(pts, 5) == {31, 39, 40, 41, 49}
    assert cut(pts, 6) == {30, 31, 39, 40, 41, 49}  # the four diagonal neighbours 30, 32, 48, 50 tie
    # the lattice spacing of synthetic_face_model(grid=9): 150/9 mm along i, 200/9 mm along j — 31 and 49 are the nearest two
    ref = pkg.data.synthetic_face_model(grid=9, rank=1).ref_points.reshape(9, 9, 3)
    spacing = np.array([ref[1, 0, 0] - ref[0, 0, 0], ref[0, 1, 1] - ref[0, 0, 1], 1.0])
    assert np.allclose(spacing, [150.0 / 9.0, 200.0 / 9.0, 1.0], rtol=1e-14, atol=0)
    face = pts * spacing
    assert cut(face, 2) == {31, 40} and cut(face, 3) == {31, 40, 49}
    for n in (81, 100):
        lf = LF.long_form(pts, cells, landmarks=pts[40:41], cuts=[(0, n)])
        assert lf["counts"] == (0, 0) and np.all(lf["cut_flags"] == 1)


def _femur_landmarks(pkg):
    _, ref_ids, ref_lms = pkg.data.load_femur_mesh("femur_reference")
    target, tgt_ids, tgt_lms = pkg.data.load_femur_mesh("femur_target")
    return target, dict(zip(tgt_ids, np.asarray(tgt_lms, dtype=np.float64))), dict(zip(ref_ids, np.asarray(ref_lms, dtype=np.float64)))


def test_the_femur_alignment(pkg):
    """landmark_alignment on the bundled femur landmarks, then the long form's transform of the 1,622-vertex target: it agrees with
    load_femur_model_and_target's target (numpy's p @ R.T + t) elementwise within 8·2⁻⁵²·(|P|·|R|ᵀ + |t|), the rounding of three
    products and three sums.  Measured where this was written: largest difference 2.8e-14, smallest slack 3.7e-14."""
    target, scan_lms, model_lms = _femur_landmarks(pkg)
    tf = pkg.data.landmark_alignment(scan_lms, model_lms)
    assert len([k for k in scan_lms if k in model_lms]) == 6 and target.n_points == 1622
    assert tf.pre_scale == 1.0 and not tf.centre.any()
    assert abs(np.linalg.det(tf.rotation) - 1.0) <= 1e-12 and np.abs(tf.rotation @ tf.rotation.T - np.eye(3)).max() <= 1e-12
    got = LF.transform(target.points, tf.pre_scale, tf.rotation, tf.centre, tf.translation)
    _, want = pkg.data.load_femur_model_and_target(50)
    bound = 8.0 * 2.0 ** -52 * (np.abs(target.points) @ np.abs(tf.rotation).T + np.abs(tf.translation)[None, :])
    diff = np.abs(got - want.points)
    print("largest difference", diff.max(), "smallest slack", (bound - diff).min())
    assert np.all(diff <= bound)
    # about another centre, behind a pre-scale: the same map of the scan (to rounding)
    scaled = {k: v * 1000.0 for k, v in scan_lms.items()}
    tf2 = pkg.data.landmark_alignment(scaled, model_lms, centre=(10.0, -20.0, 5.0), pre_scale=1.0 / 1000.0)
    got2 = LF.transform(target.points * 1000.0, tf2.pre_scale, tf2.rotation, tf2.centre, tf2.translation)
    assert np.abs(got2 - want.points).max() <= 1e-9
    with pytest.raises(ValueError):
        pkg.data.landmark_alignment({"a": [0, 0, 0]}, model_lms)


def test_symbol_header_and_signature(pkg):
    nat = pkg._native
    assert hasattr(nat.lib(), "icp_scans_prepare_many")
    header = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    for word in ("icp_scans_prepare_many(", "icp_scan_transform", "ICP_SCAN_MAX_CUTS", "ICP_SCAN_PREP_ROUND_BYTES", "LOWEST IDS"):
        assert word in header
    res, args = nat.SIGNATURES["icp_scans_prepare_many"]
    # (the entry point's declaration has 22 parameters, n_items .. status)
    assert res is ctypes.c_int and len(args) == 22 and args[1] is ctypes.c_int
    T = nat.ScanTransform
    assert ctypes.sizeof(T) == 136
    assert [(getattr(T, f).offset, getattr(T, f).size) for f in ("struct_size", "pre_scale", "rotation", "centre", "translation")] == \
        [(0, 8), (8, 8), (16, 72), (88, 24), (112, 24)]
    assert callable(pkg.prepare_scans) and callable(pkg.data.landmark_alignment) and callable(pkg.data.aligned_and_partial_targets)


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def test_prepare_scans_validates_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    Mesh, Tf = pkg.data.TriangleMesh, pkg.data.ScanTransform
    pts, cells = LF.lattice(9)
    mesh, ok, lm = Mesh(pts, cells), Tf(), pts[4:6].copy()

    def moved(i, j, value):
        p = pts.copy()
        p[i, j] = value
        return Mesh(p, cells)

    rot_nan, rot_big = np.eye(3), np.eye(3)
    rot_nan[1, 2], rot_big[0, 0] = np.nan, 2.0 ** 401
    bad_cells = cells.copy()
    bad_cells[0, 1] = 9
    neg_cells = cells.copy()
    neg_cells[1, 2] = -1
    bad = [dict(scans=[], transforms=ok),
           dict(scans=[Mesh(np.zeros((0, 3)), np.zeros((0, 3)))], transforms=ok),                     # M = 0
           dict(scans=[mesh], transforms=Tf(0.0)), dict(scans=[mesh], transforms=Tf(-1.0)), dict(scans=[mesh], transforms=Tf(np.nan)),
           dict(scans=[mesh], transforms=Tf(np.inf)),
           dict(scans=[moved(3, 1, np.inf)], transforms=ok), dict(scans=[moved(8, 2, np.nan)], transforms=ok),
           dict(scans=[moved(0, 0, 2.0 ** 401)], transforms=ok),
           dict(scans=[moved(0, 0, 2.0 ** 300)], transforms=Tf(2.0 ** 101)),                          # |s·x| = 2^401
           dict(scans=[mesh], transforms=Tf(1.0, rot_nan)), dict(scans=[mesh], transforms=Tf(1.0, rot_big)),
           dict(scans=[mesh], transforms=Tf(1.0, np.eye(3), [0.0, -2.0 ** 401, 0.0])),
           dict(scans=[mesh], transforms=Tf(1.0, np.eye(3), np.zeros(3), [np.inf, 0.0, 0.0])),
           dict(scans=[mesh], transforms=ok, landmarks=np.array([[0.0, np.nan, 0.0]])),
           dict(scans=[Mesh(pts, bad_cells)], transforms=ok), dict(scans=[Mesh(pts, neg_cells)], transforms=ok),
           dict(scans=[mesh], transforms=ok, landmarks=lm, cuts=[(0, 1)] * 8),                        # n_cuts = 8
           dict(scans=[mesh], transforms=ok, landmarks=lm, cuts=[(2, 1)]),                            # cut_landmark = L
           dict(scans=[mesh], transforms=ok, landmarks=lm, cuts=[(-1, 1)]),
           dict(scans=[mesh], transforms=ok, landmarks=lm, cuts=[(0, -1)]),
           dict(scans=[mesh], transforms=ok, cuts=[(0, 1)]),                                          # a cut without landmarks
           dict(scans=[mesh], transforms=ok, mask_ids=[3, -1]), dict(scans=[mesh], transforms=ok, mask_ids=[2 ** 31]),
           dict(scans=[mesh, mesh], transforms=[ok]), dict(scans=[mesh, mesh], transforms=ok, landmarks=[lm]),
           dict(scans=[mesh, mesh], transforms=ok, landmarks=lm, cuts=[[(0, 1)]]),
           dict(scans=[mesh, mesh], transforms=ok, mask_ids=[[1], [2], [3]]),
           dict(scans=[mesh], transforms=ok, want=("aligned", "nonsense")), dict(scans=[mesh], transforms=ok, want=())]
    for kw in bad:
        with pytest.raises(ValueError):
            pkg.prepare_scans(**kw)
    good = [dict(scans=mesh, transforms=ok), dict(scans=[mesh, mesh], transforms=[ok, Tf(1e-3, np.eye(3), [1.0, 2.0, 3.0], [4.0, 5.0, 6.0])]),
            dict(scans=[mesh, mesh], transforms=ok, landmarks=lm, cuts=[(0, 0), (1, 100)], mask_ids=[4, 4, 9, 10 ** 9]),
            dict(scans=[mesh, mesh], transforms=ok, landmarks=[lm, lm[:1]], cuts=[[(1, 2)], []], mask_ids=[[1], np.zeros(0, dtype=np.int64)]),
            dict(scans=[moved(0, 0, 2.0 ** 400)], transforms=ok), dict(scans=[Mesh(pts, np.zeros((0, 3)))], transforms=ok, want=("partial",))]
    for kw in good:
        with pytest.raises(AssertionError, match="icp_scans_prepare_many reached"):
            pkg.prepare_scans(**kw)


CANARY = 7.0


def _native_call(pkg, n_items=2, M=None, T=None, points=None, cells=None, transform=None, landmarks=None, L=None, cuts=((0, 3),), n_cuts=None,
                 mask=(1, 1, 50), status=True):
    """the same item n_items times, straight through ctypes, every output canary-filled -> (rc, status, the output arrays)"""
    nat, lib = pkg._native, pkg._native.lib()
    dp, ip, up = nat.c_double_p, nat.c_int_p, nat.c_ubyte_p
    pts0, cells0 = LF.lattice(9)
    pts = np.ascontiguousarray(pts0 if points is None else points, dtype=np.float64)
    cl = np.ascontiguousarray(cells0 if cells is None else cells, dtype=np.int32)
    lm = np.ascontiguousarray(pts0[4:6] if landmarks is None else landmarks, dtype=np.float64)
    tf = transform if transform is not None else nat.ScanTransform(ctypes.sizeof(nat.ScanTransform), 1.0, (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1))
    tfs = (nat.ScanTransform * max(n_items, 1))(*[tf] * max(n_items, 1))
    cut_l = np.array([c[0] for c in cuts], dtype=np.int32)
    cut_c = np.array([c[1] for c in cuts], dtype=np.int32)
    mk = np.array(mask, dtype=np.int32)
    i32 = lambda v: np.full(max(n_items, 1), v, dtype=np.int32)  # noqa: E731
    n_pts, n_tri = i32(pts.shape[0] if M is None else M), i32(cl.shape[0] if T is None else T)
    n_lm, n_ct, n_mk = i32(lm.shape[0] if L is None else L), i32(len(cuts) if n_cuts is None else n_cuts), i32(mk.shape[0])
    outs = {"aligned": np.full((9, 3), CANARY), "landmarks": np.full((2, 3), CANARY), "flags": np.full(9, 7, dtype=np.uint8),
            "ppts": np.full((9, 3), CANARY), "ptris": np.full((8, 3), 7, dtype=np.int32), "kept": np.full(9, 7, dtype=np.int32),
            "counts": np.full(2 * max(n_items, 1), 7, dtype=np.int32)}
    st = np.full(max(n_items, 1), 99, dtype=np.int32)
    rep = lambda a, t: (t * max(n_items, 1))(*[a.ctypes.data_as(t)] * max(n_items, 1))  # noqa: E731
    rc = lib.icp_scans_prepare_many(n_items, 0, n_pts.ctypes.data_as(ip), rep(pts, dp), n_tri.ctypes.data_as(ip), rep(cl, ip), tfs,
                                    n_lm.ctypes.data_as(ip), rep(lm, dp), n_ct.ctypes.data_as(ip), rep(cut_l, ip), rep(cut_c, ip),
                                    n_mk.ctypes.data_as(ip), rep(mk, ip), rep(outs["aligned"], dp), rep(outs["landmarks"], dp),
                                    rep(outs["flags"], up), rep(outs["ppts"], dp), rep(outs["ptris"], ip), rep(outs["kept"], ip),
                                    outs["counts"].ctypes.data_as(ip), st.ctypes.data_as(ip) if status else None)
    return rc, st, outs


def _untouched(outs):
    return all(np.all(a == 7) for a in outs.values())


def test_the_library_refuses_bad_arguments_before_touching_a_device(pkg):
    """ICP_ERR_INVALID_ARG for every item, nothing written — also on a machine without a GPU, where touching the device would be
    ICP_ERR_DEVICE instead"""
    nat = pkg._native
    eye = (1, 0, 0, 0, 1, 0, 0, 0, 1)

    def tf(size=ctypes.sizeof(nat.ScanTransform), s=1.0, rot=eye, c=(0, 0, 0), t=(0, 0, 0)):
        return nat.ScanTransform(size, s, (ctypes.c_double * 9)(*rot), (ctypes.c_double * 3)(*c), (ctypes.c_double * 3)(*t))

    pts, cells = LF.lattice(9)

    def moved(value, i=5, j=1):
        p = pts.copy()
        p[i, j] = value
        return p

    def tri(value):
        c = cells.copy()
        c[3, 2] = value
        return c

    big = 2.0 ** 401
    cases = [dict(transform=tf(size=128)), dict(transform=tf(size=0)),
             dict(transform=tf(s=0.0)), dict(transform=tf(s=-2.0)), dict(transform=tf(s=np.nan)), dict(transform=tf(s=np.inf)),
             dict(points=moved(np.inf)), dict(points=moved(-np.inf)), dict(points=moved(np.nan)),
             dict(landmarks=np.array([[0.0, 0.0, np.nan], [1.0, 1.0, 1.0]])), dict(landmarks=np.array([[0.0, np.inf, 0.0], [1.0, 1.0, 1.0]])),
             dict(transform=tf(rot=(1, 0, 0, 0, np.nan, 0, 0, 0, 1))), dict(transform=tf(rot=(1, 0, np.inf, 0, 1, 0, 0, 0, 1))),
             dict(transform=tf(c=(0, np.nan, 0))), dict(transform=tf(t=(np.inf, 0, 0))),
             dict(points=moved(big)), dict(landmarks=np.array([[0.0, -big, 0.0], [1.0, 1.0, 1.0]])), dict(transform=tf(rot=(big,) + eye[1:])),
             dict(transform=tf(c=(0, 0, -big))), dict(transform=tf(t=(big, 0, 0))),
             dict(points=moved(2.0 ** 300), transform=tf(s=2.0 ** 101)),   # |s·x| = 2^401
             dict(cells=tri(9)), dict(cells=tri(-1)),
             dict(M=0), dict(M=(1 << 26) + 1), dict(T=-1), dict(T=(1 << 26) + 1), dict(L=-1),
             dict(n_cuts=8, cuts=((0, 1),) * 8), dict(n_cuts=-1), dict(cuts=((2, 3),)), dict(cuts=((-1, 3),)), dict(cuts=((0, -1),)),
             dict(mask=(1, -1, 3))]
    for kw in cases:
        rc, st, outs = _native_call(pkg, **kw)
        assert rc == -1 and np.all(st == -1), kw
        assert _untouched(outs), kw
    for kw in (dict(n_items=0), dict(n_items=-3), dict(n_items=65536), dict(status=False)):
        rc, st, outs = _native_call(pkg, **kw)
        assert rc == -1 and np.all(st == 99) and _untouched(outs), kw
    assert b"null argument" in pkg._native.lib().icp_last_error()
