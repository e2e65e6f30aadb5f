"""GPU: registration metrics and Dice of many meshes in one call (icp_mesh_metrics_many; the experiment summary of
apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:43-64) against the one-item path (icp_mesh_metrics) and a CPU restatement of
Dice's counts from oracle calls; identity, separation, batch invariance, the study's size and argument errors."""
import ctypes

import numpy as np
import pytest

from conftest import make_theta, open_patch_target
from test_mesh_metrics_many_cpu import dice_samples

pytestmark = pytest.mark.gpu

S, SEED = 10000, 1024


def one_item(pkg, ctx, theta):
    m = pkg.evaluate_reconstruction_to_ground_truth(ctx, theta)
    return np.array([m["average2surface"], m["hausdorff"], m["average2surface_boundary_aware"], m["max_boundary_aware"], m["kept"]])


def five(m, b):
    return np.array([m["avg"][b], m["hausdorff"][b], m["average2surface_boundary_aware"][b], m["max_boundary_aware"][b], m["kept"][b]])


def target_normals(oracle, points, cells):
    """vertex normals of the target: an OracleModel on its points and cells with a zero basis"""
    M = points.shape[0]
    return oracle.OracleModel(points, cells, np.zeros((M, 3)), np.zeros((3 * M, 1)), np.ones(1)).vertex_normals(points)


def cpu_dice_counts(oracle, om, theta, t_points, t_normals, n=S, seed=SEED):
    """Dice's counts restated from oracle calls: samples in the union box, nearest vertex, its normal, the stated dot product"""
    x = om.instance(theta)
    nx = om.vertex_normals(x)
    lo = np.minimum(x.min(axis=0), t_points.min(axis=0))
    hi = np.maximum(x.max(axis=0), t_points.max(axis=0))
    p = dice_samples(lo, hi, n, seed)

    def inside(pts, nrm):
        idx, _ = oracle.nearest_vertex(p, pts)
        v, nv = pts[idx], nrm[idx]
        return (nv[:, 0] * (v[:, 0] - p[:, 0]) + nv[:, 1] * (v[:, 1] - p[:, 1])) + nv[:, 2] * (v[:, 2] - p[:, 2]) > 0.0
    a, b = inside(x, nx), inside(_f(t_points), t_normals)
    return int(a.sum()), int(b.sum()), int((a & b).sum())


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def counts(m, b):
    return int(m["n_inside_reconstruction"][b]), int(m["n_inside_target"][b]), int(m["n_inside_both"][b])


@pytest.fixture(scope="module")
def two_targets(pkg, femur50):
    model, target = femur50
    pts, cells = open_patch_target(target)
    patch = pkg.data.TriangleMesh(pts, cells)
    ctxs = [pkg.IcpContext(model, target, device=0), pkg.IcpContext(model, patch, device=0)]
    yield [target, patch], ctxs
    for c in ctxs:
        c.close()


def test_same_bits_as_one_item(pkg, femur50, two_targets):
    model, _ = femur50
    targets, ctxs = two_targets
    B = 12
    th = np.stack([make_theta(model, 60 + b, shape_scale=0.4) for b in range(B)])
    for ctx in ctxs:
        m = pkg.registration_metrics(ctx, th, dice_samples=S, seed=SEED)
        assert np.all(m["status"] == 0)
        for b in range(B):
            want = one_item(pkg, ctx, th[b])
            assert np.array_equal(five(m, b), want, equal_nan=True), (b, five(m, b), want)
            assert 0.0 <= m["dice"][b] <= 1.0
    assert np.all(m["kept"] < model.n_points)  # (the open target drops some vertices: the boundary-aware path ran)
    m0 = pkg.registration_metrics(ctxs[0], th, dice_samples=0)
    assert np.all(np.isnan(m0["dice"])) and np.all(np.isnan(m0["n_inside_both"]))
    assert np.array_equal(m0["avg"], pkg.registration_metrics(ctxs[0], th, dice_samples=S)["avg"])


def test_dice_counts_equal_cpu_restatement(pkg, oracle, femur50, femur50_oracle, two_targets):
    model, target = femur50
    om, _ = femur50_oracle
    _, ctxs = two_targets
    tn = target_normals(oracle, target.points, target.cells)
    th = np.stack([make_theta(model, 90 + b, shape_scale=0.4) for b in range(3)])
    m = pkg.registration_metrics(ctxs[0], th, dice_samples=S, seed=SEED)
    for b in range(3):
        na, nb, nab = cpu_dice_counts(oracle, om, th[b], target.points, tn)
        assert counts(m, b) == (na, nb, nab), b
        assert m["dice"][b] == 2.0 * nab / (na + nb)
        assert 0.5 < m["dice"][b] < 1.0  # (the same bone, a few mm apart)
    assert pkg.dice_coefficient(ctxs[0], th[1], S, SEED) == m["dice"][1]
    other = pkg.registration_metrics(ctxs[0], th[:1], dice_samples=S, seed=SEED + 1)
    assert counts(other, 0) != counts(m, 0)  # (another seed: other samples)


def test_identity(pkg, oracle, femur50, femur50_oracle):
    model, _ = femur50
    om, _ = femur50_oracle
    th = make_theta(model, 7, shape_scale=0.5)
    self_mesh = pkg.data.TriangleMesh(om.instance(th), model.cells)
    ctx = pkg.IcpContext(model, self_mesh, device=0)
    try:
        m = pkg.registration_metrics(ctx, th[None, :], dice_samples=S, seed=SEED)
        na, nb, nab = counts(m, 0)
        assert na == nb == nab and na > 0
        assert m["dice"][0] == 1.0
        assert m["avg"][0] == 0.0 and m["hausdorff"][0] == 0.0
    finally:
        ctx.close()


def test_separation(pkg, femur50, femur50_oracle, two_targets):
    model, target = femur50
    om, _ = femur50_oracle
    _, ctxs = two_targets
    th = make_theta(model, 11, shape_scale=0.3, pose=False)
    x = om.instance(th)
    extent = (x[:, 0].max() - x[:, 0].min()) + (target.points[:, 0].max() - target.points[:, 0].min())
    shifts = [0.0, 5.0, 20.0, extent + 10.0]
    thetas = np.stack([th] * len(shifts))
    thetas[:, 1] += shifts
    m = pkg.registration_metrics(ctxs[0], thetas, dice_samples=S, seed=SEED)
    d = m["dice"]
    assert d[0] > d[1] > d[2] > d[3], d
    assert m["n_inside_both"][3] == 0 and d[3] == 0.0
    assert m["n_inside_reconstruction"][3] > 0 and m["n_inside_target"][3] > 0


def test_batch_invariance(pkg, femur50, two_targets):
    """40 items on three targets (the 58,322-vertex one among them) in one call, then calls of 1 and 7 items in shuffled order"""
    model, _ = femur50
    _, ctxs = two_targets
    _, big = pkg.data.synthetic_femur_target()
    cbig = pkg.IcpContext(model, big, device=0)
    try:
        allc = ctxs + [cbig]
        B = 40
        th = np.stack([make_theta(model, 400 + b, shape_scale=0.4) for b in range(B)])
        cx = [allc[b % 3] for b in range(B)]
        keys = ["avg", "hausdorff", "dice", "average2surface_boundary_aware", "max_boundary_aware", "kept", "n_inside_reconstruction",
                "n_inside_target", "n_inside_both"]
        whole = pkg.registration_metrics(cx, th, dice_samples=4000, seed=SEED)
        assert np.all(whole["status"] == 0)
        perm = np.random.default_rng(3).permutation(B)
        parts = {k: np.zeros(B) for k in keys}
        i, size = 0, 1
        while i < B:
            sel = perm[i:i + size]
            m = pkg.registration_metrics([cx[b] for b in sel], th[sel], dice_samples=4000, seed=SEED)
            for k in keys:
                parts[k][sel] = m[k]
            i += size
            size = 8 - size  # 1, 7, 1, 7, …
        for k in keys:
            assert np.array_equal(whole[k], parts[k], equal_nan=True), k
    finally:
        cbig.close()


def test_study_size(pkg, oracle):
    """femur-200 (rank 201) against the 58,322-vertex synthetic target, 300 items from random_initial_parameters"""
    model, _ = pkg.data.load_femur_model_and_target(200)
    _, big = pkg.data.synthetic_femur_target()
    ctx = pkg.IcpContext(model, big, device=0)
    try:
        B = 300
        th = np.stack([pkg.random_initial_parameters(model, b) for b in range(B)])
        m = pkg.registration_metrics(ctx, th, dice_samples=S, seed=SEED)
        assert np.all(m["status"] == 0)
        for k in ("avg", "hausdorff", "dice", "kept"):
            assert np.all(np.isfinite(m[k])), k
        assert np.all((m["dice"] >= 0.0) & (m["dice"] <= 1.0))
        for b in range(B):
            assert np.array_equal(five(m, b), one_item(pkg, ctx, th[b]), equal_nan=True), b
        om = oracle.OracleModel.from_model(model)
        tn = target_normals(oracle, big.points, big.cells)
        for b in (0, 150, 299):
            assert counts(m, b) == cpu_dice_counts(oracle, om, th[b], big.points, tn), b
    finally:
        ctx.close()


def test_argument_errors(pkg, femur50, two_targets):
    model, _ = femur50
    _, ctxs = two_targets
    nat, lib = pkg._native, pkg._native.lib()
    m200, t200 = pkg.data.load_femur_model_and_target(200)
    c200 = pkg.IcpContext(m200, t200, device=0)
    try:
        th = np.stack([make_theta(model, b) for b in range(2)])
        out = np.full(18, 7.0)
        status = np.full(2, 99, dtype=np.int32)
        o, s = out.ctypes.data_as(nat.c_double_p), status.ctypes.data_as(nat.c_int_p)

        def call(cx, thetas, n_samples=100, n=2):
            c_ctx = (ctypes.c_void_p * len(cx))(*[c.h if c is not None else None for c in cx])
            c_th = (nat.c_double_p * len(thetas))(*[t.ctypes.data_as(nat.c_double_p) if t is not None else None for t in thetas])
            return lib.icp_mesh_metrics_many(n, c_ctx, c_th, n_samples, 1024, o, s)
        assert call([ctxs[0], None], list(th)) == -1
        assert call([ctxs[0], ctxs[1]], [th[0], None]) == -1
        bad = th.copy()
        bad[1, 3] = np.inf
        assert call([ctxs[0], ctxs[1]], list(bad)) == -1
        assert call([ctxs[0], c200], [th[0], np.zeros(10 + m200.rank)]) == -1  # mixed models
        assert call(ctxs, list(th), -1) == -1
        assert call(ctxs, list(th), (1 << 24) + 1) == -1
        assert call(ctxs, list(th), n=0) == -1
        assert np.all(out == 7.0) and np.all(status == 99)
        assert call(ctxs, list(th)) == 0 and np.all(status == 0) and np.all(np.isfinite(out))
    finally:
        c200.close()
