"""GPU: many deterministic ICP fits in one call (icp_fit_deterministic_many; api/other/IcpBasedSurfaceFitting.scala:46-126) against the
one-fit path (icp_fit_deterministic) and the oracle, ModelAndTargetSampling's per-recursion directions (:63-69), batch invariance,
the study's size (StdIcpVsChainICPrandomInitComparisonAll.scala:106-163) and argument errors."""
import ctypes

import numpy as np
import pytest

from conftest import make_theta, open_patch_target

pytestmark = pytest.mark.gpu

SEQ = (1.0, 0.1, 0.01)


def samples(model, target, seed, k=300):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, model.n_points, k).astype(np.int32)
    tps = target.points[rng.integers(0, target.n_points, k)] + rng.normal(size=(k, 3)) * 0.01
    return ids, tps


def one_fit_per_recursion(pkg, ctx, theta, dirs, seq, n_it, ids, tps, step=1.0):
    """icp_fit_deterministic called once per recursion (n_iterations = 0, one sigma2), each result the next start"""
    th = theta.copy()
    for rec, d in enumerate(dirs):
        s = seq[rec // (n_it + 1)]
        fit = pkg.IcpBasedSurfaceFitting(ctx, step, "ModelSampling" if d == 0 else "TargetSampling", ids, tps)
        th = fit.runfitting(0, (s,), th)
    return th


def oracle_per_recursion(oracle, om, ot, theta, dirs, seq, n_it, ids, tps, step=1.0):
    th = theta.copy()
    for rec, d in enumerate(dirs):
        th = oracle.fit_deterministic(om, ot, th, 0, (seq[rec // (n_it + 1)],), direction=int(d), model_ids=ids, target_pts=tps,
                                      step_length=step)
    return th


def rel(a, b):
    return np.abs(a[10:] - b[10:]).max() / np.abs(b[10:]).max()


@pytest.fixture(scope="module")
def two_targets(pkg, oracle, femur50):
    model, target = femur50
    pts, cells = open_patch_target(target)
    patch = pkg.data.TriangleMesh(pts, cells)
    ctxs = [pkg.IcpContext(model, target, device=0), pkg.IcpContext(model, patch, device=0)]
    orc = [oracle.OracleMesh(target.points, target.cells), oracle.OracleMesh(pts, cells)]
    yield [target, patch], ctxs, orc
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("direction", ["ModelSampling", "TargetSampling"])
def test_batched_single_direction_matches_one_fit_and_oracle(pkg, oracle, femur50, femur50_oracle, two_targets, direction):
    model, _ = femur50
    om, _ = femur50_oracle
    targets, ctxs, orc = two_targets
    n_it, B = 4, 12
    ids, _ = samples(model, targets[0], 5)
    tps = [samples(model, targets[b % 2], 100 + b)[1] for b in range(B)]
    th0 = np.stack([make_theta(model, 40 + b, shape_scale=0.3) for b in range(B)])
    got, status = pkg.icp_fits([ctxs[b % 2] for b in range(B)], th0, n_it, SEQ, direction, ids, tps)
    assert np.all(status == 0)
    d = 0 if direction == "ModelSampling" else 1
    for b in range(B):
        assert np.array_equal(got[b, :10], th0[b, :10])
        one = pkg.IcpBasedSurfaceFitting(ctxs[b % 2], 1.0, direction, ids, tps[b]).runfitting(n_it, SEQ, th0[b])
        assert rel(got[b], one) <= 1e-10, b
        want = oracle.fit_deterministic(om, orc[b % 2], th0[b], n_it, SEQ, direction=d, model_ids=ids, target_pts=tps[b])
        assert rel(got[b], want) <= 1e-7, b


def test_model_and_target_sampling_matches_composed_one_fit_and_oracle(pkg, oracle, femur50, femur50_oracle, two_targets):
    model, target = femur50
    om, _ = femur50_oracle
    targets, ctxs, orc = two_targets
    n_it, B = 4, 4
    R = len(SEQ) * (n_it + 1)
    ids, tps = samples(model, target, 9)
    th0 = np.stack([make_theta(model, 60 + b, shape_scale=0.3) for b in range(B)])
    dirs = pkg.direction_schedule(B, R, seed=11)
    assert 0 < dirs.sum() < dirs.size
    got, status = pkg.icp_fits([ctxs[b % 2] for b in range(B)], th0, n_it, SEQ, pkg.ModelAndTargetSampling, ids, tps, directions=dirs)
    assert np.all(status == 0)
    # the same schedule drawn from the seed inside icp_fits
    again, _ = pkg.icp_fits([ctxs[b % 2] for b in range(B)], th0, n_it, SEQ, pkg.ModelAndTargetSampling, ids, tps, seed=11)
    assert np.array_equal(got, again)
    for b in range(B):
        one = one_fit_per_recursion(pkg, ctxs[b % 2], th0[b], dirs[b], SEQ, n_it, ids, tps)
        assert rel(got[b], one) <= 1e-10, b
        want = oracle_per_recursion(oracle, om, orc[b % 2], th0[b], dirs[b], SEQ, n_it, ids, tps)
        assert rel(got[b], want) <= 1e-7, b
        assert np.array_equal(got[b, :10], th0[b, :10])


def test_fitting_class_model_and_target_sampling_matches_oracle(pkg, oracle, femur50, femur50_oracle, two_targets):
    """IcpBasedSurfaceFitting(…, "ModelAndTargetSampling") draws a direction per recursion (seed 1024) instead of acting as ModelSampling"""
    model, target = femur50
    om, ot = femur50_oracle
    _, ctxs, _ = two_targets
    n_it = 4
    ids, tps = samples(model, target, 21)
    th0 = make_theta(model, 77, shape_scale=0.3)
    got = pkg.IcpBasedSurfaceFitting(ctxs[0], 1.0, "ModelAndTargetSampling", ids, tps).runfitting(n_it, SEQ, th0)
    dirs = pkg.direction_schedule(1, len(SEQ) * (n_it + 1), seed=1024)[0]
    want = oracle_per_recursion(oracle, om, ot, th0, dirs, SEQ, n_it, ids, tps)
    assert rel(got, want) <= 1e-7
    model_only = oracle.fit_deterministic(om, ot, th0, n_it, SEQ, direction=0, model_ids=ids, target_pts=tps)
    assert rel(got, model_only) > 1e-6  # (what the wrapper computed before: ModelSampling throughout)


def test_batch_invariance(pkg, femur50, two_targets):
    """40 fits (more than one factorisation launch takes) on three targets, the 58,322-vertex one among them: one call, then calls of
    1 and 7 fits in shuffled order — the same bits"""
    model, _ = femur50
    targets, ctxs, _ = two_targets
    _, big = pkg.data.synthetic_femur_target()
    cbig = pkg.IcpContext(model, big, device=0)
    allc, allt = ctxs + [cbig], targets + [big]
    B, n_it, seq = 40, 2, (1.0, 0.1)
    ids, _ = samples(model, targets[0], 31)
    tps = [samples(model, allt[b % 3], 200 + b)[1] for b in range(B)]
    th0 = np.stack([make_theta(model, 300 + b, shape_scale=0.3) for b in range(B)])
    dirs = pkg.direction_schedule(B, len(seq) * (n_it + 1), seed=5)
    cx = [allc[b % 3] for b in range(B)]
    whole, st = pkg.icp_fits(cx, th0, n_it, seq, pkg.ModelAndTargetSampling, ids, tps, directions=dirs)
    assert np.all(st == 0)
    perm = np.random.default_rng(3).permutation(B)
    parts, i, size = np.zeros_like(whole), 0, 1
    while i < B:
        sel = perm[i:i + size]
        out, st = pkg.icp_fits([cx[b] for b in sel], th0[sel], n_it, seq, pkg.ModelAndTargetSampling, ids, [tps[b] for b in sel],
                               directions=dirs[sel])
        assert np.all(st == 0)
        parts[sel] = out
        i += size
        size = 8 - size  # 1, 7, 1, 7, …
    assert np.array_equal(whole, parts)
    cbig.close()


def test_study_size(pkg, oracle):
    """femur-200 (rank 201), all 1,622 model points and 1,622 target samples, (1e-15,), 100 iterations, ModelAndTargetSampling: 8 fits on
    two targets against the one-fit path recursion by recursion; two of them against the oracle over their first 20 recursions"""
    model, target = pkg.data.load_femur_model_and_target(200)
    pts, cells = open_patch_target(target)
    patch = pkg.data.TriangleMesh(pts, cells)
    ctxs = [pkg.IcpContext(model, target, device=0), pkg.IcpContext(model, patch, device=0)]
    B, n_it, seq = 8, 100, (1e-15,)
    R = n_it + 1
    ids = np.arange(model.n_points, dtype=np.int32)
    tps = [target.points.copy(), pts.copy()]
    th0 = np.stack([pkg.random_initial_parameters(model, b + 1) for b in range(B)])
    dirs = pkg.direction_schedule(B, R, seed=1024)
    cx = [ctxs[b % 2] for b in range(B)]
    got, st = pkg.icp_fits(cx, th0, n_it, seq, pkg.ModelAndTargetSampling, ids, [tps[b % 2] for b in range(B)], directions=dirs)
    assert np.all(st == 0)

    def avg_dist(ctx, theta):
        _, _, d2 = ctx.closestPointOnTarget(ctx.transformedMesh(theta))
        return np.sqrt(d2).mean()

    for b in range(B):
        one = one_fit_per_recursion(pkg, cx[b], th0[b], dirs[b], seq, n_it, ids, tps[b % 2])
        assert rel(got[b], one) <= 1e-9, b
        assert avg_dist(cx[b], got[b]) < avg_dist(cx[b], th0[b]), b
    om = oracle.OracleModel.from_model(model)
    orc = [oracle.OracleMesh(target.points, target.cells), oracle.OracleMesh(pts, cells)]
    n20 = 20
    first, st = pkg.icp_fits(cx[:2], th0[:2], n20 - 1, seq, pkg.ModelAndTargetSampling, ids, tps, directions=dirs[:2, :n20])
    assert np.all(st == 0)
    for b in range(2):
        want = oracle_per_recursion(oracle, om, orc[b], th0[b], dirs[b, :n20], seq, n20 - 1, ids, tps[b])
        assert rel(first[b], want) <= 1e-7, b
    for c in ctxs:
        c.close()


def test_argument_errors_leave_theta_out_untouched(pkg, femur50, two_targets):
    nat, lib = pkg._native, pkg._native.lib()
    model, target = femur50
    _, ctxs, _ = two_targets
    ids, tps = samples(model, target, 41)
    r = model.rank

    def call(contexts, thetas, dirs=None, direction=0, n_ids=None):
        n = len(contexts)
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        out = np.full_like(th, 123.0)
        status = np.full(n, 7, dtype=np.int32)
        fp = nat.FitParams(direction, ids.shape[0] if n_ids is None else n_ids, ids.ctypes.data_as(nat.c_int_p), tps.shape[0],
                           tps.ctypes.data_as(nat.c_double_p), 1.0)
        c_ctx = (ctypes.c_void_p * n)(*[c.h for c in contexts])
        c_fp = (ctypes.POINTER(nat.FitParams) * n)(*[ctypes.pointer(fp)] * n)
        c_in = (nat.c_double_p * n)(*[th[b].ctypes.data_as(nat.c_double_p) for b in range(n)])
        c_out = (nat.c_double_p * n)(*[out[b].ctypes.data_as(nat.c_double_p) for b in range(n)])
        sig = np.array([1.0, 0.1])
        d = None if dirs is None else np.ascontiguousarray(dirs, dtype=np.uint8)
        rc = lib.icp_fit_deterministic_many(n, c_ctx, c_fp, c_in, None if d is None else d.ctypes.data_as(nat.c_ubyte_p), 1, 2,
                                            sig.ctypes.data_as(nat.c_double_p), c_out, status.ctypes.data_as(nat.c_int_p))
        assert np.all(out == 123.0) and np.all(status == 7)
        return rc

    th = np.stack([make_theta(model, 90 + b, shape_scale=0.3) for b in range(2)])
    other, otarget = pkg.data.load_femur_model_and_target(200)
    c200 = pkg.IcpContext(other, otarget, device=0)
    th200 = make_theta(other, 3, shape_scale=0.3)
    assert call([ctxs[0], c200], [th[0], th200[:10 + r]]) == -1                           # two models
    bad_dir = np.zeros((2, 4), dtype=np.uint8)
    bad_dir[1, 2] = 2
    assert call(ctxs, th, dirs=bad_dir) == -1                                               # unknown direction byte
    nan = th.copy()
    nan[1, 12] = np.nan
    assert call(ctxs, nan) == -1                                                            # non-finite theta_init
    assert call(ctxs, th, n_ids=0) == -1                                                    # model side used, no ids
    assert b"model ids" in lib.icp_last_error()
    mixed = np.array([[0, 1, 0, 0], [0, 0, 0, 0]], dtype=np.uint8)
    assert call(ctxs, th, dirs=mixed, n_ids=0) == -1
    c200.close()
