"""CPU: PCA shape models with Procrustes alignment (icp_pca_models_many, api.pca_models) — the numpy long form the GPU tests compare
with (tests/pca_model_long_form.py): its two rigid solvers against each other, equivariance under a global motion, the Gram route
against numpy's SVD, the rank rule on centred data; the ABI surface, the Python-side argument checks with the native library stubbed
out, and the real library's refusal of every limit before it touches a device."""
import ctypes
import os

import numpy as np
import pytest

import pca_model_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def femur(pkg):
    return pkg.data.load_femur_model(50)


def conditioning_bound(meshes, gap):
    """1e3·2⁻⁵²·max|coordinate|/gap: the project's margin over the rotation's conditioning"""
    return 1e3 * EPS * max(float(np.abs(m).max()) for m in meshes) / gap


def test_two_rotation_solvers_agree(femur):
    """Kabsch by SVD with the determinant correction against Horn by eigh, through three rounds of alignment"""
    for seed, n in ((1, 12), (2, 5)):
        meshes = LF.posed_instances(femur, n, seed=seed)
        horn, kabsch = LF.gpa(meshes, 3, 0.0, "horn"), LF.gpa(meshes, 3, 0.0, "kabsch")
        bound = conditioning_bound(meshes, horn["gap"])
        spread = np.abs(horn["aligned"] - kabsch["aligned"]).max()
        print(f"n = {n}: max|coordinate| {max(np.abs(m).max() for m in meshes):.1f}, gap {horn['gap']:.4f}, "
              f"|Horn - Kabsch| {spread:.3e} mm, bound {bound:.3e}")
        assert 0.0 < horn["gap"] < 1.0 and spread <= bound
        assert np.abs(horn["mean"] - kabsch["mean"]).max() <= bound
        assert np.abs(horn["transforms"] - kabsch["transforms"])[:, :9].max() <= bound / 100.0  # (a rotation entry: no 200 mm lever)
        for tf, x, a in zip(horn["transforms"], meshes, horn["aligned"]):  # the composite reproduces the aligned mesh
            R = tf[:9].reshape(3, 3)
            assert abs(np.linalg.det(R) - 1.0) <= 1e-13 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-13
            assert np.abs(x @ R.T + tf[9:] - a).max() <= bound


def test_gpa_zero_rounds_and_halt(femur):
    meshes = LF.posed_instances(femur, 12, seed=3)
    none = LF.gpa(meshes, 0, 1e-3)
    assert none["rounds"] == 0 and np.array_equal(none["aligned"], np.stack(meshes))
    assert np.array_equal(none["transforms"], np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (12, 1)))
    full = LF.gpa(meshes, 8, 0.0)
    print("rms per round", full["rms"])
    assert full["rounds"] == 8 and all(a > b for a, b in zip(full["rms"][:3], full["rms"][1:4]))
    # a threshold that every RMS value misses by a factor >= 1.5 on either side stops behind the first round below it
    halt = 1e-3
    assert all(r >= 1.5 * halt or r <= halt / 1.5 for r in full["rms"])
    k = next(i for i, r in enumerate(full["rms"]) if r < halt)
    assert LF.gpa(meshes, 8, halt)["rounds"] == k + 1 and LF.gpa(meshes, 1, halt)["rounds"] == 1


def test_global_motion(femur):
    """GPA of a set and of the same set under one global rigid motion: the same model up to that motion"""
    meshes = LF.posed_instances(femur, 10, seed=4)
    rng = np.random.default_rng(40)
    R, t = LF.random_rotation(rng, 1.0), np.array([30.0, -50.0, 12.0])
    moved = [m @ R.T + t for m in meshes]
    a, b = LF.long_form(meshes, iterations=3, halt_distance=0.0), LF.long_form(moved, iterations=3, halt_distance=0.0)
    bound = conditioning_bound(moved, min(a["gap"], b["gap"]))
    assert np.abs(a["aligned"] @ R.T + t - b["aligned"]).max() <= bound
    assert np.abs(a["mean"] @ R.T + t - b["mean"]).max() <= bound
    assert a["rank"] == b["rank"] == 9
    assert np.abs(a["variance"] - b["variance"]).max() <= 1e-10 * a["variance"][0]
    # the covariance rotates with the motion: rows of B·diag(var)·Bᵀ
    rot = lambda B: (B.reshape(-1, 3, B.shape[1]).transpose(0, 2, 1) @ R.T).transpose(0, 2, 1).reshape(B.shape)  # noqa: E731
    Ba, Bb = rot(a["basis"]), b["basis"]
    rows = [0, 7, 2000, 4865]
    cov_a, cov_b = (Ba[rows] * a["variance"]) @ Ba.T, (Bb[rows] * b["variance"]) @ Bb.T
    assert np.abs(cov_a - cov_b).max() <= 1e-9 * np.abs(cov_b).max()


def test_gram_route_equals_svd(femur):
    for n, seed in ((3, 5), (12, 6), (40, 7)):
        lf = LF.long_form(LF.posed_instances(femur, n, seed=seed), iterations=3, halt_distance=0.0)
        theta, U = LF.pca_svd(lf["aligned"], lf["mean"])
        err = np.abs(lf["theta"][:n - 1] - theta[:n - 1]).max()
        print(f"n = {n}: theta_1 {theta[0]:.4e}, |Gram - SVD| {err:.3e}")
        assert err <= 1e-10 * theta[0]
        N, B = lf["aligned"].shape[1], lf["basis"]
        assert lf["rank"] == n - 1 and np.abs(B.T @ B / N - np.eye(n - 1)).max() <= 1e3 * EPS * theta[0] / theta[n - 2]
        # invariants, not single vectors: the projector onto the span
        assert np.abs(B @ (B.T @ U[:, 0]) / N - U[:, 0]).max() <= 1e-9


def test_rank_rule(femur):
    """on centred data the one structural zero eigenvalue falls below τ and the smallest real one above it; a duplicated mesh loses
    one more component; identical meshes keep none"""
    for n, seed in ((3, 8), (12, 9), (40, 10)):
        meshes = LF.posed_instances(femur, n, seed=seed)
        lf = LF.long_form(meshes, iterations=3, halt_distance=0.0)
        zero, smallest = lf["theta"][n - 1], lf["theta"][n - 2]
        print(f"n = {n}: structural zero {zero:.2e}, tau {lf['tau']:.2e} (tau_0 {lf['tau0']:.2e}), smallest real eigenvalue {smallest:.3f}")
        assert abs(zero) < lf["tau"] < smallest and lf["tau0"] < lf["tau"] and lf["rank"] == n - 1
        dup = LF.long_form(meshes + [meshes[1]], iterations=3, halt_distance=0.0)
        assert dup["rank"] == n - 1 and np.all(np.abs(dup["theta"][n - 1:]) < dup["tau"])  # n + 1 meshes: n − 1 = (n + 1) − 2
    same = LF.long_form([meshes[0]] * 5, iterations=3, halt_distance=0.0)
    assert same["rank"] == 0 and same["trace"] <= same["tau0"]


# ---- the surface

def test_symbol_header_and_signature(pkg):
    nat = pkg._native
    assert hasattr(nat.lib(), "icp_pca_models_many")
    header = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    for word in ("icp_pca_models_many(", "ICP_PCA_MODELS_MAX_ROUNDS", "NOT Scalismo's procrustesDistance", "tau_0"):
        assert word in header
    res, args = nat.SIGNATURES["icp_pca_models_many"]
    # (the entry point's declaration has 17 parameters, n_items .. status)
    assert res is ctypes.c_int and len(args) == 17 and args[1] is ctypes.c_int
    assert callable(pkg.pca_models) and callable(pkg.pca_model) and callable(pkg.leave_one_out_pca_models)


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def test_pca_models_validates_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    rng = np.random.default_rng(0)
    a, b, c = (rng.normal(size=(7, 3)) for _ in range(3))
    short, nan = rng.normal(size=(6, 3)), a.copy()
    nan[2, 1] = np.nan
    bad = [dict(mesh_sets=[]), dict(mesh_sets=[[a]]), dict(mesh_sets=[[a] * 257]), dict(mesh_sets=[[a, short]]),
           dict(mesh_sets=[[a, nan]]), dict(mesh_sets=[[a, np.zeros((7, 2))]]), dict(mesh_sets=[[a, np.zeros((0, 3))]]),
           dict(mesh_sets=[[a, b, c]], rank=0), dict(mesh_sets=[[a, b, c]], rank=3), dict(mesh_sets=[[a, b, c]], rank=[1, 2]),
           dict(mesh_sets=[[a, b, c]], gpa_iterations=-1), dict(mesh_sets=[[a, b, c]], gpa_iterations=33),
           dict(mesh_sets=[[a, b, c]], halt_distance=-1e-3), dict(mesh_sets=[[a, b, c]], halt_distance=np.nan),
           dict(mesh_sets=[[a, b, c]], halt_distance=np.inf), dict(mesh_sets=[[a, b, c]], reference=short),
           dict(mesh_sets=[[a, b, c]], reference=nan), dict(mesh_sets=[[a, b], [a, c]], reference=[a]),
           dict(mesh_sets=[[a, b, c]], want=("variance", "nonsense"))]
    for kw in bad:
        with pytest.raises(ValueError):
            pkg.pca_models(**kw)
    with pytest.raises(ValueError):
        pkg.leave_one_out_pca_models([a, b])
    mesh = pkg.data.TriangleMesh(a, np.array([[0, 1, 2]]))
    good = [dict(mesh_sets=[[a, b]]), dict(mesh_sets=[[a, b, c], [mesh, c]], rank=[2, None], gpa_iterations=[0, 32], halt_distance=0.0),
            dict(mesh_sets=[[a, b, c]], reference=b, cells=np.array([[0, 1, 2]]), want=())]
    for kw in good:
        with pytest.raises(AssertionError, match="icp_pca_models_many reached"):
            pkg.pca_models(**kw)
    with pytest.raises(AssertionError, match="icp_pca_models_many reached"):
        pkg.leave_one_out_pca_models([a, b, c])
    with pytest.raises(AssertionError, match="icp_pca_models_many reached"):
        pkg.pca_model([a, b, c], rank=1)


CANARY = 7.0


def _native_call(pkg, n_items=2, meshes=None, n_meshes=None, ids=None, pool_points=None, rank=2, rounds=3, halt=1e-5, reference=None,
                 n_pool=None, status=True, null_ids=False):
    """the same item n_items times, straight through ctypes, every output canary-filled -> (rc, status, the output arrays)"""
    nat, lib = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    rng = np.random.default_rng(1)
    pool = [np.ascontiguousarray(m, dtype=np.float64) for m in (meshes if meshes is not None else [rng.normal(size=(9, 3)) for _ in range(4)])]
    k = max(n_items, 1)
    row = np.array(ids if ids is not None else [0, 1, 2, 3], dtype=np.int32)
    i32 = lambda v: np.full(k, v, dtype=np.int32)  # noqa: E731
    pp = np.array(pool_points if pool_points is not None else [m.shape[0] for m in pool], dtype=np.int32)
    nm, rk, it = i32(len(row) if n_meshes is None else n_meshes), i32(rank), i32(rounds)
    hd = np.full(k, halt, dtype=np.float64)
    outs = {"variance": np.full(8, CANARY), "basis": np.full((27, 8), CANARY), "mean": np.full((9, 3), CANARY),
            "transforms": np.full((8, 12), CANARY), "info": np.full(8, CANARY)}
    st = np.full(k, 99, dtype=np.int32)
    rep = lambda a, t: (t * k)(*[a.ctypes.data_as(t)] * k)  # noqa: E731
    pool_arr = (dp * len(pool))(*[m.ctypes.data_as(dp) for m in pool])
    ref = None if reference is None else rep(np.ascontiguousarray(reference, dtype=np.float64), dp)
    rc = lib.icp_pca_models_many(n_items, 0, len(pool) if n_pool is None else n_pool, pp.ctypes.data_as(ip), pool_arr, nm.ctypes.data_as(ip),
                                 (ip * k)() if null_ids else rep(row, ip), ref, rk.ctypes.data_as(ip), it.ctypes.data_as(ip),
                                 hd.ctypes.data_as(dp), rep(outs["variance"], dp), rep(outs["basis"], dp), rep(outs["mean"], dp),
                                 rep(outs["transforms"], dp), rep(outs["info"], dp), st.ctypes.data_as(ip) if status else None)
    return rc, st, outs


def test_the_library_refuses_every_limit_before_touching_a_device(pkg):
    """ICP_ERR_INVALID_ARG for every item, nothing written — also on a machine without a GPU, where touching the device would be
    ICP_ERR_DEVICE instead"""
    rng = np.random.default_rng(2)
    four = [rng.normal(size=(9, 3)) for _ in range(4)]

    def spoiled(value):
        m = [x.copy() for x in four]
        m[2][5, 1] = value
        return m

    bad_ref = np.zeros((9, 3))
    bad_ref[0, 0] = np.inf
    cases = [dict(ids=[0], rank=1), dict(n_meshes=1), dict(n_meshes=0), dict(n_meshes=257), dict(ids=list(range(4)) * 65, rank=2),  # n = 260
             dict(rank=0), dict(rank=4), dict(rank=-1), dict(rounds=-1), dict(rounds=33),
             dict(halt=-1.0), dict(halt=np.nan), dict(halt=np.inf),
             dict(ids=[0, 1, 4, 2]), dict(ids=[0, -1, 2, 3]), dict(null_ids=True),
             dict(meshes=four[:3] + [rng.normal(size=(8, 3))]),                       # two N in one item
             dict(pool_points=[9, 9, 0, 9]), dict(pool_points=[9, 9, -3, 9]),        # N < 1
             dict(pool_points=[715827883] * 4),                                       # 3N > INT32_MAX (refused before a point is read)
             dict(meshes=spoiled(np.nan)), dict(meshes=spoiled(np.inf)), dict(meshes=spoiled(-np.inf)),
             dict(reference=bad_ref)]
    for kw in cases:
        rc, st, outs = _native_call(pkg, **kw)
        assert rc == -1 and np.all(st == -1), kw
        assert all(np.all(a == CANARY) for a in outs.values()), kw
    assert b"n_meshes" in pkg._native.lib().icp_last_error()
    for kw in (dict(n_items=0), dict(n_items=-3), dict(n_items=65536), dict(status=False), dict(n_pool=0)):
        rc, st, outs = _native_call(pkg, **kw)
        assert rc == -1 and np.all(st == 99) and all(np.all(a == CANARY) for a in outs.values()), kw
