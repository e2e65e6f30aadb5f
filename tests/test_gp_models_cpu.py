"""CPU: Gaussian-process shape models from analytic kernels (icp_gp_models_many) — the numpy long form the GPU tests compare against
(tests/gp_model_long_form.py) checked against the dense kernel matrix, femur_kernel's values, the Python-side argument checks with the
native library stubbed out, and the real library's refusal of every bad argument before it touches a device."""
import ctypes
import os

import numpy as np
import pytest

import gp_model_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense(pkg, pts, terms):
    K = np.zeros((3 * len(pts), 3 * len(pts)))
    for t in terms:
        K += t(pts[:, None, :], pts[None, :, :]).transpose(0, 2, 1, 3).reshape(K.shape)
    return K


def _small(pkg, n=30, seed=3):
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 3)) * np.array([60.0, 15.0, 10.0])
    return pts, pkg.data.femur_kernel(pts)


def test_symbol_header_and_signature(pkg):
    nat = pkg._native
    assert hasattr(nat.lib(), "icp_gp_models_many")
    header = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    for word in ("icp_gp_models_many(", "icp_kernel_term", "ICP_GP_MODELS_CHUNK_BYTES", "ICP_GP_MODELS_MAX_PIVOTS", "ICP_GP_MODELS_MAX_TERMS"):
        assert word in header
    res, args = nat.SIGNATURES["icp_gp_models_many"]
    assert res is ctypes.c_int and len(args) == 15 and args[1] is ctypes.c_int
    assert ctypes.sizeof(nat.KernelTerm) == 11 * 8
    assert callable(pkg.gp_models) and callable(pkg.gp_model) and callable(pkg.data.femur_kernel)


def test_long_form_kernel_columns_are_the_dense_matrix(pkg):
    pts, terms = _small(pkg)
    K = _dense(pkg, pts, terms)
    assert np.array_equal(K, K.T)
    rows = [0, 7, 44, 89]
    assert np.abs(LF.kernel_columns(pts, terms, rows) - K[:, rows]).max() <= 1e-13 * np.abs(K).max()
    assert np.abs(LF.kernel_diagonal(len(pts), terms) - np.diag(K)).max() <= 1e-13 * np.abs(K).max()


@pytest.mark.parametrize("m", [1, 5, 40, 90])
def test_long_form_against_the_dense_matrix(pkg, m):
    """trace(K) = Σθ + Σ residual to 1e-14 relative; with rank = m, |K − B diag(var) Bᵀ|_ab <= sqrt(res_a res_b) + 1e-9 max|K| (the
    residual matrix K − L Lᵀ is positive semi-definite: Cauchy–Schwarz)"""
    pts, terms = _small(pkg)
    K = _dense(pkg, pts, terms)
    lf = LF.long_form(pts, terms, m)
    assert lf["m_eff"] == m and len(set(lf["pivots"].tolist())) == m
    assert np.all(lf["step_taken"] == lf["step_max"]) and np.all(np.diff(lf["variance"]) <= 0)
    assert abs(lf["trace"] - np.trace(K)) <= 1e-14 * np.trace(K)
    assert abs(lf["trace"] - (lf["theta"].sum() + lf["residual"].sum())) <= 1e-14 * lf["trace"]
    assert lf["residual"].min() >= -m * 2.0 ** -52 * np.diag(K).max()
    B = lf["basis"]
    n = len(pts)
    assert np.abs(B.T @ B / n - np.eye(m)).max() <= 1e3 * 2.0 ** -52 * lf["variance"][0] / lf["variance"][-1]
    res = np.maximum(lf["residual"], 0.0)
    err = np.abs(K - (B * lf["variance"]) @ B.T)
    assert np.all(err <= np.sqrt(res[:, None] * res[None, :]) + 1e-9 * np.abs(K).max())
    if m == 90:  # full rank: the model IS the kernel matrix
        assert err.max() <= 1e-9 * np.abs(K).max()


def test_long_form_on_the_femur_reference(pkg):
    """the sizes of the issue's table: N = 1,622, 51 pivots hold about 85 % of the trace; sampled rows within the Cauchy–Schwarz bound"""
    mesh, _, _ = pkg.data.load_femur_mesh("femur_reference")
    terms = pkg.data.femur_kernel(mesh)
    lf = LF.long_form(mesh.points, terms, 51)
    assert lf["m_eff"] == 51
    share = lf["theta"].sum() / lf["trace"]
    assert 0.80 < share < 0.90
    assert abs(lf["trace"] - (lf["theta"].sum() + lf["residual"].sum())) <= 1e-14 * lf["trace"]
    rows = np.arange(0, 3 * mesh.n_points, 97)
    Kr = LF.kernel_columns(mesh.points, terms, rows).T
    B = lf["basis"]
    res = np.maximum(lf["residual"], 0.0)
    err = np.abs(Kr - (B[rows] * lf["variance"]) @ B.T)
    assert np.all(err <= np.sqrt(res[rows][:, None] * res[None, :]) + 1e-9 * np.abs(Kr).max())


def test_long_form_stops_and_takes_pivots_handed_in(pkg):
    pts, terms = _small(pkg)
    own = LF.long_form(pts, terms, 40)
    again = LF.long_form(pts, terms, 40, pivots=own["pivots"])
    assert np.array_equal(own["L"], again["L"]) and np.array_equal(own["variance"], again["variance"])
    other = LF.long_form(pts, terms, 40, pivots=own["pivots"][::-1].copy())
    assert other["m_eff"] == 40 and np.any(other["step_taken"] < other["step_max"])
    tol = LF.long_form(pts, terms, 90, rel_tolerance=0.2)
    assert 1 <= tol["m_eff"] < 90 and tol["sum_after"] <= 0.2 * tol["trace"] < tol["step_sum"][-1]
    dup = np.concatenate([pts[:10], pts[:10]])
    d = LF.long_form(dup, terms, 60)
    assert d["m_eff"] <= 30 and np.all(np.isfinite(d["basis"]))


def test_femur_kernel_values(pkg):
    mesh, _, _ = pkg.data.load_femur_mesh("femur_reference")
    terms = pkg.data.femur_kernel(mesh)
    assert [(t.scale, t.sigma) for t in terms] == [(10.0, 90.0), (5.0, 40.0), (3.0, 10.0)]
    B = terms[0].A
    assert np.array_equal(B, B.T) and np.array_equal(terms[1].A, np.eye(3)) and np.array_equal(terms[2].A, np.eye(3))
    w, v = np.linalg.eigh(B)
    assert np.allclose(w, [1.0, 1.0, 10.0], rtol=0, atol=1e-12)
    # the axis of the ten-fold variance is the bone's length: the direction of largest spread of the points
    p = mesh.points - mesh.points.mean(axis=0)
    spread = np.linalg.eigh(p.T @ p)[1][:, -1]
    assert abs(abs(v[:, -1] @ spread) - 1.0) <= 1e-12
    u = pkg.data.axis_of_main_variance(mesh.points)
    for signs in ([1, -1, 1], [-1, -1, -1]):
        us = u * np.array(signs, dtype=np.float64)
        assert np.allclose(us @ np.diag([10.0, 1.0, 1.0]) @ us.T, B, rtol=0, atol=1e-14)
    x = mesh.points[5]
    k0 = sum(t(x, x) for t in terms)
    assert np.allclose(k0, 10.0 * B + 8.0 * np.eye(3), rtol=0, atol=1e-13)
    y = x + np.array([30.0, 0.0, 40.0])  # |x − y| = 50
    want = 10.0 * np.exp(-2500.0 / 8100.0) * B + (5.0 * np.exp(-2500.0 / 1600.0) + 3.0 * np.exp(-25.0)) * np.eye(3)
    assert np.allclose(sum(t(x, y) for t in terms), want, rtol=0, atol=1e-13)
    assert abs(LF.kernel_diagonal(1, terms).sum() - (10.0 * 12.0 + 24.0)) <= 1e-12  # trace(K)/N = 144


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def _bad_terms(pkg):
    T = pkg.data.GaussianKernelTerm
    asym = np.eye(3)
    asym[0, 1] = 1e-17
    indef = np.diag([1.0, 1.0, -1e-3])
    indef2 = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    return [[T(1.0, 10.0, asym)], [T(1.0, 10.0, indef)], [T(1.0, 10.0, indef2)], [T(1.0, 10.0, np.zeros((3, 3)))], [T(1.0, 0.0)], [T(1.0, -3.0)],
            [T(1.0, np.inf)], [T(0.0, 10.0)], [T(-1.0, 10.0)], [T(np.nan, 10.0)], [], [T(1.0, 10.0)] * 9]


def test_gp_models_validate_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    T = pkg.data.GaussianKernelTerm
    mesh = pkg.data.TriangleMesh(np.arange(21.0).reshape(7, 3) ** 2, np.array([[0, 1, 2]]))
    ok = [T(2.0, 30.0)]
    bad = [dict(meshes=[], kernels=[ok], n_pivots=3),
           dict(meshes=[mesh], kernels=ok, n_pivots=3, rank=4),          # rank > pivots
           dict(meshes=[mesh], kernels=ok, n_pivots=22),                 # pivots > 3N
           dict(meshes=[mesh], kernels=ok, n_pivots=0),
           dict(meshes=[mesh], kernels=ok, n_pivots=3, rank=0),
           dict(meshes=[mesh], kernels=ok, n_pivots=3, rel_tolerance=1.0),
           dict(meshes=[mesh], kernels=ok, n_pivots=3, rel_tolerance=-0.1),
           dict(meshes=[mesh, mesh], kernels=[ok], n_pivots=3),          # one kernel per mesh, or one for all
           dict(meshes=[mesh, mesh], kernels=ok, n_pivots=[3]),
           dict(meshes=[mesh], kernels=ok, n_pivots=3, want=("variance", "nonsense"))]
    bad += [dict(meshes=[mesh], kernels=[k], n_pivots=3) for k in _bad_terms(pkg)]
    for kw in bad:
        with pytest.raises(ValueError):
            pkg.gp_models(**kw)
    big = pkg.data.TriangleMesh(np.zeros((100, 3)), np.array([[0, 1, 2]]))
    with pytest.raises(ValueError):
        pkg.gp_models([big], ok, 257)                                    # pivots > 256
    inf = mesh.points.copy()
    inf[3, 1] = np.inf
    with pytest.raises(ValueError):
        pkg.gp_model(pkg.data.TriangleMesh(inf, mesh.cells), ok, 3)
    with pytest.raises(AssertionError, match="icp_gp_models_many reached"):  # good arguments go through to the library
        pkg.gp_model(mesh, [T(1.0, 10.0, np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]]))], 21, 5)


def _native_call(pkg, pts, terms, n_pivots, rank, tol=None, n_items=1):
    """one item (or the same one n_items times) straight through ctypes -> (rc, status, the output arrays)"""
    nat, L = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    arr = (nat.KernelTerm * max(len(terms), 1))()
    for t, k in enumerate(terms):
        arr[t].scale, arr[t].sigma = k.scale, k.sigma
        arr[t].A[:] = np.asarray(k.A, dtype=np.float64).reshape(-1).tolist()
    n = n_items
    i32 = lambda v: np.full(n, v, dtype=np.int32)  # noqa: E731
    n_pts, n_terms, mp, rk = i32(pts.shape[0]), i32(len(terms)), i32(n_pivots), i32(rank)
    var, info = np.full(300, 7.0), np.full(4, 7.0)
    status = np.full(n, 99, dtype=np.int32)
    c_pts = (dp * n)(*[pts.ctypes.data_as(dp)] * n)
    c_terms = (ctypes.POINTER(nat.KernelTerm) * n)(*[ctypes.cast(arr, ctypes.POINTER(nat.KernelTerm))] * n)
    c_var = (dp * n)(*[var.ctypes.data_as(dp)] * n)
    c_info = (dp * n)(*[info.ctypes.data_as(dp)] * n)
    c_tol = None if tol is None else np.full(n, tol).ctypes.data_as(dp)
    rc = L.icp_gp_models_many(n, 0, n_pts.ctypes.data_as(ip), c_pts, n_terms.ctypes.data_as(ip), c_terms, mp.ctypes.data_as(ip),
                              rk.ctypes.data_as(ip), c_tol, c_var, None, None, None, c_info, status.ctypes.data_as(ip))
    return rc, status, var, info


def test_the_library_refuses_bad_arguments_before_touching_a_device(pkg):
    """ICP_ERR_INVALID_ARG for the item, nothing written — also on a machine without a GPU, where touching the device would be
    ICP_ERR_DEVICE instead"""
    T = pkg.data.GaussianKernelTerm
    pts = np.arange(21.0).reshape(7, 3) ** 2
    ok = [T(2.0, 30.0)]
    cases = [(pts, ok, 3, 4, None),            # rank > pivots
             (pts, ok, 22, 5, None),           # pivots > 3N
             (np.zeros((100, 3)), ok, 257, 5, None),  # pivots > 256
             (pts, ok, 3, 0, None), (pts, ok, 0, 0, None),
             (pts, ok, 3, 3, 1.0), (pts, ok, 3, 3, -0.5), (pts, ok, 3, 3, np.nan)]
    cases += [(pts, k, 3, 3, None) for k in _bad_terms(pkg)]
    for bad_value in (np.inf, -np.inf, np.nan):
        p = pts.copy()
        p[6, 2] = bad_value
        cases.append((p, ok, 3, 3, None))
    for p, k, m, r, tol in cases:
        rc, status, var, info = _native_call(pkg, p, k, m, r, tol, n_items=2)
        assert rc == -1 and np.all(status == -1), (m, r, tol, k)
        assert np.all(var == 7.0) and np.all(info == 7.0)
    L = pkg._native.lib()
    status = np.full(2, 99, dtype=np.int32)
    assert L.icp_gp_models_many(0, 0, None, None, None, None, None, None, None, None, None, None, None, None, status.ctypes.data_as(pkg._native.c_int_p)) == -1
    assert L.icp_gp_models_many(2, 0, None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert L.icp_gp_models_many(65536, 0, None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert np.all(status == 99)
