"""CPU: general kernel terms of Gaussian-process shape models (icp_gp_models_general_many, icp_region_weights_many) — the
numpy long form the GPU tests compare against (tests/face_kernel_long_form.py) checked against the dense kernel matrix and hand-computed
values, the face kernel's terms, the Python-side argument checks with the native library stubbed out, and the real library's refusal
of every bad argument before it touches a device."""
import ctypes
import os

import numpy as np
import pytest

import face_kernel_long_form as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def test_symbols_header_signatures_and_struct_size(pkg):
    nat = pkg._native
    header = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    for word in ("icp_gp_models_general_many(", "icp_region_weights_many(", "icp_kernel_term_general", "ICP_KERNEL_GAUSSIAN 0",
                 "ICP_KERNEL_BSPLINE3 1", "struct_size", "mirror_gain", "DEVIATION"):
        assert word in header
    for name in ("icp_gp_models_general_many", "icp_region_weights_many"):
        assert hasattr(nat.lib(), name)
    res, args = nat.SIGNATURES["icp_gp_models_general_many"]
    assert res is ctypes.c_int and len(args) == 15 and args[5] is ctypes.POINTER(ctypes.POINTER(nat.KernelTermGeneral))
    res, args = nat.SIGNATURES["icp_region_weights_many"]
    assert res is ctypes.c_int and len(args) == 9
    g = nat.KernelTermGeneral
    assert ctypes.sizeof(g) == 120 and ctypes.sizeof(nat.KernelTerm) == 88
    assert [getattr(g, f).offset for f, _ in g._fields_] == [0, 4, 8, 16, 24, 28, 32, 40, 112]
    assert (nat.KERNEL_GAUSSIAN, nat.KERNEL_BSPLINE3) == (0, 1)
    for fn in (pkg.region_weights, pkg.face_kernel, pkg.data.BSplineKernelTerm, pkg.data.FaceMask):
        assert callable(fn)


def test_gaussian_term_keeps_its_positional_form_and_gains_three_fields(pkg):
    T = pkg.data.GaussianKernelTerm
    t = T(2.0, 30.0)
    assert (t.scale, t.sigma, t.weights, t.mirror_gain, t.mirror_axis, t.plain) == (2.0, 30.0, None, 0.0, 0, True) and np.array_equal(t.A, np.eye(3))
    t = T(2.0, 30.0, np.diag([1.0, 2.0, 3.0]), np.ones(4), 0.5, 1)
    assert not t.plain and t.mirror_axis == 1 and t.weights.dtype == np.float64
    assert not T(2.0, 30.0, weights=np.ones(3)).plain
    x, y = np.array([1.0, 2.0, 3.0]), np.array([2.0, 2.0, 5.0])
    assert np.array_equal(T(2.0, 30.0)(x, y), 2.0 * np.exp(-(5.0 / 900.0)) * np.eye(3))
    b = pkg.data.BSplineKernelTerm(4.0, -2)
    assert (b.scale, b.level, b.weights, b.mirror_gain, b.mirror_axis) == (4.0, -2, None, 0.0, 0) and np.array_equal(b.A, np.eye(3))
    with pytest.raises(ValueError):
        pkg.data.BSplineKernelTerm(4.0, -2.5)


def test_beta_and_the_one_dimensional_sums_by_hand():
    assert np.array_equal(F.beta3([0.0, 1.0, -1.0, 2.0, -2.0, 2.5, 0.5, -1.5]),
                          [2.0 / 3.0, 1.0 / 6.0, 1.0 / 6.0, 0.0, 0.0, 0.0, (2.0 / 3.0 - 0.25) + 0.0625, ((1.0 / 6.0 * 0.5) * 0.5) * 0.5])
    b0, b1 = 2.0 / 3.0, 1.0 / 6.0
    # on lattice nodes: S(0, 0) = beta(1)^2 + beta(0)^2 + beta(1)^2 (k = -2 and 2 add exact zeros); S(0, 1): k = 0 and 1; S(0, 2): k = 1;
    # S(0, 3): k = 1 .. 2 holds only zero products; S(0, 4): k = 2 alone, zero; S(0, 5): an empty range
    assert F.spline_sum(0.0, 0.0) == (b1 * b1 + b0 * b0) + b1 * b1 == 0.5
    assert F.spline_sum(0.0, 1.0) == (b1 * b0 + b0 * b1) == F.spline_sum(1.0, 0.0)
    assert F.spline_sum(0.0, 2.0) == b1 * b1
    assert F.spline_sum(0.0, 3.0) == 0.0 and F.spline_sum(0.0, 4.0) == 0.0 and F.spline_sum(0.0, 5.0) == 0.0
    # negative coordinates through ceil and floor: invariant under a shift by whole cells and under mirroring both arguments
    assert F.spline_sum(-3.0, -2.0) == F.spline_sum(0.0, 1.0) and F.spline_sum(-8.0, -8.0) == 0.5
    for u, v in ((-0.3, 1.2), (-2.7, -1.1), (5.25, 3.5)):
        assert abs(F.spline_sum(u, v) - F.spline_sum(-u, -v)) <= 4 * EPS and abs(F.spline_sum(u, v) - F.spline_sum(v, u)) <= 4 * EPS
        k = np.arange(-10.0, 11.0)
        assert abs(F.spline_sum(u, v) - (F.beta3(u - k) * F.beta3(v - k)).sum()) <= 4 * EPS
    # the partition of unity of the cubic B-spline
    assert abs(F.beta3(0.3 - np.arange(-3.0, 4.0)).sum() - 1.0) <= 4 * EPS


def test_base_kernel_on_the_lattice(pkg):
    """lat27 at level -2 (c = 1/4): the points are the nodes -2, 0, 2; neighbours are two cells apart"""
    T = pkg.data.BSplineKernelTerm
    lat = F.lat27()
    b = F.base_kernel(T(1.0, -2), lat, lat[13])  # the centre (0, 0, 0)
    assert b[13] == (0.5 * 0.5) * 0.5 and b[14] == (0.5 * 0.5) * (1.0 / 36.0) and b[0] == ((1.0 / 36.0) * (1.0 / 36.0)) * (1.0 / 36.0)
    b = F.base_kernel(T(1.0, 0), lat, lat[13])   # level 0: eight cells apart, nothing overlaps
    assert b[13] == 0.125 and np.count_nonzero(b) == 1
    g = pkg.data.GaussianKernelTerm(1.0, 8.0)
    assert np.array_equal(F.base_kernel(g, lat, lat[13]), np.exp(-((lat ** 2).sum(axis=1) / 64.0)))


def test_plain_terms_have_the_plain_long_forms_bits(pkg):
    import gp_model_long_form as LF
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(30, 3)) * np.array([60.0, 15.0, 10.0])
    terms = pkg.data.femur_kernel(pts)
    rows = [0, 7, 44, 89]
    assert np.array_equal(F.kernel_columns(pts, terms, rows), LF.kernel_columns(pts, terms, rows))
    assert np.array_equal(F.kernel_diagonal(pts, terms), LF.kernel_diagonal(30, terms))


CASES = [("sym11", 11, 0.0), ("jit11", 11, 1.5), ("jit6", 6, 1.5)]


@pytest.mark.parametrize("name,g,jitter", CASES)
@pytest.mark.parametrize("mask", ["all", "part"])
def test_face_kernel_matrix_is_symmetric_positive_semi_definite(pkg, name, g, jitter, mask):
    pts = F.patch(g, jitter)
    terms = F.face_terms(pkg.data.BSplineKernelTerm, pts, F.masks(pts)[mask])
    K = F.dense(pts, terms)
    kmax = np.abs(K).max()
    assert np.abs(K - K.T).max() <= 1e-14 * kmax  # (two summation orders of at most five products per dimension)
    assert np.linalg.eigvalsh(0.5 * (K + K.T)).min() >= -1e-12 * kmax
    assert np.array_equal(F.kernel_diagonal(pts, terms), np.diag(K))
    if name == "sym11" and mask == "all":
        assert np.array_equal(pts[:, 0].reshape(11, 11)[5], np.zeros(11))  # a column of the grid on the mirror plane
        assert np.abs(np.diag(K).reshape(-1, 3)[:, 0].reshape(11, 11)[5]).max() < 0.31 * kmax  # there x rows keep 1 - 0.7 of the value


@pytest.mark.parametrize("name,g,jitter,m", [("jit6", 6, 1.5, 5), ("jit6", 6, 1.5, 64), ("jit6", 6, 1.5, 65), ("jit11", 11, 1.5, 200),
                                              ("sym11", 11, 0.0, 256)])
def test_long_form_against_the_dense_matrix(pkg, name, g, jitter, m):
    """DESIGN 5.13's CPU bounds: the trace identity to 1e-14 relative, |K - B diag(var) B^T|_ab <= sqrt(res_a res_b) + 1e-9 max|K|"""
    pts = F.patch(g, jitter)
    terms = F.face_terms(pkg.data.BSplineKernelTerm, pts, F.masks(pts)["part"])
    K = F.dense(pts, terms)
    lf = F.long_form(pts, terms, m)
    n = len(pts)
    assert lf["m_eff"] == m and len(set(lf["pivots"].tolist())) == m and np.all(lf["step_taken"] == lf["step_max"])
    assert abs(lf["trace"] - np.trace(K)) <= 1e-14 * np.trace(K)
    assert abs(lf["trace"] - (lf["theta"].sum() + lf["residual"].sum())) <= 1e-14 * lf["trace"]
    assert lf["residual"].min() >= -m * EPS * np.diag(K).max()
    B = lf["basis"]
    assert np.abs(B.T @ B / n - np.eye(m)).max() <= 1e3 * EPS * lf["variance"][0] / lf["variance"][-1]
    res = np.maximum(lf["residual"], 0.0)
    err = np.abs(K - (B * lf["variance"]) @ B.T)
    assert np.all(err <= np.sqrt(res[:, None] * res[None, :]) + 1e-9 * np.abs(K).max())


def test_lattice_mesh_full_rank_and_numerical_rank(pkg):
    T = pkg.data.BSplineKernelTerm
    lat = F.lat27()
    for levels in (F.FACE_LEVELS, ((-2, 4.0),), ((0, 1.0),)):
        terms = F.face_terms(T, lat, None, 0.7, levels)
        lf = F.long_form(lat, terms, 81)
        assert lf["m_eff"] == 81
        K = F.dense(lat, terms)
        assert np.abs(K - (lf["basis"] * lf["variance"]) @ lf["basis"].T).max() <= 1e-9 * np.abs(K).max()
    terms = F.face_terms(T, lat, None, 1.0)
    d = F.kernel_diagonal(lat, terms)
    assert int((d == 0.0).sum()) == 9  # the x rows of the nine points on the mirror plane
    lf = F.long_form(lat, terms, 81)
    assert lf["m_eff"] == 45 and lf["residual"].max() <= 81 * EPS * d.max() and np.all(d[lf["pivots"]] > 0)
    e0 = np.zeros((3, 3))
    e0[0, 0] = 1.0
    assert np.array_equal(F.kernel_diagonal(F.ONE_POINT, [T(1.0, -2, e0, None, 1.0, 0)]), np.zeros(3))


def test_mixed_terms_weights_and_an_axis_other_than_x(pkg):
    pts = F.patch(6, 1.5)
    w = F.region_weights(pts, pts[pts[:, 1] > 0.0])
    terms = [pkg.data.GaussianKernelTerm(3.0, 50.0, np.diag([1.0, 2.0, 1.0]), w, 0.5, 1), pkg.data.BSplineKernelTerm(2.0, -5)]
    K = F.dense(pts, terms)
    assert np.abs(K - K.T).max() <= 1e-14 * np.abs(K).max() and np.linalg.eigvalsh(0.5 * (K + K.T)).min() >= -1e-12 * np.abs(K).max()
    # one entry by hand: rows (vertex 3, y) and (vertex 20, y)
    x, y = pts[3], pts[20]
    ym = y * np.array([1.0, -1.0, 1.0])
    g = lambda a, b: np.exp(-(((a - b) ** 2).sum() / 2500.0))  # noqa: E731
    c = 2.0 ** -5
    bs = np.prod([F.spline_sum(x[i] * c, y[i] * c) for i in range(3)])
    want = 3.0 * w[3] * w[20] * 2.0 * (g(x, y) - 0.5 * g(x, ym)) + 2.0 * bs
    assert abs(K[3 * 3 + 1, 3 * 20 + 1] - want) <= 1e-13 * np.abs(K).max()
    want_x = 3.0 * w[3] * w[20] * (g(x, y) + 0.5 * g(x, ym)) + 2.0 * bs
    assert abs(K[3 * 3, 3 * 20] - want_x) <= 1e-13 * np.abs(K).max() and K[3 * 3, 3 * 20 + 1] == 0.0


def test_region_weights_long_form():
    pts = F.patch(11, 1.5)
    reg = pts[pts[:, 0] >= -20.0]
    w = F.region_weights(pts, reg)
    assert np.all(w[pts[:, 0] >= -20.0] == 1.0) and np.all(w[pts[:, 0] < -20.0] < 1.0) and np.all(w > 0.0)
    i = int(np.argmin(pts[:, 0]))
    d2 = ((pts[i] - reg) ** 2).sum(axis=1).min()
    assert abs(w[i] - np.exp(-d2 / 1600.0)) <= 4 * EPS


def test_face_kernel_terms(pkg):
    pts = F.patch(6, 1.5)
    mesh = pkg.data.TriangleMesh(pts, F.grid_cells(6))
    terms = pkg.face_kernel(mesh)  # the mask of 3 everywhere: no device call
    assert [(t.level, t.scale) for t in terms] == [(-6, 128.0), (-5, 64.0), (-4, 32.0), (-3, 10.0), (-2, 4.0)]
    assert pkg.data.FACE_KERNEL_LEVELS == F.FACE_LEVELS
    for t in terms:
        assert isinstance(t, pkg.data.BSplineKernelTerm) and np.array_equal(t.A, np.eye(3)) and t.weights is None
        assert (t.mirror_gain, t.mirror_axis) == (0.7, 0)
    mask = pkg.data.FaceMask(F.masks(pts)["part"])
    assert np.array_equal(mask.region(mesh, -4), pts) and np.array_equal(mask.region(mesh, -3), pts[pts[:, 0] >= -20.0])
    with pytest.raises(ValueError):
        mask.region(mesh, 4)
    with pytest.raises(ValueError):
        pkg.data.FaceMask(np.zeros(5, dtype=np.int32)).region(mesh, 0)


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def _bad_general_terms(pkg, n):
    G, S = pkg.data.GaussianKernelTerm, pkg.data.BSplineKernelTerm
    couple = np.array([[1.0, 0.5, 0.0], [0.5, 1.0, 0.0], [0.0, 0.0, 1.0]])
    w = np.ones(n)
    neg, nan, zero = w.copy(), w.copy(), np.zeros(n)
    neg[2], nan[1] = -1e-9, np.nan
    return [[S(0.0, -2)], [S(np.inf, -2)], [S(1.0, 33)], [S(1.0, -33)],
            [S(1.0, 30)], [S(1.0, 23)],                     # |coordinate| 2^level >= 2^31 on the tests' points (up to 400)
            [S(1.0, -2, np.diag([1.0, 1.0, -1.0]))], [S(1.0, -2, np.zeros((3, 3)))],
            [S(1.0, -2, None, None, 1.5)], [S(1.0, -2, None, None, -0.1)], [S(1.0, -2, None, None, np.nan)],
            [S(1.0, -2, None, None, 0.5, 3)], [S(1.0, -2, None, None, 0.0, -1)],
            [S(1.0, -2, couple, None, 0.5, 0)], [S(1.0, -2, couple, None, 0.5, 1)],
            [G(1.0, 10.0, couple, None, 1.0, 0)], [G(1.0, 0.0, None, None, 0.5)], [G(-1.0, 10.0, None, w)],
            [S(1.0, -2, None, neg)], [S(1.0, -2, None, nan)], [S(1.0, -2, None, zero)], [S(1.0, -2, None, np.ones(n + 1))],
            [G(1.0, 10.0), S(1.0, -2, None, zero)], [S(1.0, -2)] * 9]


def test_general_terms_validate_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    G, S = pkg.data.GaussianKernelTerm, pkg.data.BSplineKernelTerm
    mesh = pkg.data.TriangleMesh(np.arange(21.0).reshape(7, 3) ** 2, np.array([[0, 1, 2]]))
    for k in _bad_general_terms(pkg, 7):
        with pytest.raises(ValueError):
            pkg.gp_models([mesh], [k], 3)
    with pytest.raises(ValueError):
        pkg.gp_models([mesh], [[S(1.0, -2), "a term"]], 3)
    with pytest.raises(ValueError):
        pkg.gp_models([mesh], [S(1.0, -2)], 22)  # the limits of the plain call hold
    couple_other = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.5], [0.0, 0.5, 1.0]])  # couples y and z only: fine about axis 0
    good = [[S(1.0, -2)], [S(1.0, 22)],  # (the largest coordinate is 400: 400 · 2^22 < 2^31 <= 400 · 2^23)
            [S(1.0, -32)], [S(1.0, -2, couple_other, np.ones(7), 1.0, 0)], [G(1.0, 10.0, None, np.ones(7))],
            [G(1.0, 10.0, None, None, 0.5, 2)], [G(1.0, 10.0), S(1.0, -3)], [S(1.0, -2, np.eye(3), None, 0.0, 2)]]
    for k in good:
        with pytest.raises(AssertionError, match="icp_gp_models_general_many reached"):
            pkg.gp_models([mesh], [k], 3)
    with pytest.raises(AssertionError, match="icp_gp_models_general_many reached"):  # one general term anywhere in the call
        pkg.gp_models([mesh, mesh], [[G(1.0, 10.0)], [S(1.0, -2)]], 3)
    with pytest.raises(AssertionError, match="icp_gp_models_many reached"):          # all plain: the call as it was
        pkg.gp_models([mesh, mesh], [[G(1.0, 10.0)], [G(2.0, 5.0, np.diag([1.0, 0.0, 2.0]))]], 3)
    with pytest.raises(AssertionError, match="icp_gp_models_many reached"):
        pkg.gp_model(mesh, [G(1.0, 10.0, None, None, 0.0, 2)], 3)                     # a gain of zero is plain whatever the axis
    # the weights call
    pts = mesh.points
    inf = pts.copy()
    inf[2, 0] = np.inf
    for kw in (dict(points=pts, region_points=np.zeros((0, 3))), dict(points=pts, region_points=pts, stddev=0.0),
               dict(points=pts, region_points=pts, stddev=-1.0), dict(points=pts, region_points=pts, stddev=np.nan),
               dict(points=inf, region_points=pts), dict(points=pts, region_points=inf), dict(points=pts[:, :2], region_points=pts),
               dict(points=[pts, pts], region_points=[pts]), dict(points=[pts, pts], region_points=[pts, pts], stddev=[1.0]),
               dict(points=[], region_points=[])):
        with pytest.raises(ValueError):
            pkg.region_weights(**kw)
    with pytest.raises(AssertionError, match="icp_region_weights_many reached"):
        pkg.region_weights(pts, pts[:2])
    with pytest.raises(AssertionError, match="icp_region_weights_many reached"):
        pkg.region_weights([pts, pts], [pts[:2], pts[3:]], [40.0, 10.0])
    with pytest.raises(AssertionError, match="icp_region_weights_many reached"):
        pkg.face_kernel(mesh, pkg.data.FaceMask(np.array([3, 3, 3, -4, -4, 3, 3], dtype=np.int32)))
    assert len(pkg.face_kernel(mesh)) == 5  # the mask of 3 everywhere reaches nothing


def _general_call(pkg, pts, terms, n_pivots=3, rank=3, tol=None, n_items=2, struct_size=None, kind=None):
    """the same item n_items times straight through ctypes -> (rc, status, the output arrays)"""
    nat, L = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    arr = (nat.KernelTermGeneral * max(len(terms), 1))()
    keep = []
    for t, k in enumerate(terms):
        gauss = hasattr(k, "sigma")
        arr[t].struct_size = ctypes.sizeof(nat.KernelTermGeneral) if struct_size is None else struct_size
        arr[t].kind = (0 if gauss else 1) if kind is None else kind
        arr[t].scale, arr[t].sigma, arr[t].level = k.scale, (k.sigma if gauss else 0.0), (0 if gauss else k.level)
        arr[t].mirror_axis, arr[t].mirror_gain = k.mirror_axis, k.mirror_gain
        arr[t].A[:] = np.asarray(k.A, dtype=np.float64).reshape(-1).tolist()
        if k.weights is not None:
            keep.append(np.ascontiguousarray(k.weights, dtype=np.float64))
            arr[t].weights = keep[-1].ctypes.data_as(dp)
    n = n_items
    i32 = lambda v: np.full(n, v, dtype=np.int32)  # noqa: E731
    n_pts, n_terms, mp, rk = i32(pts.shape[0]), i32(len(terms)), i32(n_pivots), i32(rank)
    var, info = np.full(300, 7.0), np.full(4, 7.0)
    status = np.full(n, 99, dtype=np.int32)
    c_pts = (dp * n)(*[pts.ctypes.data_as(dp)] * n)
    c_terms = (ctypes.POINTER(nat.KernelTermGeneral) * n)(*[ctypes.cast(arr, ctypes.POINTER(nat.KernelTermGeneral))] * n)
    c_var = (dp * n)(*[var.ctypes.data_as(dp)] * n)
    c_info = (dp * n)(*[info.ctypes.data_as(dp)] * n)
    c_tol = None if tol is None else np.full(n, tol).ctypes.data_as(dp)
    rc = L.icp_gp_models_general_many(n, 0, n_pts.ctypes.data_as(ip), c_pts, n_terms.ctypes.data_as(ip), c_terms, mp.ctypes.data_as(ip),
                                      rk.ctypes.data_as(ip), c_tol, c_var, None, None, None, c_info, status.ctypes.data_as(ip))
    return rc, status, var, info


def test_the_library_refuses_bad_general_arguments_before_touching_a_device(pkg):
    """ICP_ERR_INVALID_ARG for the item, nothing written — also on a machine without a GPU, where touching the device would be
    ICP_ERR_DEVICE instead"""
    G, S = pkg.data.GaussianKernelTerm, pkg.data.BSplineKernelTerm
    pts = np.arange(21.0).reshape(7, 3) ** 2
    ok = [S(2.0, -3)]
    cases = [dict(terms=k) for k in _bad_general_terms(pkg, 7) if not (k[0].weights is not None and len(k[0].weights) != 7)]
    cases += [dict(terms=ok, struct_size=0), dict(terms=ok, struct_size=88), dict(terms=ok, struct_size=128), dict(terms=ok, kind=2),
              dict(terms=ok, kind=-1), dict(terms=ok, n_pivots=3, rank=4), dict(terms=ok, n_pivots=22, rank=5), dict(terms=ok, tol=1.0),
              dict(terms=[G(1.0, np.inf)]), dict(terms=[])]
    for kw in cases:
        rc, status, var, info = _general_call(pkg, pts, **kw)
        assert rc == -1 and np.all(status == -1), kw
        assert np.all(var == 7.0) and np.all(info == 7.0)
    for bad_value in (np.inf, np.nan):
        p = pts.copy()
        p[6, 2] = bad_value
        rc, status, var, info = _general_call(pkg, p, ok)
        assert rc == -1 and np.all(status == -1) and np.all(var == 7.0)
    big = pts.copy()
    big[0, 0] = 2.0 ** 33  # level -3: 2^30 is in range; level -2: 2^31 is not
    assert _general_call(pkg, big, [S(1.0, -2)])[0] == -1
    L, ip = pkg._native.lib(), pkg._native.c_int_p
    status = np.full(2, 99, dtype=np.int32)
    assert L.icp_gp_models_general_many(0, 0, None, None, None, None, None, None, None, None, None, None, None, None, status.ctypes.data_as(ip)) == -1
    assert L.icp_gp_models_general_many(2, 0, None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert np.all(status == 99)


def test_the_library_refuses_bad_region_arguments_before_touching_a_device(pkg):
    nat, L = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    pts = np.arange(21.0).reshape(7, 3) ** 2
    inf = pts.copy()
    inf[4, 1] = np.inf

    def call(p, reg, n_reg, sd, n_pts=7):
        out = np.full(7, 7.0)
        status = np.full(2, 99, dtype=np.int32)
        two = lambda a: (dp * 2)(*[a.ctypes.data_as(dp)] * 2)  # noqa: E731
        rc = L.icp_region_weights_many(2, 0, np.full(2, n_pts, dtype=np.int32).ctypes.data_as(ip), two(p),
                                       np.full(2, n_reg, dtype=np.int32).ctypes.data_as(ip), two(reg), np.full(2, sd).ctypes.data_as(dp), two(out),
                                       status.ctypes.data_as(ip))
        return rc, status, out
    for p, reg, n_reg, sd, n_pts in ((pts, pts, 0, 40.0, 7), (pts, pts, -1, 40.0, 7), (pts, pts, 3, 0.0, 7), (pts, pts, 3, -2.0, 7),
                                     (pts, pts, 3, np.nan, 7), (pts, pts, 3, np.inf, 7), (inf, pts, 3, 40.0, 7), (pts, inf, 7, 40.0, 7),
                                     (pts, pts, 3, 40.0, 0)):
        rc, status, out = call(p, reg, n_reg, sd, n_pts)
        assert rc == -1 and np.all(status == -1) and np.all(out == 7.0), (n_reg, sd, n_pts)
    status = np.full(2, 99, dtype=np.int32)
    assert L.icp_region_weights_many(0, 0, None, None, None, None, None, None, status.ctypes.data_as(ip)) == -1
    assert L.icp_region_weights_many(2, 0, None, None, None, None, None, None, None) == -1
    assert np.all(status == 99)
