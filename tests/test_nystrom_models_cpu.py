"""CPU: Gaussian-process shape models by the Nyström approximation (icp_nystrom_models_many) — the symbol, the Python-side argument
checks with the native library stubbed out, the library's own refusal of bad items before it touches a device, the numpy long form
the GPU tests compare against (tests/nystrom_model_long_form.py) checked against the dense matrices, and data.uniform_mesh_samples."""
import ctypes
import os

import numpy as np
import pytest

import nystrom_model_long_form as NLF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _small(pkg, n_mesh=30, n_samples=12, seed=3):
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n_mesh, 3)) * np.array([60.0, 15.0, 10.0])
    smp = rng.normal(size=(n_samples, 3)) * np.array([60.0, 15.0, 10.0])
    return pts, smp, pkg.data.femur_kernel(pts)


def test_symbol_header_and_signature(pkg):
    nat = pkg._native
    assert hasattr(nat.lib(), "icp_nystrom_models_many")
    header = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    for word in ("icp_nystrom_models_many(", "ICP_NYSTROM_MAX_ROWS 2400", "ICP_NYSTROM_MAX_RANK 256", "ICP_ERR_NOT_CONVERGED"):
        assert word in header
    res, args = nat.SIGNATURES["icp_nystrom_models_many"]
    assert res is ctypes.c_int and len(args) == 17 and args[1] is ctypes.c_int
    assert callable(pkg.nystrom_models) and callable(pkg.nystrom_model) and callable(pkg.data.uniform_mesh_samples)


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def test_nystrom_models_validate_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    T, BS = pkg.data.GaussianKernelTerm, pkg.data.BSplineKernelTerm
    mesh = pkg.data.TriangleMesh(np.arange(21.0).reshape(7, 3) ** 2, np.array([[0, 1, 2]]))
    smp = mesh.points[:4] + 0.5
    ok = [T(2.0, 30.0)]
    inf = smp.copy()
    inf[2, 1] = np.inf
    w7, w4 = np.ones(7), np.ones(4)
    bad = [[],
           [(mesh, smp, ok, 0)], [(mesh, smp, ok, 13)],                      # 1 <= rank <= 3n
           [(mesh, np.zeros((100, 3)), ok, 257)],                            # rank > 256
           [(mesh, np.zeros((801, 3)), ok, 5)],                              # 3n > 2,400
           [(mesh, inf, ok, 3)], [(mesh, smp[:, :2], ok, 3)], [(mesh, smp, ok, 2.5)],
           [(mesh, smp, [], 3)], [(mesh, smp, [T(1.0, -3.0)], 3)], [(mesh, smp, [T(1.0, 10.0, np.diag([1.0, 1.0, -1e-3]))], 3)],
           [(mesh, smp, [BS(1.0, 40)], 3)],
           [(mesh, smp, [T(1.0, 10.0, None, w7)], 3)],                       # weights at the mesh points, none at the samples
           [(mesh, smp, [T(1.0, 10.0, None, w7)], 3, [np.ones(5)])],         # sample weights of the wrong length
           [(mesh, smp, [T(1.0, 10.0)], 3, [w4])],                           # sample weights for a term without weights
           [(mesh, smp, [T(1.0, 10.0, None, w7)], 3, [w4, w4])],
           [(mesh, smp, ok)]]
    for items in bad:
        with pytest.raises(ValueError):
            pkg.nystrom_models(items)
    for kw in (dict(min_variance=-1e-3), dict(min_variance=np.nan), dict(min_variance=[1e-8, 1e-8]), dict(want=("variance", "nonsense"))):
        with pytest.raises(ValueError):
            pkg.nystrom_models([(mesh, smp, ok, 3)], **kw)
    with pytest.raises(AssertionError, match="icp_nystrom_models_many reached"):  # good arguments go through to the library
        pkg.nystrom_model(mesh, smp, [T(1.0, 10.0, None, w7, 0.5, 0), BS(2.0, -3)], 12, [w4, None])


def test_the_library_refuses_bad_items_before_touching_a_device(pkg):
    """past the Python-side checks (NLF.native_call): ICP_ERR_INVALID_ARG for every such item and nothing written — also on a machine
    without a GPU, where touching the device would be ICP_ERR_DEVICE instead"""
    T = pkg.data.GaussianKernelTerm
    pts = np.arange(21.0).reshape(7, 3) ** 2
    smp = pts[:4] + 0.5
    ok = [T(2.0, 30.0)]
    nan = smp.copy()
    nan[2, 1] = np.nan
    inf = pts.copy()
    inf[6, 2] = np.inf
    items = [(pts, np.zeros((801, 3)), ok, 5), (pts, np.zeros((100, 3)), ok, 257), (pts, smp, ok, 13), (pts, nan, ok, 3), (inf, smp, ok, 3),
             (pts, smp, ok, 0), (pts, smp, [], 3), (pts, smp, [T(1.0, 0.0)], 3), (pts, smp, [T(1.0, 10.0)] * 9, 3)]
    rc, status, outs = NLF.native_call(pkg, items)
    assert rc == -1 and np.all(status == -1)
    assert all(np.all(a == 7.0) for o in outs for a in o.values())
    for bad in (-1.0, -1e-300, np.nan, np.inf):
        rc, status, outs = NLF.native_call(pkg, [(pts, smp, ok, 3)] * 2, min_variance=[bad, bad])
        assert rc == -1 and np.all(status == -1) and all(np.all(a == 7.0) for o in outs for a in o.values())
    L, ip = pkg._native.lib(), pkg._native.c_int_p
    status = np.full(2, 99, dtype=np.int32)
    none = [None] * 14
    assert L.icp_nystrom_models_many(0, 0, *none, status.ctypes.data_as(ip)) == -1
    assert L.icp_nystrom_models_many(65536, 0, *none, status.ctypes.data_as(ip)) == -1
    assert L.icp_nystrom_models_many(2, 0, *none, None) == -1
    assert np.all(status == 99)


@pytest.mark.parametrize("k", [1, 7, 20, 36])
def test_long_form_against_the_dense_matrix(pkg, k):
    """Σ_i var_i b_i b_iᵀ = k(X,S) U_k Λ_k⁻¹ U_kᵀ k(S,X) to 1e-12 max|K|; variances descending; the eigenvectors handed in are used"""
    pts, smp, terms = _small(pkg)
    lf = NLF.long_form(pts, smp, terms, k)
    n = len(smp)
    K, Kxs = lf["K"], lf["Kxs"]
    assert np.array_equal(K, K.T) and K.shape == (36, 36) and Kxs.shape == (90, 36)
    assert np.abs(Kxs - NLF.cross(pts, smp, terms)).max() == 0.0
    assert lf["k_eff"] == k and np.all(np.diff(lf["variance"]) <= 0) and lf["basis"].shape == (90, k)
    w, v = lf["eigh_values"], lf["eigh_vectors"]
    assert np.abs(lf["variance"] - w[:k] / n).max() == 0.0
    cov = (lf["basis"] * lf["variance"]) @ lf["basis"].T
    want = Kxs @ (v[:, :k] / w[:k]) @ v[:, :k].T @ Kxs.T
    assert np.abs(cov - want).max() <= 1e-12 * np.abs(K).max()
    flipped = NLF.long_form(pts, smp, terms, k, eigenvalues=w, eigenvectors=-v[:, :k])
    assert np.array_equal(flipped["basis"], -lf["basis"])


def test_long_form_reproduces_the_kernel_matrix_on_its_own_samples(pkg):
    """S = X and k = R: the model's covariance K U Λ⁻¹ Uᵀ K is K itself.  eigh is backward stable at R·2⁻⁵²·|K|, which Λ⁻¹ amplifies by
    λ₁/λ_R at the most: the bound is 10·R·2⁻⁵²·(λ₁/λ_R)·max|K|"""
    pts, _, terms = _small(pkg, n_mesh=14)
    lf = NLF.long_form(pts, pts, terms, 42, min_variance=0.0)
    K, w = lf["K"], lf["eigh_values"]
    assert lf["k_eff"] == 42 and w[-1] > 0
    cov = (lf["basis"] * lf["variance"]) @ lf["basis"].T
    err, bound = np.abs(cov - K).max(), 10 * 42 * EPS * (w[0] / w[-1]) * np.abs(K).max()
    print(f"|cov - K| = {err:.3e} (bound {bound:.3e}, condition {w[0] / w[-1]:.3e})")
    assert err <= bound


def test_long_form_min_variance_drops_the_tail(pkg):
    """duplicated sample points: the kernel matrix is rank-deficient, eigenvalues at rounding level (some negative) do not count"""
    pts, smp, terms = _small(pkg)
    dup = np.concatenate([smp, smp[:5]])
    lf = NLF.long_form(pts, dup, terms, 51)
    assert lf["k_eff"] == 36 and np.all(np.isfinite(lf["basis"])) and lf["basis"].shape == (90, 36)
    assert np.abs(lf["eigh_values"][36:]).max() <= 51 * EPS * lf["eigh_values"][0]


def test_long_form_general_terms_reduce_to_plain_ones(pkg):
    """a Gaussian term with weights 1 and no mirror goes through the general expressions: the plain term's matrix to rounding"""
    pts, smp, terms = _small(pkg)
    T = pkg.data.GaussianKernelTerm
    general = [T(t.scale, t.sigma, t.A, np.ones(len(pts))) for t in terms]
    sw = [np.ones(len(smp))] * len(terms)
    a = NLF.long_form(pts, smp, terms, 5)
    b = NLF.long_form(pts, smp, general, 5, sample_weights=sw)
    assert np.abs(a["K"] - b["K"]).max() <= 4 * EPS * np.abs(a["K"]).max()
    assert np.abs(a["Kxs"] - b["Kxs"]).max() <= 4 * EPS * np.abs(a["K"]).max()


def _two_triangles(pkg):
    """two triangles of areas 1 and 3"""
    pts = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 5.0], [3.0, 0.0, 5.0], [0.0, 2.0, 5.0]])
    return pkg.data.TriangleMesh(pts, np.array([[0, 1, 2], [3, 4, 5]]))


def test_uniform_mesh_samples(pkg):
    mesh = _two_triangles(pkg)
    p = mesh.points
    area = [0.5 * np.linalg.norm(np.cross(p[c[1]] - p[c[0]], p[c[2]] - p[c[0]])) for c in mesh.cells]
    assert abs(area[0] - 1.0) <= 1e-12 and abs(area[1] - 3.0) <= 1e-12
    n = 4000
    pts, tri = pkg.data.uniform_mesh_samples(mesh, n, seed=5, return_cells=True)
    again = pkg.data.uniform_mesh_samples(mesh, n, seed=5)
    other = pkg.data.uniform_mesh_samples(mesh, n, seed=6)
    assert pts.shape == (n, 3) and tri.shape == (n,) and np.array_equal(pts, again) and not np.array_equal(pts, other)
    # every point lies on its triangle: barycentric coordinates in [0, 1] that sum to 1 and give the point back
    a, b, c = p[mesh.cells[tri, 0]], p[mesh.cells[tri, 1]], p[mesh.cells[tri, 2]]
    for i in range(0, n, 37):
        sol, res, _, _ = np.linalg.lstsq(np.stack([b[i] - a[i], c[i] - a[i]], axis=1), pts[i] - a[i], rcond=None)
        assert sol.min() >= -1e-12 and sol.sum() <= 1.0 + 1e-12
        assert np.abs(a[i] + sol[0] * (b[i] - a[i]) + sol[1] * (c[i] - a[i]) - pts[i]).max() <= 1e-12
    # the counts follow area: binomial(n, 1/4), within 5 standard deviations
    count0 = int((tri == 0).sum())
    sd = np.sqrt(n * 0.25 * 0.75)
    print(f"triangle 0 drew {count0} of {n} (expected {n // 4}, sd {sd:.1f})")
    assert abs(count0 - n * 0.25) <= 5 * sd
    femur, _, _ = pkg.data.load_femur_mesh("femur_reference")
    s = pkg.data.uniform_mesh_samples(femur, 100, seed=1)
    assert s.shape == (100, 3) and np.all(s.min(axis=0) >= femur.points.min(axis=0)) and np.all(s.max(axis=0) <= femur.points.max(axis=0))
    for bad in (0, 2.5):
        with pytest.raises(ValueError):
            pkg.data.uniform_mesh_samples(femur, bad)
