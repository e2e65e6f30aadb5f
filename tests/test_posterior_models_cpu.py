"""CPU: posterior shape models from correspondences (icp_posterior_models_many) — the binding, the Python-side argument checks with the
native library stubbed out, landmark_correspondences on the femur fixtures, and the numpy long form the GPU tests compare against
(tests/posterior_long_form.py) checked against the textbook Gaussian-process posterior."""
import ctypes
import os
import types

import numpy as np
import pytest

import posterior_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_header_and_signature(pkg):
    nat = pkg._native
    L = nat.lib()
    assert hasattr(L, "icp_posterior_models_many")
    header = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    assert "icp_posterior_models_many(" in header
    for word in ("ICP_POSTERIOR_MODELS_CHUNK_BYTES", "ICP_POSTERIOR_MODELS_GROUP", "ICP_POSTERIOR_MODELS_SLOT_BYTES", "icp_model_desc"):
        assert word in header
    res, args = nat.SIGNATURES["icp_posterior_models_many"]
    pp = ctypes.POINTER(nat.c_double_p)
    assert res is ctypes.c_int and len(args) == 13
    assert args[0] is ctypes.c_int32 and args[1] is ctypes.POINTER(ctypes.c_void_p) and args[2] is nat.c_int_p
    assert args[3] is ctypes.POINTER(nat.c_int_p) and all(a is pp for a in args[4:12]) and args[12] is nat.c_int_p
    assert callable(pkg.posterior_models) and callable(pkg.IcpContext.posterior) and callable(pkg.data.landmark_correspondences)


def test_without_a_context_the_native_call_refuses(pkg):
    """null contexts and bad sizes: ICP_ERR_INVALID_ARG, nothing written, no crash"""
    nat, L = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    n_obs = np.array([1, 1], dtype=np.int32)
    ids = np.zeros(1, dtype=np.int32)
    pts, s2, out = np.zeros(3), np.ones(1), np.full(8, 7.0)
    status = np.full(2, 99, dtype=np.int32)
    c_ctx = (ctypes.c_void_p * 2)(None, None)
    c_ids = (ip * 2)(ids.ctypes.data_as(ip), ids.ctypes.data_as(ip))
    two = lambda a: (dp * 2)(a.ctypes.data_as(dp), a.ctypes.data_as(dp))  # noqa: E731
    call = lambda n, ctx: L.icp_posterior_models_many(n, ctx, n_obs.ctypes.data_as(ip), c_ids, two(pts), two(s2), None, two(out), None, None,  # noqa: E731
                                                      None, None, status.ctypes.data_as(ip))
    assert call(2, c_ctx) == -1 and call(0, c_ctx) == -1 and call(65536, c_ctx) == -1 and call(2, None) == -1
    assert L.icp_posterior_models_many(2, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert np.all(out == 7.0) and np.all(status == 99)


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def test_posterior_models_validate_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    r, N = 5, 7
    ctx = types.SimpleNamespace(rank=r, N=N, h=None, model=None)
    ids, pts = np.array([0, 3, 3]), np.zeros((3, 3))
    cov = np.broadcast_to(np.eye(3), (3, 3, 3)).copy()
    bad = [
        dict(vertex_ids=[], points=[]),                                              # no items
        dict(vertex_ids=[ids], points=[pts]),                                        # neither noise form
        dict(vertex_ids=[ids], points=[pts], sigma2=[1.0], covariances=[cov]),       # both
        dict(vertex_ids=[ids], points=[pts], sigma2=[0.0]),                          # sigma2 <= 0
        dict(vertex_ids=[ids], points=[pts], sigma2=[np.nan]),
        dict(vertex_ids=[ids], points=[pts[:2]], sigma2=[1.0]),                      # shapes
        dict(vertex_ids=[ids], points=[pts], covariances=[cov[:2]]),
        dict(vertex_ids=[np.array([0, N])], points=[pts[:2]], sigma2=[1.0]),         # id out of range
        dict(vertex_ids=[np.array([-1])], points=[pts[:1]], sigma2=[1.0]),
        dict(vertex_ids=[np.array([], dtype=np.int32)], points=[pts[:0]], sigma2=[1.0]),  # no observation
        dict(vertex_ids=[ids, ids], points=[pts, pts], sigma2=[1.0]),                # one noise entry per item
        dict(vertex_ids=[ids], points=[pts], sigma2=[1.0], want=("alpha", "nonsense")),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            pkg.posterior_models(ctx, **kw)
    inf = pts.copy()
    inf[1, 2] = np.inf
    with pytest.raises(ValueError):
        pkg.posterior_models(ctx, [ids], [inf], sigma2=[1.0])
    nan_cov = cov.copy()
    nan_cov[0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        pkg.posterior_models(ctx, [ids], [pts], covariances=[nan_cov])
    with pytest.raises(ValueError):  # one context per item, or one for all
        pkg.posterior_models([ctx, ctx], [ids], [pts], sigma2=[1.0])
    with pytest.raises(ValueError):  # IcpContext.posterior goes through the same checks
        pkg.IcpContext.posterior(ctx, ids, pts)


def test_landmark_correspondences_on_the_femur_fixtures(pkg):
    model = pkg.data.load_femur_model(50)
    _, names_r, lm_r = pkg.data.load_femur_mesh("femur_reference")
    _, names_t, lm_t = pkg.data.load_femur_mesh("femur_target")
    assert names_r == names_t
    ids, pts = pkg.data.landmark_correspondences(model, lm_r, lm_t)
    assert ids.dtype == np.int32 and ids.shape == (len(names_r),) and pts.shape == (len(names_r), 3)
    assert ids.min() >= 0 and ids.max() < model.n_points
    assert np.array_equal(pts, np.asarray(lm_t, dtype=np.float64))
    d_all = np.linalg.norm(model.ref_points[None, :, :] - np.asarray(lm_r, dtype=np.float64)[:, None, :], axis=2)
    assert np.allclose(d_all[np.arange(len(ids)), ids], d_all.min(axis=1), rtol=0, atol=1e-12)
    # ties go to the lowest index: a model whose vertices 2 and 5 coincide, and a landmark midway between two others
    ref = np.array([[0.0, 0, 0], [4, 0, 0], [1, 1, 1], [0, 4, 0], [2, 0, 0], [1, 1, 1], [-2, 0, 0]])
    tiny = types.SimpleNamespace(ref_points=ref)
    ids, _ = pkg.data.landmark_correspondences(tiny, [[1, 1, 1.25], [3, 0, 0], [-1, 0, 0]], np.zeros((3, 3)))
    assert ids.tolist() == [2, 1, 0]
    with pytest.raises(ValueError):
        pkg.data.landmark_correspondences(tiny, np.zeros((2, 3)), np.zeros((3, 3)))


def _small_model(pkg, seed=5, N=12, r=5):
    rng = np.random.default_rng(seed)
    basis, _ = np.linalg.qr(rng.normal(size=(3 * N, r)))
    cells = np.array([[i, (i + 1) % N, (i + 2) % N] for i in range(N)], dtype=np.int32)
    return pkg.data.StatisticalMeshModel(rng.normal(size=(N, 3)), cells, 0.1 * rng.normal(size=(N, 3)), basis,
                                         np.sort(rng.uniform(0.5, 9.0, size=r))[::-1])


@pytest.mark.parametrize("sigma2", [1.0, 0.1, 0.01])
def test_long_form_is_the_textbook_posterior(pkg, sigma2):
    """isotropic noise: Q M⁻¹ Qᵀ = K − K_xo (K_oo + σ²I)⁻¹ K_ox and μ + Qα = μ + K_xo (K_oo + σ²I)⁻¹ (y − m_o), K = Q Qᵀ"""
    model = _small_model(pkg)
    rng = np.random.default_rng(11)
    ids = np.array([3, 7, 7, 0, 10])  # (a repeat, as Scalismo's regression allows)
    y = model.ref_points[ids] + rng.normal(size=(5, 3))
    lf = LF.long_form(model, ids, y, sigma2=sigma2)
    Q = lf["Q"]
    K = Q @ Q.T
    rows = (3 * ids[:, None] + np.arange(3)[None, :]).reshape(-1)
    G = np.linalg.inv(K[np.ix_(rows, rows)] + sigma2 * np.eye(rows.size))
    post = K - K[:, rows] @ G @ K[rows, :]
    got = Q @ lf["Minv"] @ Q.T
    assert np.abs(got - post).max() <= 1e-10 * max(1.0, np.abs(post).max())
    e = ((y - model.ref_points[ids]) - model.mean_def[ids]).reshape(-1)
    mean = model.mean_def + (K[:, rows] @ G @ e).reshape(-1, 3)
    assert np.abs(lf["mean"] - mean).max() <= 1e-10 * max(1.0, np.abs(mean).max())
    # the decomposition: D M⁻¹ D = V S Vᵀ, S descending, and the model (Φ V, S) has the posterior's covariance
    assert np.all(np.diff(lf["S"]) <= 0)
    basis = model.basis @ lf["V"]
    assert np.abs((basis * lf["S"]) @ basis.T - post).max() <= 1e-10 * max(1.0, np.abs(post).max())
    a, b = np.arange(model.n_points), np.arange(model.n_points)[::-1]
    assert np.allclose(LF.covariance_blocks(Q, lf["Minv"], a, b), LF.model_blocks(basis, lf["S"], a, b), rtol=0, atol=1e-10)
    assert np.allclose(LF.point_variances(Q, lf["Minv"]), np.trace(LF.covariance_blocks(Q, lf["Minv"], a, a), axis1=1, axis2=2), rtol=0, atol=1e-10)


def test_long_form_with_full_covariances_reduces_to_the_isotropic_one(pkg):
    model = _small_model(pkg, seed=6)
    ids = np.array([1, 4, 9])
    y = model.ref_points[ids] + 0.5
    iso = LF.long_form(model, ids, y, sigma2=0.3)
    full = LF.long_form(model, ids, y, covariances=np.broadcast_to(0.3 * np.eye(3), (3, 3, 3)))
    for k in ("M", "alpha", "S", "mean"):
        assert np.allclose(iso[k], full[k], rtol=0, atol=1e-12)
