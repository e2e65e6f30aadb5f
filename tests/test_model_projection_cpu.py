"""CPU: the batched model projection (icp_model_instances_many, icp_model_coefficients_many) — the bindings, the Python-side argument
checks with the native library stubbed out, and loggers.experiment_coefficients building one batched call."""
import ctypes
import types

import numpy as np
import pytest


def test_symbols_and_signatures(pkg):
    nat = pkg._native
    L = nat.lib()
    assert hasattr(L, "icp_model_instances_many") and hasattr(L, "icp_model_coefficients_many")
    pp = ctypes.POINTER(nat.c_double_p)
    res, args = nat.SIGNATURES["icp_model_instances_many"]
    assert res is ctypes.c_int and len(args) == 4
    assert args[0] is ctypes.c_int32 and args[1] is ctypes.POINTER(ctypes.c_void_p) and args[2] is pp and args[3] is pp
    res, args = nat.SIGNATURES["icp_model_coefficients_many"]
    assert res is ctypes.c_int and len(args) == 8
    assert args[0] is ctypes.c_int32 and args[1] is ctypes.POINTER(ctypes.c_void_p)
    assert args[2] is pp and args[3] is pp and args[4] is pp and args[6] is pp
    assert args[5] is nat.c_double_p and args[7] is nat.c_int_p
    for name in ("transformed_meshes", "model_coefficients"):
        assert callable(getattr(pkg, name))
    assert callable(pkg.IcpContext.coefficients) and callable(pkg.IcpContext.project)
    assert callable(pkg.loggers.experiment_coefficients)


def test_without_a_context_the_native_calls_refuse(pkg):
    """null contexts and bad sizes: ICP_ERR_INVALID_ARG, nothing written, no crash"""
    nat, L = pkg._native, pkg._native.lib()
    th = np.zeros(16)
    out = np.full(6, 7.0)
    coeffs = np.full(12, 7.0)
    status = np.full(2, 99, dtype=np.int32)
    dp = nat.c_double_p
    c_ctx = (ctypes.c_void_p * 2)(None, None)
    c_th = (dp * 2)(th.ctypes.data_as(dp), th.ctypes.data_as(dp))
    c_out = (dp * 2)(out.ctypes.data_as(dp), out.ctypes.data_as(dp))
    assert L.icp_model_instances_many(2, c_ctx, c_th, c_out) == -1
    assert L.icp_model_instances_many(0, c_ctx, c_th, c_out) == -1
    assert L.icp_model_instances_many(65536, c_ctx, c_th, c_out) == -1
    assert L.icp_model_instances_many(2, None, None, None) == -1
    o, s = coeffs.ctypes.data_as(dp), status.ctypes.data_as(nat.c_int_p)
    assert L.icp_model_coefficients_many(2, c_ctx, None, c_th, None, o, None, s) == -1
    assert L.icp_model_coefficients_many(0, c_ctx, None, c_th, None, o, None, s) == -1
    assert L.icp_model_coefficients_many(2, None, None, None, None, None, None, None) == -1
    assert np.all(out == 7.0) and np.all(coeffs == 7.0) and np.all(status == 99)


def _fake_ctx(rank, n=7):
    return types.SimpleNamespace(rank=rank, N=n, h=None)


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def test_transformed_meshes_validate_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    r = 5
    ctx = _fake_ctx(r)
    ok = np.zeros((3, 10 + r))
    with pytest.raises(ValueError):  # no items
        pkg.transformed_meshes(ctx, [])
    with pytest.raises(ValueError):  # wrong width
        pkg.transformed_meshes(ctx, np.zeros((3, 9 + r)))
    with pytest.raises(ValueError):  # one context per item, or one for all
        pkg.transformed_meshes([ctx, ctx], ok)
    with pytest.raises(ValueError):  # a context of another rank against these widths
        pkg.transformed_meshes([ctx, ctx, _fake_ctx(r + 1)], ok)
    with pytest.raises(ValueError):  # models of different vertex counts cannot share one array
        pkg.transformed_meshes([ctx, ctx, _fake_ctx(r, 8)], ok)
    bad = ok.copy()
    bad[2, 4] = np.inf
    with pytest.raises(ValueError):
        pkg.transformed_meshes(ctx, bad)


def test_model_coefficients_validate_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    r, N = 5, 7
    ctx = _fake_ctx(r, N)
    mesh = np.zeros((N, 3))
    th = np.zeros(10 + r)
    th[0] = 1.0
    pose = th[:10].copy()
    with pytest.raises(ValueError):  # neither meshes nor thetas
        pkg.model_coefficients(ctx)
    with pytest.raises(ValueError):  # no items
        pkg.model_coefficients(ctx, meshes=[])
    with pytest.raises(ValueError):  # both for an item
        pkg.model_coefficients(ctx, meshes=[mesh], thetas=[th])
    with pytest.raises(ValueError):  # neither for an item
        pkg.model_coefficients(ctx, meshes=[mesh, None], thetas=[None, None])
    with pytest.raises(ValueError):  # lists of different lengths
        pkg.model_coefficients(ctx, meshes=[mesh, mesh], thetas=[None])
    with pytest.raises(ValueError):  # one context per item, or one for all
        pkg.model_coefficients([ctx, ctx], meshes=[mesh])
    with pytest.raises(ValueError):  # mixed models: another rank, another vertex count
        pkg.model_coefficients([ctx, _fake_ctx(r + 1, N)], meshes=[mesh, mesh])
    with pytest.raises(ValueError):
        pkg.model_coefficients([ctx, _fake_ctx(r, N + 1)], meshes=[mesh, mesh])
    with pytest.raises(ValueError):  # a mesh of another size
        pkg.model_coefficients(ctx, meshes=[np.zeros((N + 1, 3))])
    with pytest.raises(ValueError):  # theta of the wrong width, non-finite theta
        pkg.model_coefficients(ctx, thetas=[np.zeros(9 + r)])
    bad = th.copy()
    bad[11] = np.nan
    with pytest.raises(ValueError):
        pkg.model_coefficients(ctx, thetas=[th, bad])
    with pytest.raises(ValueError):  # one pose per item
        pkg.model_coefficients(ctx, meshes=[mesh, mesh], poses=[pose])
    with pytest.raises(ValueError):  # a pose of the wrong length
        pkg.model_coefficients(ctx, meshes=[mesh], poses=[np.zeros(9)])
    nf = pose.copy()
    nf[2] = np.inf
    with pytest.raises(ValueError):  # a non-finite pose
        pkg.model_coefficients(ctx, meshes=[mesh], poses=[nf])
    sc = pose.copy()
    sc[0] = 1.0 + 2.0 ** -52
    with pytest.raises(ValueError):  # s != 1
        pkg.model_coefficients(ctx, meshes=[mesh], poses=[sc])
    with pytest.raises(ValueError):  # the one-item forms go the same way
        pkg.IcpContext.coefficients(ctx, mesh, pose=sc)
    with pytest.raises(ValueError):
        pkg.IcpContext.project(ctx, np.zeros((N + 2, 3)))


def test_one_item_forms_go_through_the_batched_entry(pkg, monkeypatch):
    calls = []

    def stub(contexts, meshes=None, thetas=None, poses=None, want_project=False):
        calls.append((contexts, meshes, thetas, poses, want_project))
        c = np.arange(5.0)[None, :]
        return (c, np.ones((1, 7, 3))) if want_project else c

    monkeypatch.setattr(pkg.api, "model_coefficients", stub)
    ctx = _fake_ctx(5)
    mesh, pose = np.zeros((7, 3)), np.zeros(10)
    assert np.array_equal(pkg.IcpContext.coefficients(ctx, mesh, pose), np.arange(5.0))
    assert pkg.IcpContext.project(ctx, mesh).shape == (7, 3)
    assert calls[0][0] is ctx and calls[0][1][0] is mesh and calls[0][3][0] is pose and calls[0][4] is False
    assert calls[1][3] == [None] and calls[1][4] is True


def test_experiment_coefficients_builds_one_batched_call(pkg, monkeypatch):
    r = 4
    ctxs = [_fake_ctx(r), _fake_ctx(r), _fake_ctx(r)]
    rng = np.random.default_rng(0)
    th = rng.normal(size=(3, 10 + r))
    th[:, 0] = 1.0
    calls = []

    def stub(contexts, meshes=None, thetas=None, poses=None, want_project=False):
        calls.append((contexts, meshes, thetas, poses, want_project))
        return np.stack([t[10:] * 2.0 for t in thetas])

    monkeypatch.setattr(pkg.api, "model_coefficients", stub)
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    got = pkg.loggers.experiment_coefficients(ctxs, th)
    assert len(calls) == 1, "one batched call for every state"
    c_ctx, c_mesh, c_th, c_pose, c_proj = calls[0]
    assert c_ctx is ctxs and c_mesh is None and c_proj is False
    assert len(c_th) == 3 and all(np.array_equal(a, b) for a, b in zip(c_th, th))
    assert all(np.array_equal(p, t[:10]) for p, t in zip(c_pose, th))  # every state's own pose is taken off its mesh
    assert np.array_equal(got, 2.0 * th[:, 10:])
    # one context for all
    calls.clear()
    pkg.loggers.experiment_coefficients(ctxs[0], list(th))
    assert calls[0][0] is ctxs[0] and len(calls[0][2]) == 3
