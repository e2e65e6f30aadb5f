"""CPU: the batched deterministic ICP entry point (icp_fit_deterministic_many) — its binding, the ModelAndTargetSampling schedule
draw and the argument checks that run before any device is touched."""
import ctypes
import types

import numpy as np
import pytest


def test_symbol_and_signature(pkg):
    nat = pkg._native
    lib = nat.lib()
    assert hasattr(lib, "icp_fit_deterministic_many")
    res, args = nat.SIGNATURES["icp_fit_deterministic_many"]
    assert res is ctypes.c_int and len(args) == 10
    assert args[1] is ctypes.POINTER(ctypes.c_void_p) and args[4] is nat.c_ubyte_p and args[9] is nat.c_int_p


def test_direction_schedule_is_seeded_binary():
    from conftest import load_package
    pkg = load_package()
    a = pkg.direction_schedule(5, 303, seed=7)
    b = pkg.direction_schedule(5, 303, seed=7)
    c = pkg.direction_schedule(5, 303, seed=8)
    assert a.shape == (5, 303) and a.dtype == np.uint8
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert set(np.unique(a)) == {0, 1}
    assert abs(a.mean() - 0.5) < 0.05  # scala.util.Random.nextBoolean: each direction with probability 1/2
    with pytest.raises(ValueError):
        pkg.direction_schedule(2, 3, seed=None)


def _fake_ctx(rank):
    return types.SimpleNamespace(rank=rank, h=None)


def test_icp_fits_validates_in_python(pkg):
    r = 6
    ctx = _fake_ctx(r)
    th = np.zeros((3, 10 + r))
    ids = np.arange(4, dtype=np.int32)
    with pytest.raises(ValueError):  # wrong width
        pkg.icp_fits(ctx, np.zeros((3, 9 + r)), 1, modelPointIds=ids)
    with pytest.raises(ValueError):  # one context per fit, or one for all
        pkg.icp_fits([ctx, ctx], th, 1, modelPointIds=ids)
    with pytest.raises(ValueError):  # ModelAndTargetSampling without a schedule needs a seed
        pkg.icp_fits(ctx, th, 1, projectionDirection=pkg.ModelAndTargetSampling, modelPointIds=ids)
    with pytest.raises(ValueError):  # schedule of the wrong shape: [n_fits, len(seq) * (numIterations + 1)]
        pkg.icp_fits(ctx, th, 1, (1.0, 0.1), directions=np.zeros((3, 3), dtype=np.uint8), modelPointIds=ids)
    with pytest.raises(ValueError):  # one target sample list, or one per fit
        pkg.icp_fits(ctx, th, 1, projectionDirection=pkg.TargetSampling, targetPointSamples=[np.zeros((2, 3))] * 2)
    with pytest.raises(ValueError):
        pkg.icp_fits(ctx, th, 1, projectionDirection="Sideways", modelPointIds=ids)


def test_without_a_context_the_native_call_refuses(pkg):
    """null contexts (there is no device here to make one): ICP_ERR_INVALID_ARG, nothing written, no crash"""
    nat, lib = pkg._native, pkg._native.lib()
    sig = np.array([1.0])
    status = np.full(2, 99, dtype=np.int32)
    assert lib.icp_fit_deterministic_many(2, None, None, None, None, 0, 1, sig.ctypes.data_as(nat.c_double_p), None,
                                          status.ctypes.data_as(nat.c_int_p)) == -1
    assert b"null argument" in lib.icp_last_error()
    assert np.all(status == 99)
    assert lib.icp_fit_deterministic_many(0, None, None, None, None, 0, 1, None, None, None) == -1
    r = 4
    th = np.zeros((2, 10 + r))
    with pytest.raises(nat.IcpNativeError) as e:
        pkg.icp_fits(_fake_ctx(r), th, 2, (1.0,), projectionDirection=pkg.ModelAndTargetSampling, modelPointIds=np.arange(3),
                     targetPointSamples=np.zeros((3, 3)), seed=3)
    assert e.value.status == -1


def test_fitting_keeps_model_and_target_sampling(pkg):
    """IcpBasedSurfaceFitting no longer treats ModelAndTargetSampling as ModelSampling (it takes the batched entry with a schedule)"""
    fit = pkg.IcpBasedSurfaceFitting(_fake_ctx(4), projectionDirection=pkg.ModelAndTargetSampling, modelPointIds=np.arange(3))
    assert fit.mixed and fit.seed == 1024
    assert not pkg.IcpBasedSurfaceFitting(_fake_ctx(4), projectionDirection=pkg.TargetSampling).mixed
