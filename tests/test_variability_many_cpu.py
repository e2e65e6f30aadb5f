"""CPU: the batched posterior variability maps (icp_posterior_variability_many) — its binding, the Python-side argument checks, and
variability_from_logs' choice of states, with the native call stubbed."""
import ctypes
import types

import numpy as np
import pytest


def test_symbol_and_signature(pkg):
    nat = pkg._native
    assert hasattr(nat.lib(), "icp_posterior_variability_many")
    res, args = nat.SIGNATURES["icp_posterior_variability_many"]
    assert res is ctypes.c_int and len(args) == 8
    assert args[0] is ctypes.c_int32 and args[1] is ctypes.POINTER(ctypes.c_void_p)
    assert args[2] is nat.c_int_p and args[4] is nat.c_int_p
    for k in (3, 5, 6, 7):
        assert args[k] is ctypes.POINTER(nat.c_double_p)
    assert pkg.posterior_variability_maps is not None and pkg.loggers.variability_from_logs is not None


def _fake_ctx(rank, n=7):
    return types.SimpleNamespace(rank=rank, N=n, h=None)


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def test_maps_validate_in_python(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    r = 5
    ctx = _fake_ctx(r)
    ok = np.zeros((3, 10 + r))
    with pytest.raises(ValueError):  # fewer than two samples
        pkg.posterior_variability_maps(ctx, [ok, ok[:1]])
    with pytest.raises(ValueError):  # wrong width
        pkg.posterior_variability_maps(ctx, [np.zeros((3, 9 + r))])
    with pytest.raises(ValueError):  # a context of another rank
        pkg.posterior_variability_maps([ctx, _fake_ctx(r + 1)], [ok, ok])
    with pytest.raises(ValueError):  # mode 1 without a reference
        pkg.posterior_variability_maps(ctx, [ok, ok], mode=[0, 1])
    with pytest.raises(ValueError):  # mode 1, a reference for the other map only
        pkg.posterior_variability_maps(ctx, [ok, ok], mode=[0, 1], theta_refs=[ok[0], None])
    with pytest.raises(ValueError):  # unknown mode
        pkg.posterior_variability_maps(ctx, [ok], mode=3)
    with pytest.raises(ValueError):  # mismatched lengths: contexts, modes, references
        pkg.posterior_variability_maps([ctx], [ok, ok])
    with pytest.raises(ValueError):
        pkg.posterior_variability_maps(ctx, [ok, ok], mode=[0])
    with pytest.raises(ValueError):
        pkg.posterior_variability_maps(ctx, [ok, ok], mode=1, theta_refs=[ok[0]])
    with pytest.raises(ValueError):  # a reference of the wrong width
        pkg.posterior_variability_maps(ctx, [ok], mode=1, theta_refs=[np.zeros(9 + r)])
    bad = ok.copy()
    bad[1, 3] = np.nan
    with pytest.raises(ValueError):  # a non-finite sample
        pkg.posterior_variability_maps(ctx, [ok, bad])
    # no maps: nothing to do, and nothing native
    assert pkg.posterior_variability_maps(ctx, []) == []
    assert pkg.posterior_variability_maps(ctx, [], want_mean=True) == ([], [])


def _synthetic_log(n, r, seed, p_accept=0.4):
    """a jsonLogFormat list as JSONAcceptRejectLogger.add_records writes it; entry 0 is accepted"""
    rng = np.random.default_rng(seed)
    log = []
    for i in range(n):
        acc = i == 0 or bool(rng.random() < p_accept)
        log.append({"index": i, "name": "p", "logvalue": {"product": float(-i)}, "status": acc,
                    "rigid": [float(v) for v in rng.normal(size=9)] if acc else [],
                    "coeff": [float(v) for v in rng.normal(size=r)] if acc else [], "datetime": ""})
    return log


def test_variability_from_logs_picks_samples_from_log(pkg, monkeypatch):
    r, N = 4, 6
    ctxs = [_fake_ctx(r, N), _fake_ctx(r, N), _fake_ctx(r, N)]
    logs = [_synthetic_log(400, r, 1), _synthetic_log(333, r, 2), _synthetic_log(120, r, 3)]
    calls = []

    def stub(contexts, sample_sets, mode=0, theta_refs=None, want_mean=False):
        calls.append((list(contexts), [np.array(a) for a in sample_sets], list(mode), list(theta_refs), want_mean))
        outs = [np.full(c.N, float(k)) for k, c in enumerate(contexts)]
        return (outs, [np.zeros((c.N, 3)) for c in contexts]) if want_mean else outs

    monkeypatch.setattr(pkg.api, "posterior_variability_maps", stub)
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    kw = dict(take_every_n=7, total=350, burn_in=20)
    res = pkg.loggers.variability_from_logs(ctxs, logs, mode=(2, 0), **kw)
    assert len(calls) == 1, "one batched call for every log and mode"
    c_ctx, c_sets, c_mode, c_refs, c_mean = calls[0]
    assert c_ctx == ctxs + ctxs and c_mode == [2, 2, 2, 0, 0, 0] and c_refs == [None] * 6 and c_mean is False
    to_theta = pkg.loggers.JSONAcceptRejectLogger.sample_to_model_parameters
    for k, lg in enumerate(logs):
        want = pkg.loggers.samples_from_log(lg, **kw)
        assert len(want) >= 2
        assert res["indices"][k] == [i for _, i in want]
        assert all(lg[i]["status"] for i in res["indices"][k])
        th = np.stack([to_theta(s) for s, _ in want])
        assert np.array_equal(c_sets[k], th) and np.array_equal(c_sets[3 + k], th)
    assert set(res["maps"]) == {2, 0}
    assert [float(m[0]) for m in res["maps"][2]] == [0.0, 1.0, 2.0] and [float(m[0]) for m in res["maps"][0]] == [3.0, 4.0, 5.0]
    # one context for all, one mode, references and the mean
    calls.clear()
    refs = [to_theta(lg[0]) for lg in logs]
    res = pkg.loggers.variability_from_logs(ctxs[0], logs, mode=1, theta_refs=refs, want_mean=True, **kw)
    assert calls[0][0] == [ctxs[0]] * 3 and calls[0][2] == [1, 1, 1] and calls[0][4] is True
    assert all(np.array_equal(a, b) for a, b in zip(calls[0][3], refs))
    assert len(res["means"]) == 3 and res["means"][0].shape == (N, 3)
    # a log with fewer than two states behind the burn-in, mismatched lengths
    with pytest.raises(ValueError):
        pkg.loggers.variability_from_logs(ctxs[0], [logs[2]], take_every_n=50, total=10000, burn_in=100)
    with pytest.raises(ValueError):
        pkg.loggers.variability_from_logs(ctxs[:2], logs, **kw)
    with pytest.raises(ValueError):
        pkg.loggers.variability_from_logs(ctxs, logs, theta_refs=refs[:1], **kw)
