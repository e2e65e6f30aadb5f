"""CPU: the batched evaluator call (icp_evaluator_log_values_many) — its binding and argument checks without a device — and the
host side of re-scoring a chain's records: which state a record is scored at (log_values_of_records, a stub in place of the
device call) and the JSON log with every named evaluator (JSONAcceptRejectLogger.add_records(logvalues=...))."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT


def test_symbol_and_signature(pkg):
    nat = pkg._native
    assert hasattr(nat.lib(), "icp_evaluator_log_values_many")
    res, args = nat.SIGNATURES["icp_evaluator_log_values_many"]
    assert res is ctypes.c_int and len(args) == 6
    assert args[0] is ctypes.c_int32 and args[1] is ctypes.POINTER(ctypes.c_void_p) and args[2] is ctypes.POINTER(nat.c_double_p)
    assert args[3] is nat.c_double_p and args[4] is nat.c_double_p and args[5] is nat.c_int_p
    # the header's declaration: same name, six parameters in this order
    text = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    m = re.search(r"ICP_API\s+int\s+icp_evaluator_log_values_many\s*\(([^;]*)\);", text)
    assert m is not None
    params = [p.split() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [p[-1].lstrip("*") for p in params] == ["n_items", "evaluators", "thetas", "values", "aux", "status"]
    assert pkg.log_values is pkg.api.log_values and pkg.loggers.log_values_of_records is not None


def test_without_a_device_the_native_call_refuses(pkg):
    """null arguments and item counts of 0 and 70,000: ICP_ERR_INVALID_ARG, nothing written, no crash"""
    nat, lib = pkg._native, pkg._native.lib()
    values, aux = np.full(2, 7.0), np.full(8, 7.0)
    status = np.full(2, 99, dtype=np.int32)
    th = np.zeros(16)
    c_ev = (ctypes.c_void_p * 2)(None, None)
    c_th = (nat.c_double_p * 2)(th.ctypes.data_as(nat.c_double_p), th.ctypes.data_as(nat.c_double_p))
    v, a, s = values.ctypes.data_as(nat.c_double_p), aux.ctypes.data_as(nat.c_double_p), status.ctypes.data_as(nat.c_int_p)
    assert lib.icp_evaluator_log_values_many(2, c_ev, c_th, v, a, s) == -1  # null items
    assert b"null argument" in lib.icp_last_error()
    assert lib.icp_evaluator_log_values_many(0, c_ev, c_th, v, a, s) == -1
    assert lib.icp_evaluator_log_values_many(70000, c_ev, c_th, v, a, s) == -1
    assert lib.icp_evaluator_log_values_many(2, None, c_th, v, a, s) == -1
    assert lib.icp_evaluator_log_values_many(2, c_ev, None, v, a, s) == -1
    assert lib.icp_evaluator_log_values_many(2, c_ev, c_th, None, a, s) == -1
    assert lib.icp_evaluator_log_values_many(2, c_ev, c_th, v, a, None) == -1
    assert lib.icp_evaluator_log_values_many(2, c_ev, c_th, v, None, s) == -1  # (aux may be null; the items are not)
    assert np.all(values == 7.0) and np.all(aux == 7.0) and np.all(status == 99)


def test_log_values_validates_in_python(pkg):
    r = 5
    ev = types.SimpleNamespace(ctx=types.SimpleNamespace(rank=r), h=None)
    other = types.SimpleNamespace(ctx=types.SimpleNamespace(rank=r + 1), h=None)
    th = np.zeros((3, 10 + r))
    with pytest.raises(ValueError):  # wrong width
        pkg.log_values(ev, np.zeros((3, 9 + r)))
    with pytest.raises(ValueError):  # one evaluator per item, or one for all
        pkg.log_values([ev, ev], th)
    with pytest.raises(ValueError):  # no items
        pkg.log_values(ev, np.zeros((0, 10 + r)))
    with pytest.raises(ValueError):  # an evaluator of another rank
        pkg.log_values([ev, ev, other], th)
    bad = th.copy()
    bad[1, 12] = np.nan
    with pytest.raises(ValueError):
        pkg.log_values(ev, bad)


def _records(rank, theta_init, seed=5):
    """fabricated step records [index, accepted, leaf, value, theta]: a rejected record carries the current state, as the host
    chain writes it; the first three steps are rejections"""
    rng = np.random.default_rng(seed)
    accepted = [0, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0]
    rec = np.zeros((len(accepted), 14 + rank))
    current = theta_init.copy()
    want = []
    for k, a in enumerate(accepted):
        if a:
            current = theta_init + rng.normal(size=theta_init.shape)
        rec[k, 0], rec[k, 1], rec[k, 2], rec[k, 3] = k, a, k % 3, -1.0 - k
        rec[k, 4:] = current
        want.append(current.copy())
    return rec, np.stack(want), accepted


def test_records_are_scored_at_the_current_state(pkg, monkeypatch):
    rank = 4
    theta_init = np.arange(10.0 + rank) / 7.0
    rec, want_states, accepted = _records(rank, theta_init)
    seen = []

    def stub(evaluator, thetas, return_aux=False):
        th = np.asarray(thetas)
        seen.append(th.copy())
        assert evaluator == "the evaluator"
        return {"value": th.sum(axis=1) * 0.25, "aux": None, "status": np.zeros(len(th), dtype=np.int32)}
    monkeypatch.setattr(pkg.api, "log_values", stub)
    for blank_rejected in (False, True):
        records = rec.copy()
        if blank_rejected:  # (a log read back: a rejected entry has no state of its own)
            records[records[:, 1] == 0.0, 4:] = 0.0
        seen.clear()
        lv = pkg.loggers.log_values_of_records(records, "the evaluator", theta_init)
        assert sorted(lv) == ["distance", "prior", "product"]
        assert len(seen) == 1 and seen[0].shape == (1 + sum(accepted), 10 + rank)  # ONE call over the distinct states
        assert np.array_equal(seen[0][0], theta_init)  # before the first acceptance: the initial state
        assert np.array_equal(lv["distance"], want_states.sum(axis=1) * 0.25)
        prior = np.array([-0.5 * (s[10:] @ s[10:]) - 0.5 * rank * np.log(2 * np.pi) for s in want_states])
        assert np.allclose(lv["prior"], prior, rtol=1e-14, atol=0.0)
        assert np.array_equal(lv["product"], lv["prior"] + lv["distance"])
        assert lv["distance"][0] == lv["distance"][2] and lv["distance"][4] == lv["distance"][3]  # rejected: the state before
    with pytest.raises(ValueError):
        pkg.loggers.log_values_of_records(rec, "the evaluator", theta_init[:-1])


def test_add_records_with_and_without_logvalues(pkg):
    rank = 4
    theta_init = np.arange(10.0 + rank) / 7.0
    rec, _, accepted = _records(rank, theta_init)
    names = {0: "icp", 1: "walk", 2: "pose"}
    L = pkg.loggers.JSONAcceptRejectLogger
    plain = L().add_records(rec, names).log_status
    # today's output: the record's own value under the one name, states for accepted records only
    for k, (e, a) in enumerate(zip(plain, accepted)):
        assert list(e) == ["index", "name", "logvalue", "status", "rigid", "coeff", "datetime"]
        assert e["index"] == k and e["name"] == names[k % 3] and e["status"] == bool(a)
        assert e["logvalue"] == {"product": -1.0 - k}
        assert e["rigid"] == ([float(v) for v in rec[k, 5:14]] if a else []) and e["coeff"] == ([float(v) for v in rec[k, 14:]] if a else [])
    again = L().add_records(rec, names, logvalues=None).log_status
    assert [dict(e, datetime="") for e in again] == [dict(e, datetime="") for e in plain]
    lv = {"product": np.arange(len(rec)) * 1.5, "prior": -np.arange(len(rec)) * 0.5, "distance": np.arange(len(rec)) * 2.0}
    full = L().add_records(rec, names, logvalues=lv).log_status
    for k, (e, p) in enumerate(zip(full, plain)):
        assert e["logvalue"] == {"product": 1.5 * k, "prior": -0.5 * k, "distance": 2.0 * k}
        assert {key: v for key, v in e.items() if key not in ("logvalue", "datetime")} == \
               {key: v for key, v in p.items() if key not in ("logvalue", "datetime")}
    with pytest.raises(ValueError):
        L().add_records(rec, names, logvalues={"product": np.zeros(3)})
