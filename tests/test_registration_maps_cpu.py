"""CPU: the per-vertex registration maps and their chain summaries (icp_registration_maps_many, icp_distance_summaries_many) — the
binding, the Python-side argument checks with stand-in contexts, and the native calls' refusals without a context."""
import ctypes
import re
import os
import types

import numpy as np
import pytest

from conftest import ROOT

MAPS = ("m2t_point", "m2t_triangle", "m2t_distance", "m2t_on_boundary", "t2m_point", "t2m_triangle", "t2m_distance")
SUMMARIES = ("m2t_mean", "m2t_max", "t2m_mean", "t2m_max")


def test_symbols_and_signatures(pkg):
    nat = pkg._native
    lib = nat.lib()
    pp = ctypes.POINTER
    assert hasattr(lib, "icp_registration_maps_many") and hasattr(lib, "icp_distance_summaries_many")
    res, args = nat.SIGNATURES["icp_registration_maps_many"]
    assert res is ctypes.c_int and len(args) == 11
    assert args[0] is ctypes.c_int32 and args[1] is pp(ctypes.c_void_p) and args[2] is pp(nat.c_double_p)
    assert [args[k] for k in (3, 5, 7, 9)] == [pp(nat.c_double_p)] * 4
    assert args[4] is pp(nat.c_int_p) and args[8] is pp(nat.c_int_p) and args[6] is pp(nat.c_ubyte_p) and args[10] is nat.c_int_p
    res, args = nat.SIGNATURES["icp_distance_summaries_many"]
    assert res is ctypes.c_int and len(args) == 9
    assert args[1] is pp(ctypes.c_void_p) and args[2] is nat.c_int_p and args[8] is nat.c_int_p
    assert [args[k] for k in range(3, 8)] == [pp(nat.c_double_p)] * 5
    # the header declares as many parameters
    text = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    for name, n in (("icp_registration_maps_many", 11), ("icp_distance_summaries_many", 9)):
        m = re.search(r"ICP_API\s+int\s+" + name + r"\s*\(([^;]*)\);", text)
        assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == n
    for f in (pkg.registration_maps, pkg.distance_summaries, pkg.IcpContext.distanceMap, pkg.loggers.distance_summaries_from_logs):
        assert callable(f)


def _fake_ctx(rank):
    return types.SimpleNamespace(rank=rank, h=None)


def test_registration_maps_validates_in_python(pkg):
    r = 5
    ctx = _fake_ctx(r)
    th = np.zeros((3, 10 + r))
    with pytest.raises(ValueError):  # wrong width
        pkg.registration_maps(ctx, np.zeros((3, 9 + r)))
    with pytest.raises(ValueError):  # one context per item, or one for all
        pkg.registration_maps([ctx, ctx], th)
    with pytest.raises(ValueError):  # no items
        pkg.registration_maps(ctx, np.zeros((0, 10 + r)))
    with pytest.raises(ValueError):  # contexts of another rank
        pkg.registration_maps([ctx, ctx, _fake_ctx(r + 1)], th)
    bad = th.copy()
    bad[1, 12] = np.nan
    with pytest.raises(ValueError):
        pkg.registration_maps(ctx, bad)
    with pytest.raises(ValueError, match="unknown output"):
        pkg.registration_maps(ctx, th, want=("m2t_distance", "m2t_normal"))
    with pytest.raises(ValueError, match="at least one output"):
        pkg.registration_maps(ctx, th, want=())
    with pytest.raises(ValueError):
        pkg.registration_maps(ctx, np.zeros((2, 3, 10 + r)))


def test_distance_summaries_validates_in_python(pkg):
    r = 5
    ctx = _fake_ctx(r)
    sets = [np.zeros((4, 10 + r)), np.zeros((1, 10 + r))]
    with pytest.raises(ValueError):  # wrong width
        pkg.distance_summaries(ctx, [np.zeros((4, 9 + r))])
    with pytest.raises(ValueError):  # one context per set, or one for all
        pkg.distance_summaries([ctx], sets)
    with pytest.raises(ValueError):  # no sets
        pkg.distance_summaries(ctx, [])
    with pytest.raises(ValueError):  # contexts of another rank
        pkg.distance_summaries([ctx, _fake_ctx(r + 1)], sets)
    with pytest.raises(ValueError, match="at least one sample"):
        pkg.distance_summaries(ctx, [sets[0], np.zeros((0, 10 + r))])
    bad = sets[0].copy()
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        pkg.distance_summaries(ctx, [sets[1], bad])
    with pytest.raises(ValueError, match="unknown output"):
        pkg.distance_summaries(ctx, sets, want=("m2t_median",))
    with pytest.raises(ValueError, match="at least one output"):
        pkg.distance_summaries(ctx, sets, want=())
    with pytest.raises(ValueError):  # a flat state is not a set
        pkg.distance_summaries(ctx, [np.zeros(10 + r)])


def test_without_a_context_the_native_calls_refuse(pkg):
    """null contexts / thetas / status, bad counts and no output at all: ICP_ERR_INVALID_ARG, nothing written, no crash"""
    nat, lib = pkg._native, pkg._native.lib()
    dp, ip, up = nat.c_double_p, nat.c_int_p, nat.c_ubyte_p
    th = np.zeros(16)
    rows = np.full(12, 7.0)
    tri = np.full(4, 7, dtype=np.int32)
    flg = np.full(4, 7, dtype=np.uint8)
    status = np.full(2, 99, dtype=np.int32)
    c_ctx = (ctypes.c_void_p * 2)(None, None)
    c_th = (dp * 2)(th.ctypes.data_as(dp), th.ctypes.data_as(dp))
    o_d = (dp * 2)(rows.ctypes.data_as(dp), rows.ctypes.data_as(dp))
    o_i = (ip * 2)(tri.ctypes.data_as(ip), tri.ctypes.data_as(ip))
    o_u = (up * 2)(flg.ctypes.data_as(up), flg.ctypes.data_as(up))
    s = status.ctypes.data_as(ip)
    outs = (o_d, o_i, o_d, o_u, o_d, o_i, o_d)
    f = lib.icp_registration_maps_many
    assert f(2, c_ctx, c_th, *outs, s) == -1          # null contexts
    assert f(2, None, c_th, *outs, s) == -1
    assert f(2, c_ctx, None, *outs, s) == -1
    assert f(2, c_ctx, c_th, *outs, None) == -1
    assert f(0, c_ctx, c_th, *outs, s) == -1
    assert f(70000, c_ctx, c_th, *outs, s) == -1
    assert f(2, c_ctx, c_th, None, None, None, None, None, None, None, s) == -1   # every output NULL
    assert b"output" in lib.icp_last_error()
    ns = np.array([1, 1], dtype=np.int32)
    n = ns.ctypes.data_as(ip)
    g = lib.icp_distance_summaries_many
    assert g(2, c_ctx, n, c_th, o_d, o_d, o_d, o_d, s) == -1   # null contexts
    assert g(2, None, n, c_th, o_d, o_d, o_d, o_d, s) == -1
    assert g(2, c_ctx, None, c_th, o_d, o_d, o_d, o_d, s) == -1
    assert g(2, c_ctx, n, None, o_d, o_d, o_d, o_d, s) == -1
    assert g(2, c_ctx, n, c_th, o_d, o_d, o_d, o_d, None) == -1
    assert g(0, c_ctx, n, c_th, o_d, o_d, o_d, o_d, s) == -1
    assert g(70000, c_ctx, n, c_th, o_d, o_d, o_d, o_d, s) == -1
    assert g(2, c_ctx, n, c_th, None, None, None, None, s) == -1
    assert np.all(rows == 7.0) and np.all(tri == 7) and np.all(flg == 7) and np.all(status == 99)
