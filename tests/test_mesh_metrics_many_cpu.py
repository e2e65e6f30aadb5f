"""CPU: the batched registration metrics (icp_mesh_metrics_many) — its binding, the Python-side argument checks, Dice's sample
generator restated in Python, and the experiment summary logger (JSONExperimentLogger)."""
import ctypes
import datetime
import json
import types

import numpy as np
import pytest

M64 = (1 << 64) - 1


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rng_uniform(seed, step, lane):
    """orc_rng_uniform (oracle/icp_oracle.c): splitmix64 over (seed, step, lane) -> (0, 1)"""
    h = _splitmix(_splitmix(_splitmix(seed) ^ ((step * 0xD1342543DE82EF95) & M64)) ^ ((lane * 0x2545F4914F6CDD1D) & M64))
    return ((h >> 11) + 0.5) / 9007199254740992.0


def dice_samples(lo, hi, n, seed):
    """Dice's sample points in the box [lo, hi]: p_k = lo_k + u(s, k) * (hi_k - lo_k), each operation rounded (numpy float64)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    u = np.array([[rng_uniform(seed, s, k) for k in range(3)] for s in range(n)])
    return lo + u * (hi - lo)


def test_symbol_and_signature(pkg):
    nat = pkg._native
    assert hasattr(nat.lib(), "icp_mesh_metrics_many")
    res, args = nat.SIGNATURES["icp_mesh_metrics_many"]
    assert res is ctypes.c_int and len(args) == 7
    assert args[1] is ctypes.POINTER(ctypes.c_void_p) and args[2] is ctypes.POINTER(nat.c_double_p)
    assert args[4] is ctypes.c_uint64 and args[6] is nat.c_int_p
    assert pkg.registration_metrics is not None and pkg.dice_coefficient is not None


def _fake_ctx(rank):
    return types.SimpleNamespace(rank=rank, h=None)


def test_registration_metrics_validates_in_python(pkg):
    r = 5
    ctx = _fake_ctx(r)
    th = np.zeros((3, 10 + r))
    with pytest.raises(ValueError):  # wrong width
        pkg.registration_metrics(ctx, np.zeros((3, 9 + r)))
    with pytest.raises(ValueError):  # one context per item, or one for all
        pkg.registration_metrics([ctx, ctx], th)
    with pytest.raises(ValueError):  # no items
        pkg.registration_metrics(ctx, np.zeros((0, 10 + r)))
    with pytest.raises(ValueError):  # contexts of another rank
        pkg.registration_metrics([ctx, ctx, _fake_ctx(r + 1)], th)
    bad = th.copy()
    bad[1, 12] = np.nan
    with pytest.raises(ValueError):
        pkg.registration_metrics(ctx, bad)
    for n in (-1, (1 << 24) + 1):
        with pytest.raises(ValueError):
            pkg.registration_metrics(ctx, th, dice_samples=n)
    with pytest.raises(ValueError):
        pkg.registration_metrics(ctx, th, seed=-1)


def test_without_a_context_the_native_call_refuses(pkg):
    """null contexts / thetas / out and bad sizes: ICP_ERR_INVALID_ARG, nothing written, no crash"""
    nat, lib = pkg._native, pkg._native.lib()
    out = np.full(18, 7.0)
    status = np.full(2, 99, dtype=np.int32)
    th = np.zeros(16)
    c_ctx = (ctypes.c_void_p * 2)(None, None)
    c_th = (nat.c_double_p * 2)(th.ctypes.data_as(nat.c_double_p), th.ctypes.data_as(nat.c_double_p))
    o, s = out.ctypes.data_as(nat.c_double_p), status.ctypes.data_as(nat.c_int_p)
    assert lib.icp_mesh_metrics_many(2, c_ctx, c_th, 100, 1024, o, s) == -1
    assert lib.icp_mesh_metrics_many(0, c_ctx, c_th, 100, 1024, o, s) == -1
    assert lib.icp_mesh_metrics_many(2, None, c_th, 100, 1024, o, s) == -1
    assert lib.icp_mesh_metrics_many(2, c_ctx, None, 100, 1024, o, s) == -1
    assert lib.icp_mesh_metrics_many(2, c_ctx, c_th, 100, 1024, None, s) == -1
    assert lib.icp_mesh_metrics_many(2, c_ctx, c_th, 100, 1024, o, None) == -1
    assert lib.icp_mesh_metrics_many(70000, c_ctx, c_th, 100, 1024, o, s) == -1
    assert np.all(out == 7.0) and np.all(status == 99)


def test_sample_generator_restated(oracle):
    """the Python restatement of the counter-based generator equals the oracle's orc_rng_uniform bit for bit"""
    lib = oracle.lib()
    for seed in (1024, 0, 7, M64):
        for s in (0, 1, 17, 9999, 123456, (1 << 24) - 1):
            for k in range(3):
                assert lib.orc_rng_uniform(seed, s, k) == rng_uniform(seed, s, k)
    p = dice_samples([-1.0, 2.0, 10.0], [3.0, 2.5, 40.0], 2000, 1024)
    assert p.shape == (2000, 3)
    assert np.all(p >= [-1.0, 2.0, 10.0]) and np.all(p <= [3.0, 2.5, 40.0])
    assert abs(p[:, 2].mean() - 25.0) < 1.0


REFERENCE_FIELDS = ["index", "modelPath", "targetPath", "samplingEuclideanLoggerPath", "samplingHausdorffLoggerPath", "coeffInit",
                    "coeffSamplingEuclidean", "coeffSamplingHausdorff", "coeffIcp", "samplingEuclidean", "samplingHausdorff", "icp",
                    "numOfEvaluationPoints", "numOfSamplePoints", "normalNoise", "datetime", "comment"]


def test_json_experiment_logger_round_trip(pkg, tmp_path):
    lg = pkg.loggers.JSONExperimentLogger(tmp_path / "experiments.json", model_path="femur.h5")
    m = {"avg": 0.5, "hausdorff": 2.25, "dice": 0.9}
    before = datetime.datetime.now().replace(microsecond=0)
    for i in range(3):
        lg.append(i, targetPath=f"t{i}.stl", samplingEuclideanLoggerPath="e.json", samplingHausdorffLoggerPath="h.json",
                  coeffInit=np.arange(4.0) * i, coeffSamplingEuclidean=np.ones(4), coeffSamplingHausdorff=np.zeros(4),
                  coeffIcp=[0.25] * 4, samplingEuclidean=m, samplingHausdorff={k: v + i for k, v in m.items()}, icp=m,
                  numOfEvaluationPoints=100, numOfSamplePoints=200, normalNoise=1.0, comment="c")
    lg.write_log()
    loaded = lg.load_log()
    assert loaded == lg.experiments and len(loaded) == 3
    with open(tmp_path / "experiments.json") as f:
        raw = json.load(f)
    for rec in raw:
        assert list(rec.keys()) == REFERENCE_FIELDS
        for key in ("samplingEuclidean", "samplingHausdorff", "icp"):
            assert sorted(rec[key]) == ["avg", "dice", "hausdorff"]
        stamp = datetime.datetime.strptime(rec["datetime"], "%Y-%m-%d %H:%M:%S")
        assert before <= stamp <= datetime.datetime.now()
    assert raw[2]["modelPath"] == "femur.h5" and raw[2]["coeffInit"] == [0.0, 2.0, 4.0, 6.0]
    assert raw[1]["samplingHausdorff"]["hausdorff"] == 3.25 and raw[0]["index"] == 0
    with pytest.raises(IOError):
        pkg.loggers.JSONExperimentLogger(tmp_path / "missing" / "experiments.json")
