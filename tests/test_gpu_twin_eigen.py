"""GPU: the speculative decompositions of BOTH lanes of a twin pass go out in one launch when the pass is finished (ranks <= 64,
icp_ctx_twin_eigen_stats) — lane 1's a finish launch and a host turn-around earlier than at its own call.

Whenever lane 1's decomposition is launched, the chain must stay the chain of one step at a time, bit for bit: a used lane 1 takes
the place behind lane 0's in the proposal's cycle of 128 decompositions (every 128th starts cold), a dropped one gives it back.  The
records of the default run are compared with those of ICP_TWIN_LATE_EIGEN=1 (lane 1's decomposition at its own call), ICP_NO_TWIN=1
and ICP_NO_SPECULATION=1; two further ranks compare early with late; a directly driven context walks through "lane 0 rejected,
lane 1 accepted" and "lane 0 accepted" rounds across cold starts, against the same calls with nothing launched ahead."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_CHAIN_SCRIPT = r"""
import json, sys, numpy as np
sys.path.insert(0, {root!r})
import __graft_entry__ as graft
pkg = graft.load_package()
model, target = pkg.data.load_femur_model_and_target(50)
rank, source = {rank!r}, {source!r}
if source != 50:
    model = pkg.data.load_femur_model(source)
if rank:
    model = pkg.data.StatisticalMeshModel(model.ref_points.copy(), model.cells.copy(), model.mean_def.copy(),
                                          np.array(model.basis[:, :rank], order="C"), model.variance[:rank].copy())
setup = pkg.femur_icp_proposal_registration(model, target, fused=2)
ctx = pkg.IcpContext(model, target, device=0)
chain = pkg.SamplingRegistration(ctx, setup, pkg.initial_parameters(model), 1024)
np.save({out!r}, chain.run({steps!r}))
json.dump(dict(runtime=pkg._native.runtime_stats(), twin=ctx.twin_stats(), eigen=ctx.twin_eigen_stats()), open({stats!r}, "w"))
chain.close(); ctx.close()
"""

_SWITCHES = ("ICP_NO_TWIN", "ICP_TWIN_LATE_EIGEN", "ICP_NO_SPECULATION", "ICP_SPECULATION", "ICP_NO_PIPELINE", "ICP_LIBRARY_PATH")
_ZERO = {"started_early": 0, "kept": 0, "cancelled_by_lane0": 0, "started_cold": 0}


def _run_chain(tmp, tag, env, steps, rank=None, source=50):
    out, stats = str(tmp / (tag + ".npy")), str(tmp / (tag + ".json"))
    base = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    script = _CHAIN_SCRIPT.format(root=ROOT, out=out, stats=stats, steps=steps, rank=rank, source=source)
    subprocess.run([sys.executable, "-c", script], check=True, env={**base, **env}, timeout=120)
    rec, st = np.load(out), json.load(open(stats))
    print(tag, "accepted", int(rec[:, 1].sum()), st)
    return rec, st


def test_early_second_lane_chain_is_the_late_chain(tmp_path):
    """400 steps at the model's own rank: default, late, one lane, no speculation — records equal bit for bit, no wait timed out, no
    decomposition gave up.  The default run starts lane-1 decompositions early, keeps some (lane 1 accepted) and cancels some
    (lane 0 accepted); the late run starts none early.  (400 steps hold three cold starts per proposal.)"""
    steps = 400
    runs = {tag: _run_chain(tmp_path, tag, env, steps) for tag, env in (("early", {}), ("late", {"ICP_TWIN_LATE_EIGEN": "1"}),
                                                                         ("one-lane", {"ICP_NO_TWIN": "1"}),
                                                                         ("no-speculation", {"ICP_NO_SPECULATION": "1"}))}
    ref = runs["late"][0]
    assert ref.shape[0] == steps
    for tag, (rec, st) in runs.items():
        differing = np.nonzero(np.abs(rec - ref).max(axis=1))[0]
        print(tag, "records differing:", len(differing), "first:", differing[:1])
        assert np.array_equal(rec, ref), tag + ": the chain differs from the late chain"
        assert st["runtime"]["wait_timeouts"] == 0 and st["runtime"]["speculation_giveups"] == 0, (tag, st)
    eg = runs["early"][1]["eigen"]
    assert eg["started_early"] > 0 and eg["kept"] > 0 and eg["cancelled_by_lane0"] > 0, eg
    assert eg["kept"] + eg["cancelled_by_lane0"] <= eg["started_early"] <= runs["early"][1]["twin"]["passes"], runs["early"][1]
    assert runs["late"][1]["eigen"] == _ZERO, runs["late"][1]
    assert runs["late"][1]["twin"]["lane1_used"] > 0, runs["late"][1]


@pytest.mark.parametrize("rank,source", [(20, 50), (64, 100)])
def test_early_second_lane_at_other_ranks(tmp_path, rank, source):
    """Rank 20 (the model's first 20 components) and rank 64 (the first 64 of the 100-component model: the largest rank of the
    four-problem launch), 200 steps: early against late."""
    a, sa = _run_chain(tmp_path, "early", {}, 200, rank=rank, source=source)
    b, sb = _run_chain(tmp_path, "late", {"ICP_TWIN_LATE_EIGEN": "1"}, 200, rank=rank, source=source)
    assert a.shape[0] == 200 and np.array_equal(a, b)
    assert sa["eigen"]["started_early"] > 0 and sb["eigen"] == _ZERO, (sa, sb)
    for st in (sa, sb):
        assert st["runtime"]["wait_timeouts"] == 0 and st["runtime"]["speculation_giveups"] == 0, st


_ROUNDS = 141  # (a multiple of three: two "lane 1 accepted" rounds, then one "lane 0 accepted")


def _lead_for_cold_lane1(rounds):
    """Leading single steps after which some round's lane 1 takes the first place of a cycle of 128 — the cold one.  The count per
    proposal: one place for the starting state's ordinary decomposition, then one per call (every call of _drive starts the
    decomposition of its proposed state ahead: the acceptance estimate stays above 0.1; a cancelled lane 1 gives its place back, so
    the places are those of one call at a time).  -> (lead, rounds whose lane 1 starts cold)"""
    for lead in range(8):
        place, cold = 1 + lead, []
        for it in range(rounds):
            calls = ("A", "C") if it % 3 == 2 else ("A", "B", "C")
            for c in calls:
                if c == "B" and place % 128 == 127:
                    cold.append(it)
                place += 1
        if cold:
            return lead, cold
    raise AssertionError("no lead puts a cold start on a lane 1")


def _drive(pkg, model, target, twin):
    """`lead` single steps, then rounds from a moving state.  Two rounds out of three: A is rejected, B accepted, and an ICP proposal
    from B's state follows (it draws from the basis started with lane 0's); every third round: A is accepted and an ICP proposal
    from A's state follows (lane 1's decomposition is cancelled, its place returned).  twin: A and B are launched ahead as one twin
    pass.  -> every step's values, the counters."""
    r = model.rank
    rng = np.random.default_rng(31)
    tp = pkg.data.decimated_point_subset(target, 2 * r)
    ctx = pkg.IcpContext(model, target, device=0)
    props = [pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, 2 * r, pkg.TargetSampling, True, decimatedTargetPoints=tp),
             pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, 2 * r, pkg.ModelSampling, True, decimatedTargetPoints=tp)]
    ev = pkg.IndependentPointDistanceEvaluator(ctx, 0.0, 2.0, pkg.ModelToTargetEvaluation, 4 * r, decimatedTargetPoints=tp)
    cur = pkg.initial_parameters(model)
    cur[10:] = 0.2 * rng.normal(size=r)
    values = []

    def step(gen, z):
        got = pkg.chain_step(ev, props, cur, gen, z=z)
        values.append([np.array(v, dtype=np.float64).ravel() for v in got[:4]])
        return got

    lead, _ = _lead_for_cold_lane1(_ROUNDS)
    for k in range(lead):
        step(k % 2, rng.normal(size=r))
    for it in range(_ROUNDS):
        ga, za = it % 2, rng.normal(size=r)
        gb, zb = (it + 1) % 2, rng.normal(size=r)
        gc, zc = (it // 2) % 2, rng.normal(size=r)
        if twin:
            assert pkg.chain_step_prelaunch2(ev, props, cur, ga, za, gb, zb) == 2, it
        a = step(ga, za)
        if it % 3 != 2:
            b = step(gb, zb)
            cur = np.array(b[0], dtype=np.float64).copy()
        else:
            cur = np.array(a[0], dtype=np.float64).copy()
        step(gc, zc)
    stats = dict(twin=ctx.twin_stats(), eigen=ctx.twin_eigen_stats(), runtime=pkg._native.runtime_stats())
    ev.close(); [p.close() for p in props]
    ctx.close()
    return values, stats


_DRIVE_SCRIPT = r"""
import pickle, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as graft
import test_gpu_twin_eigen as t
pkg = graft.load_package()
model, target = pkg.data.load_femur_model_and_target(50)
pickle.dump([t._drive(pkg, model, target, twin) for twin in (False, True)], open({out!r}, "wb"))
"""


def test_driven_rounds_across_cold_starts(tmp_path):
    """141 rounds of a directly driven context (a child process: steps are launched ahead only while the process has ONE live
    context): every value of every call equals that of the same calls with nothing launched ahead.  Every pass starts lane 1's
    decomposition early; 94 are kept, 47 cancelled by an accepted lane 0; at least one lane 1 starts cold."""
    out = str(tmp_path / "drive.pkl")
    base = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    subprocess.run([sys.executable, "-c", _DRIVE_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)], check=True, env=base,
                   timeout=120)
    (want, s0), (got, s1) = pickle.load(open(out, "rb"))
    print(s0, s1, _lead_for_cold_lane1(_ROUNDS))
    assert s0["twin"]["passes"] == 0 and s0["eigen"] == _ZERO, s0
    assert s1["twin"] == {"passes": _ROUNDS, "lane1_used": 2 * _ROUNDS // 3, "lane1_dropped": _ROUNDS // 3}, s1
    eg = s1["eigen"]
    assert eg["started_early"] == _ROUNDS and eg["kept"] == 2 * _ROUNDS // 3 and eg["cancelled_by_lane0"] == _ROUNDS // 3, s1
    assert eg["started_cold"] >= 1, s1
    for st in (s0, s1):
        assert st["runtime"]["wait_timeouts"] == 0 and st["runtime"]["speculation_giveups"] == 0, st
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g, w):
            assert np.array_equal(a, b), "call %d differs" % k
