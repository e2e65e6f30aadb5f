"""GPU: the twin pass of the lone-chain step (icp_chain_step_prelaunch2) — the chain's next two proposals, both from the state it is
at, go through one set of five launches as two lanes; a rejected first proposal finds the second step's results waiting.

Whatever the twin pass does, the chain must be the chain of one step at a time, bit for bit: the records of the default run are compared
with those of ICP_NO_TWIN=1, of a run without speculative decompositions and of a run whose first pre-launched front is starved
of the word it waits for (the context then falls back to unpipelined steps).  A second rank takes the plain (streamed) first launch,
a mixture with many random-walk leaves puts given coefficients into both lanes, and a directly driven context checks that a dropped
second lane is ordered before whatever replaces it."""
import json
import os
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
rank = {rank!r}
if rank:
    model = pkg.data.StatisticalMeshModel(model.ref_points.copy(), model.cells.copy(), model.mean_def.copy(),
                                          np.array(model.basis[:, :rank], order="C"), model.variance[:rank].copy())
setup = pkg.femur_icp_proposal_registration(model, target, fused=2)
w_rw = {w_rw!r}
if w_rw is not None:
    setup.w_icp, setup.w_rw = 1.0 - w_rw, w_rw
ctx = pkg.IcpContext(model, target, device=0)
chain = pkg.SamplingRegistration(ctx, setup, pkg.initial_parameters(model), 1024)
np.save({out!r}, chain.run({steps!r}))
json.dump(dict(runtime=pkg._native.runtime_stats(), twin=ctx.twin_stats(), paths=ctx.step_paths()), open({stats!r}, "w"))
chain.close(); ctx.close()
"""

_SWITCHES = ("ICP_NO_TWIN", "ICP_NO_SPECULATION", "ICP_SPECULATION", "ICP_NO_PIPELINE", "ICP_TEST_STARVE_PIPELINE", "ICP_LIBRARY_PATH")


def _run_chain(tmp, tag, env, steps, rank=None, w_rw=None):
    out, stats = str(tmp / (tag + ".npy")), str(tmp / (tag + ".json"))
    base = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    if any(k.startswith("ICP_TEST_") for k in env):  # (the starvation hooks exist in the test-hooks build only)
        hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
        assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
        env = {**env, "ICP_LIBRARY_PATH": hooks}
    script = _CHAIN_SCRIPT.format(root=ROOT, out=out, stats=stats, steps=steps, rank=rank, w_rw=w_rw)
    subprocess.run([sys.executable, "-c", script], check=True, env={**base, **env}, timeout=120)
    rec, st = np.load(out), json.load(open(stats))
    print(tag, "accepted", int(rec[:, 1].sum()), st)
    return rec, st


@pytest.fixture(scope="module")
def femur50_twin_chains(tmp_path_factory):
    """The bundled femur-50 model and its own 1,622-vertex target, 400 steps of the lone-chain step, a child process per variant
    -> {tag: (records, stats)}."""
    tmp = tmp_path_factory.mktemp("twin_step")
    variants = (("twin", {}), ("one-lane", {"ICP_NO_TWIN": "1"}), ("twin-no-speculation", {"ICP_NO_SPECULATION": "1"}),
                ("twin-starved", {"ICP_TEST_STARVE_PIPELINE": "1"}))
    return {tag: _run_chain(tmp, tag, env, 400) for tag, env in variants}


def test_twin_chain_is_the_one_lane_chain(femur50_twin_chains):
    """Records of all variants equal bit for bit; more than 50 of the 400 steps accepted; no device-side wait timed out and no
    speculative decomposition gave up, except in the starved run, which falls back to unpipelined steps at least once."""
    ref = femur50_twin_chains["one-lane"][0]
    assert ref.shape[0] == 400 and ref[:, 1].sum() > 50
    for tag, (rec, st) in femur50_twin_chains.items():
        differing = np.nonzero(np.abs(rec - ref).max(axis=1))[0]
        print(tag, "records differing:", len(differing), "first:", differing[:1])
        assert np.array_equal(rec, ref), tag + ": the chain differs from the one-lane chain"
        if tag == "twin-starved":
            assert st["runtime"]["pipeline_fallbacks"] >= 1, st
        else:
            assert st["runtime"]["wait_timeouts"] == 0 and st["runtime"]["speculation_giveups"] == 0, (tag, st)
        assert st["paths"]["merged"] >= 400 and st["paths"]["per_stage"] == 0 and st["paths"]["wide"] == 0, (tag, st)


def test_twin_passes_are_issued_used_and_dropped(femur50_twin_chains):
    """The default run issues twin passes, uses second-lane results (at most one per rejected step) and drops some (accepted first
    lanes); ICP_NO_TWIN=1 issues none."""
    rec, st = femur50_twin_chains["twin"]
    tw = st["twin"]
    rejected = int((rec[:, 1] == 0).sum())
    assert tw["passes"] > 0 and tw["lane1_used"] > 0 and tw["lane1_dropped"] > 0, tw
    assert tw["lane1_used"] <= rejected, (tw, rejected)
    assert tw["lane1_used"] + tw["lane1_dropped"] <= tw["passes"], tw
    off = femur50_twin_chains["one-lane"][1]["twin"]
    assert off == {"passes": 0, "lane1_used": 0, "lane1_dropped": 0}, off


def test_twin_rank20_takes_the_plain_first_launch(tmp_path):
    """Rank 20 (the first 20 components of the same model), 100 steps: below rank 32 the first launch has the plain (streamed)
    body in both lanes.  Same chain with and without the twin pass."""
    a, sa = _run_chain(tmp_path, "twin", {}, 100, rank=20)
    b, sb = _run_chain(tmp_path, "one-lane", {"ICP_NO_TWIN": "1"}, 100, rank=20)
    assert np.array_equal(a, b)
    assert sa["twin"]["passes"] > 0 and sa["twin"]["lane1_used"] > 0 and sb["twin"]["passes"] == 0
    assert sa["runtime"]["wait_timeouts"] == 0 and sa["runtime"]["speculation_giveups"] == 0, sa


def test_twin_random_walk_leaves_in_both_lanes(tmp_path):
    """The mixture's random-walk weight raised to 0.5: half of the steps are given coefficients (generator < 0), so such leaves
    land in either lane and in both.  Same chain with and without the twin pass."""
    a, sa = _run_chain(tmp_path, "twin", {}, 200, w_rw=0.5)
    b, sb = _run_chain(tmp_path, "one-lane", {"ICP_NO_TWIN": "1"}, 200, w_rw=0.5)
    assert (a[:, 2] == 2).sum() > 50  # (leaf 2: the shape random walk)
    assert np.array_equal(a, b)
    assert sa["twin"]["passes"] > 0 and sa["twin"]["lane1_used"] > 0, sa
    assert sa["runtime"]["wait_timeouts"] == 0 and sa["runtime"]["speculation_giveups"] == 0, sa


def _chain_objects(pkg, ctx, r, tp):
    props = [pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, 2 * r, pkg.TargetSampling, True, decimatedTargetPoints=tp),
             pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, 2 * r, pkg.ModelSampling, True, decimatedTargetPoints=tp)]
    ev = pkg.IndependentPointDistanceEvaluator(ctx, 0.0, 2.0, pkg.ModelToTargetEvaluation, 4 * r, decimatedTargetPoints=tp)
    return ev, props


def _drive(pkg, model, target, twin):
    """Nine rounds from a moving state: a step that is "rejected" (its posteriors put the state on record), then steps A and B of
    the next two proposals.  Even rounds: A is rejected and B asked for (the second lane's results are used; every third round B is
    a random-walk proposal); odd rounds: A is accepted and a random walk from the NEW state follows (the second lane is dropped and
    the replacement must be ordered behind it).  twin: A and B are launched ahead as one twin pass.  -> every step's values."""
    r = model.rank
    rng = np.random.default_rng(29)
    tp = pkg.data.decimated_point_subset(target, 2 * r)
    ctx = pkg.IcpContext(model, target, device=0)
    ev, props = _chain_objects(pkg, ctx, r, tp)
    cur = pkg.initial_parameters(model)
    cur[10:] = 0.2 * rng.normal(size=r)
    values = []

    def step(gen, key):
        got = pkg.chain_step(ev, props, cur, gen, z=key) if gen >= 0 else pkg.chain_step(ev, props, cur, -1, theta_prop=key)
        values.append([np.array(v, dtype=np.float64).ravel() for v in got[:4]])
        return got

    for it in range(9):
        step(it % 2, rng.normal(size=r))
        ga, za = (it + 1) % 2, rng.normal(size=r)
        gb, kb = it % 2, rng.normal(size=r)
        if it % 3 == 2:
            gb, kb = -1, cur.copy()
            kb[10:] += 0.05 * rng.normal(size=r)
        rw = rng.normal(size=r)
        if twin:
            assert pkg.chain_step_prelaunch2(ev, props, cur, ga, za, gb, kb) == 2
        a = step(ga, za)
        if it % 2 == 0:
            b = step(gb, kb)
            cur = np.array(b[0], dtype=np.float64).copy()
        else:
            cur = np.array(a[0], dtype=np.float64).copy()
            nxt = cur.copy()
            nxt[10:] += 0.05 * rw
            step(-1, nxt)
            pm = props[1].icpPosterior(nxt, with_aux=False)
            values.append([pm.corr_id.astype(np.float64).ravel(), pm.corr_point.ravel()])
    stats = ctx.twin_stats()
    ev.close(); [p.close() for p in props]
    ctx.close()
    return values, stats


_DRIVE_SCRIPT = r"""
import pickle, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as graft
import test_gpu_twin_step as t
pkg = graft.load_package()
model, target = pkg.data.load_femur_model_and_target(50)
pickle.dump([t._drive(pkg, model, target, twin) for twin in (False, True)], open({out!r}, "wb"))
"""


def test_dropped_second_lane_is_ordered_before_its_replacement(tmp_path):
    """After an accepted first lane the second lane is dropped while its part of the finish launch may still run, and the step
    that replaces it is given slots and scratch the dropped launches wrote: its values — and those of every step served from a second
    lane — must equal those of a context stepped through the same calls without anything launched ahead.  (A child process: steps
    are launched ahead only while the process has ONE live context.)"""
    import pickle
    out = str(tmp_path / "drive.pkl")
    base = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    subprocess.run([sys.executable, "-c", _DRIVE_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)], check=True, env=base,
                   timeout=120)
    (want, s0), (got, s1) = pickle.load(open(out, "rb"))
    assert s0 == {"passes": 0, "lane1_used": 0, "lane1_dropped": 0}, s0
    assert s1 == {"passes": 9, "lane1_used": 5, "lane1_dropped": 4}, s1
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g, w):
            assert np.array_equal(a, b), "call %d differs" % k
