"""GPU: hand-over from the on-device loop to the host-stepped chain on the same proposals (ranks <= 64).

The loop carries the proposals' count of decompositions through its chain and raises the completion words of the memo entries it
decomposes to the places it takes — one per accepted step.  The host's completion-word numbers (icp_eigen_count.hpp) must stay above
those words: a speculative decomposition given a number below the stale word of a recycled entry would look complete to the next
step's first launch at once (it waits for word - number >= 0), which would then draw from a basis still being written.

A context takes a few host steps (its numbers are small), then a loop with many acceptances, then host steps that are all accepted —
each draws from the basis started ahead for the state before, in entries the loop has put off record.  Their values are compared
with those of a fresh context stepped through the same calls from the loop's final state."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOOP_STEPS, HOST_STEPS = 300, 12


def _objects(pkg, model, target):
    r = model.rank
    tp = pkg.data.decimated_point_subset(target, 2 * r)
    ctx = pkg.IcpContext(model, target, device=0)
    props = [pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, 2 * r, pkg.TargetSampling, True, decimatedTargetPoints=tp),
             pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, 2 * r, pkg.ModelSampling, True, decimatedTargetPoints=tp)]
    ev = pkg.IndependentPointDistanceEvaluator(ctx, 0.0, 2.0, pkg.ModelToTargetEvaluation, 4 * r, decimatedTargetPoints=tp)
    return ctx, props, ev


def _accepted_host_steps(pkg, ev, props, cur, n, seed):
    """n ICP steps, every proposal accepted: step k+1 draws from the basis started ahead in step k.  -> every step's values"""
    rng = np.random.default_rng(seed)
    cur, values = cur.copy(), []
    for k in range(n):
        got = pkg.chain_step(ev, props, cur, k % 2, z=rng.normal(size=len(cur) - 10))
        values.append([np.array(v, dtype=np.float64).ravel() for v in got[:4]])
        cur = np.array(got[0], dtype=np.float64).copy()
    return values


def test_host_steps_behind_a_device_loop_with_many_acceptances(pkg):
    """Values of the host steps behind the loop equal those of a fresh context to rounding: rtol 1e-9, atol 1e-10 — the two contexts'
    warm-started decompositions start from other bases and agree to ~1e-11 each, over 12 steps of step length 0.1 on coefficients
    of order 1 (the tolerances the loop's own comparisons between two decomposition histories use); a basis read while it is being
    written misses them by orders of magnitude.  No wait timed out, no decomposition gave up, nothing was repeated."""
    nat = pkg._native
    model, target = pkg.data.load_femur_model_and_target(50)
    r = model.rank
    before = nat.runtime_stats()
    ctx, props, ev = _objects(pkg, model, target)
    start = pkg.initial_parameters(model)
    start[10:] = 0.2 * np.random.default_rng(5).normal(size=r)
    _accepted_host_steps(pkg, ev, props, start, 2, seed=1)  # (the host's own count stays small)
    theta = start.copy()
    logp = np.array([pkg.ModelPriorEvaluator(r).logValue(theta) + ev.logValue(theta)])
    mix = nat.MhMixture(C.sizeof(nat.MhMixture), (C.c_double * 2)(0.5, 0.5), 0.9, 0.1, 0.1, 0.0, (C.c_double * 3)(0.01, 0.01, 0.01),
                        (C.c_double * 3)(0.1, 0.1, 0.1))
    acc = (C.c_int64 * 1)()
    rc = nat.lib().icp_chains_run_on_device(1, (C.c_void_p * 1)(ev.h), 2, (C.c_void_p * 2)(*[p.h for p in props]), C.byref(mix),
                                            (C.c_uint64 * 1)(911), (C.c_int64 * 1)(0), (nat.c_double_p * 1)(theta.ctypes.data_as(nat.c_double_p)),
                                            logp.ctypes.data_as(nat.c_double_p), LOOP_STEPS, None, acc)
    assert rc == 0
    print("loop: accepted", acc[0], "of", LOOP_STEPS, ctx.step_paths())
    assert ctx.step_paths()["device_loop"] == LOOP_STEPS
    assert acc[0] >= 40, "the loop must raise the words well above the host's numbers"
    got = _accepted_host_steps(pkg, ev, props, theta, HOST_STEPS, seed=2)
    ev.close(); [p.close() for p in props]
    ctx.close()

    ctx, props, ev = _objects(pkg, model, target)
    want = _accepted_host_steps(pkg, ev, props, theta, HOST_STEPS, seed=2)
    ev.close(); [p.close() for p in props]
    ctx.close()
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g, w):
            assert np.all(np.isfinite(a)), "step %d is not finite" % k
            assert np.allclose(a, b, rtol=1e-9, atol=1e-10), "step %d differs by %g" % (k, np.abs(a - b).max())
    after = nat.runtime_stats()
    for key in ("wait_timeouts", "speculation_giveups", "step_redos"):
        assert after[key] == before[key], (key, before, after)
