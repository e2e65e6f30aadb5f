"""GPU: the log values of many states under many evaluators in one call (icp_evaluator_log_values_many; the reference's logger
scores every named evaluator on every logged sample, JSONAcceptRejectLogger.scala:84-106) against the one-item path
(icp_evaluator_log_value on a fresh evaluator) bit for bit, against the oracle, across chunkings, around a running chain, on a
chain's records and through its argument errors."""
import ctypes

import numpy as np
import pytest

from conftest import make_theta, open_patch_target

pytestmark = pytest.mark.gpu

ICP_ERR_EMPTY, ICP_ERR_BUSY = -5, -6  # include/icp_proposal.h
INDEPENDENT, HAUSDORFF, COLLECTIVE = 0, 1, 2
ORACLE_REL = {INDEPENDENT: 1e-11, HAUSDORFF: 1e-12, COLLECTIVE: 1e-11}  # what tests/test_gpu_parity.py holds the one-item path to
# (kind, mode, K_e): every kind and mode at the study's 4·rank points; one query, partial waves (63, 65) on both sides
CONFIGS = ([(INDEPENDENT, m, 204) for m in (0, 1, 2)] + [(INDEPENDENT, 2, k) for k in (1, 63, 65)] + [(HAUSDORFF, 2, 0)] +
           [(COLLECTIVE, m, 204) for m in (0, 1, 2)] + [(COLLECTIVE, 2, k) for k in (1, 63, 65)])


def make_evaluator(pkg, ctx, kind, mode, k):
    if kind == INDEPENDENT:
        return pkg.IndependentPointDistanceEvaluator(ctx, 0.0, 2.0, mode, k)
    if kind == HAUSDORFF:
        return pkg.HausdorffDistanceEvaluator(ctx, 1.0)
    return pkg.CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator(ctx, 0.1, 0.3, 1.0, mode, k)


def oracle_params(pkg, oracle, target, kind, mode, k):
    if kind == HAUSDORFF:
        return oracle.evaluator_params(oracle.EVAL_HAUSDORFF, 2, p0=1.0)
    tp = pkg.data.decimated_point_subset(target, k)
    if kind == INDEPENDENT:
        return oracle.evaluator_params(oracle.EVAL_INDEPENDENT, mode, n_model_ids=min(k, 1622), target_pts=tp, p0=0.0, p1=2.0)
    return oracle.evaluator_params(oracle.EVAL_COLLECTIVE, mode, n_model_ids=min(k, 1622), target_pts=tp, p0=0.1, p1=0.3, p2=1.0)


def one_item(pkg, ctx, kind, mode, k, theta):
    """icp_evaluator_log_value on a fresh evaluator: (value, aux[4], status) — through ctypes, so that an empty set is a status"""
    nat = pkg._native
    ev = make_evaluator(pkg, ctx, kind, mode, k)
    out, aux = ctypes.c_double(), np.zeros(4)
    th = np.ascontiguousarray(theta, dtype=np.float64)
    st = nat.lib().icp_evaluator_log_value(ev.h, th.ctypes.data_as(nat.c_double_p), ctypes.byref(out), aux.ctypes.data_as(nat.c_double_p))
    ev.close()
    return out.value, aux, st


@pytest.fixture(scope="module")
def targets(pkg, femur50):
    """closed (the bundled target), open (a hole: boundary vertices) and the 58,322-vertex synthetic target, one context each"""
    model, target = femur50
    pts, cells = open_patch_target(target)
    meshes = [target, pkg.data.TriangleMesh(pts, cells), pkg.data.synthetic_femur_target()[1]]
    ctxs = [pkg.IcpContext(model, m, device=0) for m in meshes]
    yield meshes, ctxs
    for c in ctxs:
        c.close()


@pytest.fixture(scope="module")
def states(femur50):
    return np.stack([make_theta(femur50[0], 700 + b, shape_scale=0.4) for b in range(12)])


@pytest.mark.parametrize("which", [0, 1], ids=["closed", "open"])
def test_same_bits_as_one_at_a_time(pkg, targets, states, which):
    """every kind x mode x K_e of CONFIGS on 12 states, all in ONE call: value, aux and status of every item are those of
    logValue(..., return_aux=True) on a fresh evaluator"""
    ctx = targets[1][which]
    evs = [make_evaluator(pkg, ctx, *cfg) for cfg in CONFIGS]
    B = len(states)
    got = pkg.log_values([e for e in evs for _ in range(B)], np.concatenate([states] * len(evs)), return_aux=True)
    for e in evs:
        e.close()
    assert np.all((got["status"] == 0) | (got["status"] == ICP_ERR_EMPTY))  # (one boundary-aware point may well be dropped)
    for c, cfg in enumerate(CONFIGS):
        for b in range(B):
            v, aux, st = one_item(pkg, ctx, *cfg, states[b])
            i = c * B + b
            assert st == got["status"][i], (cfg, b)
            assert np.array_equal(got["value"][i], v, equal_nan=True), (cfg, b, got["value"][i], v)
            assert np.array_equal(got["aux"][i], aux, equal_nan=True), (cfg, b, got["aux"][i], aux)


def _mixed_items(pkg, targets, model, n=40):
    _, ctxs = targets
    cfgs = [c for c in CONFIGS if c[2] in (0, 204)]  # the seven kind x mode pairs
    evs = {}
    items = []
    for b in range(n):
        t, cfg = b % 3, cfgs[b % len(cfgs)]
        if b == 5:
            t, cfg = 2, (HAUSDORFF, 2, 0)  # 58,322 target -> model distances: the reductions' block size above 4,096
        if (t, cfg) not in evs:
            evs[(t, cfg)] = make_evaluator(pkg, ctxs[t], *cfg)
        items.append((t, cfg))
    th = np.stack([make_theta(model, 900 + b, shape_scale=0.4) for b in range(n)])
    return evs, items, th


def test_mixed_call_and_chunkings(pkg, femur50, targets):
    """40 items cycling through all kinds and modes on three contexts in one call, then the same items in shuffled calls of 1 and 7"""
    model, _ = femur50
    evs, items, th = _mixed_items(pkg, targets, model)
    B = len(items)
    assert (2, (HAUSDORFF, 2, 0)) in items and len({t for t, _ in items}) == 3 and len({c for _, c in items}) == 7
    ev_of = [evs[it] for it in items]
    whole = pkg.log_values(ev_of, th, return_aux=True)
    assert np.all(whole["status"] == 0) and np.all(np.isfinite(whole["value"]))
    parts = {"value": np.zeros(B), "aux": np.zeros((B, 4)), "status": np.full(B, 99, dtype=np.int32)}
    perm = np.random.default_rng(3).permutation(B)
    i, size = 0, 1
    while i < B:
        sel = perm[i:i + size]
        m = pkg.log_values([ev_of[b] for b in sel], th[sel], return_aux=True)
        for k in parts:
            parts[k][sel] = m[k]
        i += size
        size = 8 - size  # 1, 7, 1, 7, …
    for k in parts:
        assert np.array_equal(whole[k], parts[k], equal_nan=True), k
    # the big target's Hausdorff item against the one-item path
    v, aux, st = one_item(pkg, targets[1][2], HAUSDORFF, 2, 0, th[5])
    assert st == 0 and whole["value"][5] == v and np.array_equal(whole["aux"][5], aux)
    for e in evs.values():
        e.close()


def test_against_the_oracle(pkg, oracle, femur50, targets, states):
    """a handful of items per kind against oracle.evaluator_log_value, at the tolerances tests/test_gpu_parity.py holds the one-item
    path to (1e-11 relative; 1e-12 for the Hausdorff evaluator)"""
    model, _ = femur50
    meshes, ctxs = targets
    om = oracle.OracleModel.from_model(model)
    cfgs = [c for c in CONFIGS if c[2] in (0, 204)]
    items = [(t, cfg, b) for t in (0, 1) for cfg in cfgs for b in (0, 7)]
    evs = {(t, cfg): make_evaluator(pkg, ctxs[t], *cfg) for t, cfg, _ in items}
    got = pkg.log_values([evs[(t, cfg)] for t, cfg, _ in items], states[[b for _, _, b in items]])
    for e in evs.values():
        e.close()
    ots = [oracle.OracleMesh(m.points, m.cells) for m in meshes[:2]]
    for i, (t, cfg, b) in enumerate(items):
        want, rc = oracle.evaluator_log_value(om, ots[t], oracle_params(pkg, oracle, meshes[t], *cfg), states[b])
        tol = ORACLE_REL[cfg[0]]
        assert rc == 0 and got["status"][i] == 0
        assert abs(got["value"][i] - want) <= tol * abs(want), (t, cfg, b, got["value"][i], want)


def test_empty_item_between_good_ones(pkg, femur50, targets, states):
    """the empty-set construction of tests/test_gpu_edges.py (a target of three separate triangles: every vertex a boundary vertex,
    the collective evaluator's model side keeps nothing) between good items: its status is ICP_ERR_EMPTY, the neighbours keep their
    bits, the call succeeds"""
    model, target = femur50
    rng = np.random.default_rng(3)
    tris = target.cells[rng.choice(target.cells.shape[0], 3, replace=False)]
    pts = target.points[tris.ravel()].copy()
    tgt = pkg.data.TriangleMesh(pts, np.arange(9, dtype=np.int32).reshape(3, 3))
    assert pkg.data.boundary_vertex_flags(tgt).all()
    ctx = pkg.IcpContext(model, tgt, device=0)
    r = model.rank
    empties = [pkg.CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator(ctx, 0.1, 0.3, 1.0, mode, 4 * r, decimatedTargetPoints=pts)
               for mode in (0, 1, 2)]  # (mode 1 keeps its points: App. D5 tests ids 0..8 of the model's sample)
    good = [make_evaluator(pkg, targets[1][0], INDEPENDENT, 2, 204), make_evaluator(pkg, targets[1][1], COLLECTIVE, 2, 204)]
    evs = [good[0], empties[0], good[1], empties[1], good[0], empties[2], good[1]]
    th = states[:7]
    nat = pkg._native
    values, aux, status = np.zeros(7), np.zeros((7, 4)), np.zeros(7, dtype=np.int32)
    rc = nat.lib().icp_evaluator_log_values_many(7, (ctypes.c_void_p * 7)(*[e.h for e in evs]),
                                                 (nat.c_double_p * 7)(*[t.ctypes.data_as(nat.c_double_p) for t in th]),
                                                 values.ctypes.data_as(nat.c_double_p), aux.ctypes.data_as(nat.c_double_p),
                                                 status.ctypes.data_as(nat.c_int_p))
    assert rc == 0
    assert list(status) == [0, ICP_ERR_EMPTY, 0, 0, 0, ICP_ERR_EMPTY, 0]
    alone = pkg.log_values([evs[b] for b in (0, 2, 4, 6)], th[[0, 2, 4, 6]], return_aux=True)
    assert np.array_equal(values[[0, 2, 4, 6]], alone["value"]) and np.array_equal(aux[[0, 2, 4, 6]], alone["aux"])
    for b, mode in ((1, 0), (3, 1), (5, 2)):
        out, a1 = ctypes.c_double(), np.zeros(4)
        fresh = pkg.CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator(ctx, 0.1, 0.3, 1.0, mode, 4 * r, decimatedTargetPoints=pts)
        st = nat.lib().icp_evaluator_log_value(fresh.h, th[b].ctypes.data_as(nat.c_double_p), ctypes.byref(out), a1.ctypes.data_as(nat.c_double_p))
        fresh.close()
        assert st == status[b]
        assert np.array_equal(values[b], out.value, equal_nan=True) and np.array_equal(aux[b], a1, equal_nan=True)
    for e in empties + good:
        e.close()
    ctx.close()


def _chain(pkg, model, target, other_evs, n=10, score_at=None):
    """n steps of a femur-50 chain through chain_step (every proposal taken as the next state); score_at: the step before which
    a log_values call on the chain's own evaluator and context (and other contexts) comes in"""
    r = model.rank
    ctx = pkg.IcpContext(model, target, device=0)
    tp = pkg.data.decimated_point_subset(target, 2 * r)
    props = [pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, 2 * r, pkg.TargetSampling, True, decimatedTargetPoints=tp),
             pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, 2 * r, pkg.ModelSampling, True, decimatedTargetPoints=tp)]
    ev = pkg.IndependentPointDistanceEvaluator(ctx, 0.0, 2.0, pkg.ModelToTargetEvaluation, 4 * r, decimatedTargetPoints=tp)
    rng = np.random.default_rng(21)
    theta = pkg.initial_parameters(model)
    theta[10:] = 0.3 * rng.normal(size=r)
    rec, scored = [], None
    for step in range(n):
        z = rng.normal(size=r)
        if step == score_at:
            th = np.stack([theta, make_theta(model, 77), theta])
            scored = pkg.log_values([ev, other_evs[0], other_evs[1]], th)
        prop, val, fwd, bwd = pkg.chain_step(ev, props, theta, generator=step % 2, z=z)
        rec.append(np.concatenate([prop, [val], fwd, bwd]))
        theta = prop
    stats = (ev.bindStats(), ctx.runtime_stats())
    ev.close(); [p.close() for p in props]; ctx.close()
    return np.stack(rec), stats, scored


def test_leaves_chains_alone(pkg, femur50, targets):
    model, target = femur50
    others = [make_evaluator(pkg, targets[1][1], COLLECTIVE, 2, 204), make_evaluator(pkg, targets[1][0], HAUSDORFF, 2, 0)]
    plain, stats0, _ = _chain(pkg, model, target, others)
    mixed, stats1, scored = _chain(pkg, model, target, others, score_at=5)
    for e in others:
        e.close()
    assert scored is not None and np.all(scored["status"] == 0)
    assert np.array_equal(plain, mixed)
    assert stats0 == stats1
    assert all(v == 0 for v in stats1[1].values()), stats1[1]  # no redo, no time-out, no fall-back


def test_records_of_a_host_chain(pkg, oracle):
    """60 steps of the chain tests/test_gpu_log.py logs (pose moves, the collective evaluator on a partial target): prior + distance of
    log_values_of_records equals every record's own value — which the chain's merged step computed, not this path.  That file sets
    no bound for the value itself; the suite holds a record's value to 1e-6 of the largest (tests/test_gpu_face.py), taken here.
    The prior: the closed form against the oracle's at the 1e-14 of tests/test_abi_cpu.py."""
    model = pkg.data.synthetic_face_model(grid=41, rank=40)
    target = pkg.data.synthetic_partial_target(model, n_remove=90)
    setup = pkg.bfm_fitting_partial(model, target, evaluator="collective")
    setup.pose_rot_sigma, setup.pose_trans_sigma = (0.02, 0.01, 0.004), (0.2, 0.1, 0.05)
    theta0, seed, n = pkg.initial_parameters(model), 31, 60
    ctx = pkg.IcpContext(model, target, device=0)
    chain = pkg.SamplingRegistration(ctx, setup, theta0, seed)
    rec = chain.run(n)
    e = setup.eval
    ev = pkg.api._Evaluator(ctx, e["kind"], e["mode"], e["n_model_ids"], e["target_pts"], e["gauss_mean"], e["gauss_sigma"], e["exp_rate"])
    lv = pkg.loggers.log_values_of_records(rec, ev, theta0)
    assert 0 < rec[:, 1].sum() < n  # accepted and rejected records
    assert np.array_equal(lv["product"], lv["prior"] + lv["distance"])
    assert np.abs(lv["product"] - rec[:, 3]).max() <= 1e-6 * np.abs(rec[:, 3]).max(), np.abs(lv["product"] - rec[:, 3]).max()
    current = theta0
    for k in range(n):
        current = rec[k, 4:] if rec[k, 1] != 0.0 else current
        assert np.array_equal(rec[k, 4:], current)  # (a rejected record carries the current state: host/icp_host.h)
        assert np.isclose(lv["prior"][k], oracle.prior_log_value(model.rank, current), rtol=1e-14, atol=0.0)
    # … and the log with every named evaluator
    full = pkg.loggers.JSONAcceptRejectLogger().add_records(rec, setup.leaf_names(), logvalues=lv).log_status
    assert all(sorted(s["logvalue"]) == ["distance", "prior", "product"] for s in full)
    assert full[n - 1]["logvalue"]["distance"] == lv["distance"][n - 1]
    ev.close(); chain.close(); ctx.close()


def test_argument_errors(pkg, femur50, targets, states):
    model, target = femur50
    nat, lib = pkg._native, pkg._native.lib()
    _, ctxs = targets
    m200, t200 = pkg.data.load_femur_model_and_target(200)
    c200 = pkg.IcpContext(m200, t200, device=0)
    busy_ctx = pkg.IcpContext(model, target, device=0)
    r = model.rank
    tp = pkg.data.decimated_point_subset(target, 2 * r)
    ev0, ev1 = make_evaluator(pkg, ctxs[0], INDEPENDENT, 2, 204), make_evaluator(pkg, ctxs[1], COLLECTIVE, 2, 204)
    ev200 = pkg.HausdorffDistanceEvaluator(c200, 1.0)
    busy_ev = pkg.IndependentPointDistanceEvaluator(busy_ctx, 0.0, 2.0, pkg.ModelToTargetEvaluation, 4 * r, decimatedTargetPoints=tp)
    busy_props = [pkg.NonRigidIcpProposal(busy_ctx, 0.1, 10.0, 5.0, 2 * r, pkg.ModelSampling, True, decimatedTargetPoints=tp)]
    values, aux = np.full(2, 7.0), np.full(8, 7.0)
    status = np.full(2, 99, dtype=np.int32)
    v, a, s = values.ctypes.data_as(nat.c_double_p), aux.ctypes.data_as(nat.c_double_p), status.ctypes.data_as(nat.c_int_p)

    def call(evs, thetas):
        c_ev = (ctypes.c_void_p * 2)(*[e.h if e is not None else None for e in evs])
        c_th = (nat.c_double_p * 2)(*[t.ctypes.data_as(nat.c_double_p) if t is not None else None for t in thetas])
        return lib.icp_evaluator_log_values_many(2, c_ev, c_th, v, a, s)
    th = [states[0].copy(), states[1].copy()]
    assert call([ev0, None], th) == -1
    assert call([ev0, ev1], [th[0], None]) == -1
    bad = th[1].copy()
    bad[3] = np.inf
    assert call([ev0, ev1], [th[0], bad]) < 0
    assert call([ev0, ev200], [th[0], np.zeros(10 + m200.rank)]) == -1  # mixed models
    tk = pkg.BatchedStepTicket([busy_ev], [busy_props], [th[0]], [0], z=[np.random.default_rng(2).normal(size=r)])
    assert call([ev0, busy_ev], th) == ICP_ERR_BUSY
    tk.abandon()
    assert np.all(values == 7.0) and np.all(aux == 7.0) and np.all(status == 99)
    assert call([ev0, busy_ev], th) == 0 and np.all(status == 0) and np.all(np.isfinite(values)) and np.all(np.isfinite(aux))
    for o in (ev0, ev1, ev200, busy_ev, busy_props[0]):
        o.close()
    c200.close(); busy_ctx.close()
