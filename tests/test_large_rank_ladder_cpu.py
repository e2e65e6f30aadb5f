"""CPU: the rank ladder of tests/large_rank_ladder.py holds both sides of every edge of the restated dispatch of ranks 65..501 and a
rank in every state of the periodic decisions, its models are what they are meant to be, and the reference
tests/test_gpu_large_ranks.py compares the device with is sound at every rank of the ladder — without a GPU.

The reference, per rank and direction, in the parity configuration (σt = 10, σn = 5, step 0.1; K and the state from
large_rank_ladder.parity_state): the oracle keeps at least half of its correspondences (the face models' target is open); its S is
1/eigvalsh(D⁻¹MD⁻¹) to 1e-12; its propose and log_transition are the numpy closed forms of kernels_posterior.hip's header at the parity
tests' bars (1e-7, 1e-8; the z = 0 step 1e-6); the smallest gap of N' is at least 1e-5·μ_max — the condition of
tests/test_small_rank_ladder_cpu.py, as stated there.  The oracle's calls of one rank run side by side on host threads (ctypes releases
the GIL; the oracle's caches are thread-local).  Rank 500, about 6 s a posterior: one state per direction — the random z forwards,
and the z = 0 step.  Every figure is printed per rank."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import large_rank_ladder as LR
from test_gpu_parity import rel_err


def test_ladder_holds_both_sides_of_every_edge():
    assert LR.LADDER == tuple(sorted(set(LR.LADDER))) and LR.LADDER[0] == LR.MIN_RANK and LR.LADDER[-1] == LR.MAX_RANK
    assert {65, 256, 257, 500} <= set(LR.LADDER)
    for name, (fn, where) in LR.DISPATCH.items():
        es = LR.edges(fn)
        print(f"{name} ({where}): changes behind rank {es}")
        assert es and where, name  # (a decision without an edge in 65..500 does not belong in DISPATCH)
        for r in es:
            assert r in LR.LADDER and (r + 1 in LR.LADDER or r + 1 == LR.REFUSED_RANK), (name, r)
    # ... and nothing is in it without a reason
    assert LR.LADDER == LR.derived_ladder()
    assert all(LR.stands_for(r) or r == LR.MIN_RANK for r in LR.LADDER)
    assert len(LR.LADDER) <= 40
    assert set(LR.CHAIN_RANKS) <= set(LR.LADDER) and set(LR.CHAIN_STEPS) == set(LR.CHAIN_RANKS)


def test_ladder_holds_every_state_of_the_periodic_decisions():
    for name, (fn, states) in LR.PERIODIC.items():
        seen = {s: [r for r in LR.LADDER if fn(r) == s] for s in states}
        print(name, seen)
        assert {fn(r) for r in range(LR.MIN_RANK, LR.MAX_RANK + 1)} == set(states), name   # the states listed are the states there are
        assert all(seen[s] for s in states), (name, seen)


def test_restated_dispatch_gives_the_values_the_code_documents():
    """figures the native sources state themselves (the table in launch_posterior_factor, the comments of kernels_step.hip,
    kernels_eigen.hip and abi_step.inl) and the edges the issue of this module lists"""
    edge = lambda name: LR.edges(LR.DISPATCH[name][0])
    assert edge("finish_plan") == [67, 82, 116] and edge("step path, closed target") == [116, 256] and edge("step path, open target") == [256]
    assert [LR.finish_plan(r) for r in (65, 68, 83, 116, 117)] == [(2, 512, 2, True), (2, 512, 2, False), (2, 512, 1, False), (2, 512, 1, False), None]
    assert edge("root sampler") == [125, 127, 217, 253, 256] and LR.root_sampler(257) == "refused"
    assert [LR.factor_launch(r) for r in (125, 126, 128, 218, 254, 257)] == [
        ("k_posterior_factor_reg<1, 1024>", False, False), ("k_posterior_factor_reg<2, 1024>", False, False),
        ("k_posterior_factor_tiles<3>", True, False), ("k_posterior_factor_tiles<4>", True, False),
        ("k_posterior_factor_generic", True, False), ("k_posterior_factor_generic", False, False)]
    assert LR.factor_tile_count(253) == 4096 and LR.factor_tile_count(217) == 3025 and LR.factor_tile_count(218) == 3080
    assert [LR.propose_launch(r) for r in (65, 128, 129, 134, 135, 500)] == [(256, 1), (256, 1), (256, 0), (256, 0), (1024, 4), (1024, 4)]
    assert [LR.propose_launch(r, True) for r in (65, 128, 129, 256, 257)] == [(1024, 3), (1024, 3), (1024, 2), (1024, 2), None]
    assert [LR.matvec_tpr_log2(r, 512) for r in (65, 116, 128, 129, 256, 257)] == [2, 2, 2, 1, 1, 0]
    assert [LR.tails_launch(r) for r in (89, 90, 125, 126)] == [(256, 2, 1), (256, 1, 1), (256, 1, 1), (1024, 0, 4)]
    assert edge("tridiagonal shapes") == [128, 192, 200, 208, 256] and edge("eigen fall-back") == [140, 200, 256]
    assert LR.eigen_route(256) == "tridiagonal" and LR.eigen_route(257) == ("k_posterior_eigen", False, False) == LR.eigen_route(500)
    assert LR.generic_eigen_lds(128) == (True, False) and LR.generic_eigen_lds(129) == (False, False)
    assert edge("k_mhw_decide") == [128, 256] and edge("context") == [500] and LR.context(501) == "refused"
    assert LR.batched_limits(256) == (True, True, True) and LR.batched_limits(257) == (False, False, True) == LR.batched_limits(500)


@pytest.mark.parametrize("r", [65, 101, 117, 201, 209])
def test_models_of_the_ladder(pkg, r):
    model, target = LR.ladder_model(pkg, r)
    assert model.rank == r and model.basis.flags.c_contiguous and model.basis.flags.owndata
    if LR.closed_target(r):
        full, full_target = pkg.data.load_femur_model_and_target(100 if r <= 101 else 200)
        assert np.array_equal(model.basis, full.basis[:, :r]) and np.array_equal(model.variance, full.variance[:r])
        assert np.array_equal(target.points, full_target.points)
    else:
        assert model.n_points == LR.FACE_GRID ** 2 and target.n_points < model.n_points and model.n_points >= 2 * LR.MAX_RANK
        again = pkg.data.synthetic_face_model(grid=LR.FACE_GRID, rank=r)
        assert np.array_equal(again.basis, model.basis) and np.all(np.diff(model.variance) <= 0) and model.variance[-1] > 0
    assert [LR.source(q) for q in (65, 101, 102, 201, 202, 500)] == ["femur-100", "femur-100", "femur-200", "femur-200", "face", "face"]
    assert LR.parity_K(r) <= model.n_points and LR.parity_K(LR.MAX_RANK) <= LR.FACE_GRID ** 2


@pytest.fixture(scope="module")
def figures():
    """rank -> the worst figures, for the summary line"""
    out = {}
    yield out
    if out:
        for k in ("S", "propose", "log T", "z = 0 step", "cond", "seconds a posterior"):
            r = max(out, key=lambda q: out[q][k])
            print(f"worst {k}: {out[r][k]:.2e} at rank {r}")
        r = min(out, key=lambda q: out[q]["gap"])
        print(f"smallest gap: {out[r]['gap']:.2e} at rank {r}")
        r = min(out, key=lambda q: out[q]["kept"])
        print(f"smallest kept share: {out[r]['kept']:.3f} at rank {r}")


@pytest.mark.parametrize("r", LR.LADDER)
def test_reference_is_sound(pkg, oracle, figures, r):
    model, target = LR.ladder_model(pkg, r)
    om, ot = oracle.OracleModel.from_model(model), oracle.OracleMesh(target.points, target.cells)
    theta, K = LR.parity_theta(model), LR.parity_K(r)
    G = LR.gram(model)
    one_state = r == LR.MAX_RANK
    zs = [np.zeros(r), np.random.default_rng(200 + r).normal(size=r)]
    pps = {d: LR.oracle_params(oracle, pkg, target, K, d)[0] for d in LR.DIRECTIONS}
    timed = []

    def posterior(d, th):
        t0 = time.perf_counter()
        po = oracle.icp_posterior(om, ot, pps[d], th)
        timed.append(time.perf_counter() - t0)
        return po

    with ThreadPoolExecutor(max_workers=12) as ex:
        post = {d: ex.submit(posterior, d, theta) for d in LR.DIRECTIONS}
        want = {(d, k): ex.submit(oracle.propose, om, ot, pps[d], theta, z) for d in LR.DIRECTIONS for k, z in enumerate(zs)}
        post = {d: f.result() for d, f in post.items()}
        want = {k: f.result() for k, f in want.items()}
        # transition densities both ways for both z; at rank 500 the random z forwards only
        pairs = [(d, k, back) for d in LR.DIRECTIONS for k in range(2) for back in (False, True) if not one_state or (k == 1 and not back)]
        logt = {(d, k, back): ex.submit(oracle.log_transition, om, ot, pps[d], *((want[d, k], theta) if back else (theta, want[d, k])))
                for d, k, back in pairs}
        post_at = {(d, k): ex.submit(posterior, d, want[d, k]) for d, k, back in pairs if back}
        logt = {k: f.result() for k, f in logt.items()}
        post_at = {k: f.result() for k, f in post_at.items()}
    worst = {"S": 0.0, "propose": 0.0, "log T": 0.0, "z = 0 step": 0.0, "gap": 1.0, "cond": 0.0, "kept": 1.0, "seconds a posterior": max(timed)}
    for d in LR.DIRECTIONS:
        po = post[d]
        kept = int(po.keep.sum())
        assert po.keep.shape == (K,) and 2 * kept >= K, (r, d, kept, K)
        Np = LR.n_prime(model, po.M)
        w = np.linalg.eigvalsh(Np)
        assert np.all(np.diff(po.S) <= 0) and np.all(po.S > 0)
        err_S = float((np.abs(np.sort(po.S) - np.sort(1.0 / w)) / np.sort(1.0 / w)).max())
        gap, cond = LR.smallest_relative_gap(Np), float(np.linalg.cond(po.M))
        errs_p, errs_t = [], []
        for k, z in enumerate(zs):
            wz = want[d, k]
            assert np.all(np.isfinite(wz)) and np.array_equal(wz[:10], theta[:10])
            errs_p.append(rel_err(LR.closed_form_propose(model, G, po.alpha, po.V, po.S, theta, z, 0.1)[10:], wz[10:]))
        step0 = rel_err(want[d, 0][10:], theta[10:] + 0.1 * (po.alpha - theta[10:]))
        for (dd, k, back), lo in logt.items():
            if dd != d:
                continue
            a, b, pa = (want[d, k], theta, post_at[d, k]) if back else (theta, want[d, k], po)
            lm = LR.closed_form_log_transition(model, G, pa.alpha, pa.M, a, b, 0.1)
            assert np.isfinite(lo) and np.isfinite(lm)
            errs_t.append(abs(lm - lo) / abs(lo))
        print(f"rank {r} {d}: K {K} kept {kept}/{K} cond(M) {cond:.1e} S {err_S:.1e} gap {gap:.1e} propose {max(errs_p):.1e} "
              f"log T {max(errs_t):.1e} z=0 step {step0:.1e}; longest posterior {max(timed):.2f} s")
        assert err_S <= 1e-12, (r, d, err_S)
        assert max(errs_p) < 1e-7 and max(errs_t) <= 1e-8 and step0 < 1e-6, (r, d, errs_p, errs_t, step0)
        assert gap >= 1e-5, (r, d, gap)
        for k, v in (("S", err_S), ("propose", max(errs_p)), ("log T", max(errs_t)), ("z = 0 step", step0), ("cond", cond)):
            worst[k] = max(worst[k], v)
        worst["gap"], worst["kept"] = min(worst["gap"], gap), min(worst["kept"], kept / K)
    if r < LR.MAX_RANK:   # a pose change: −∞ (one cheap call; at rank 500 the GPU test's own)
        other = want["ModelSampling", 1].copy()
        other[1] += 0.1
        assert oracle.log_transition(om, ot, pps["ModelSampling"], theta, other) == -np.inf
    figures[r] = worst


def test_oracle_chain_time_sizes_the_step_counts(pkg, oracle):
    """CHAIN_STEPS is sized so that the oracle's chains — what the GPU test's time consists of, a host thread each — stay within a few
    seconds: 0.15 s a step at rank 65, 0.6 s at 116..135, 1.1 s at 218, 1.6 s at 254 and 257 on the CPU this was written on"""
    from conftest import oracle_chains_parallel
    from test_gpu_chain import oracle_chain_config
    jobs = []
    for r in LR.CHAIN_RANKS:
        model, target = LR.ladder_model(pkg, r)
        setup, theta0, seed = LR.chain_setup(pkg, model, target)
        om, ot = oracle.OracleModel.from_model(model), oracle.OracleMesh(target.points, target.cells)
        jobs.append((om, ot, oracle_chain_config(oracle, setup), theta0, seed, LR.CHAIN_STEPS[r]))
    t0 = time.perf_counter()
    res = oracle_chains_parallel(oracle, jobs)
    print(f"the oracle's {len(jobs)} chains side by side: {time.perf_counter() - t0:.2f} s")
    for r, (acc, comp, logp, states) in zip(LR.CHAIN_RANKS, res):
        print(f"rank {r}: {LR.CHAIN_STEPS[r]} steps, accepted {int(acc.sum())}, components {comp.tolist()}")
        assert np.all(np.isfinite(logp)) and np.all(np.isfinite(states)) and acc.sum() >= 2
