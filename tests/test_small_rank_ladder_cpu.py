"""CPU: the rank ladder of tests/small_rank_ladder.py holds both sides of every edge of the restated dispatch, its models are what
they are meant to be, and the reference tests/test_gpu_small_ranks.py compares the device with is sound at every rank of the ladder —
without a GPU.

The reference, per rank and direction, in the parity configuration (K = 2r, σt = 10, σn = 5, step 0.1, make_theta(model, seed)):
the oracle keeps correspondences; its S is 1/eigvalsh(D⁻¹MD⁻¹) to 1e-12; its propose and log_transition are the numpy closed forms of
kernels_posterior.hip's header at the parity tests' bars (1e-7, 1e-8); the smallest gap of N' is at least 1e-5·μ_max, the level at
which the eigenvector bar of 1e-7 holds at rank 51 (eps·μ_max / gap).  Every figure is printed per rank."""
import numpy as np
import pytest

import small_rank_ladder as SR
from test_gpu_eigen_spectra import factor_kernel as factor_kernel_to_256
from test_gpu_parity import rel_err


def test_ladder_holds_both_sides_of_every_edge():
    assert SR.LADDER == tuple(sorted(set(SR.LADDER))) and SR.LADDER[0] == 1 and SR.LADDER[-1] == SR.MAX_RANK
    assert {1, 2, 3, SR.MAX_RANK} <= set(SR.LADDER)
    for name, fn in SR.DISPATCH.items():
        es = SR.edges(fn)
        print(f"{name}: changes behind rank {es}")
        assert es, name  # (a decision without an edge in 1..64 does not belong in DISPATCH)
        for r in es:
            assert r in SR.LADDER and r + 1 in SR.LADDER, (name, r)
    # ... and nothing is in it without a reason
    assert SR.LADDER == SR.derived_ladder()
    assert all(SR.stands_for(r) or r in (1, SR.MAX_RANK) for r in SR.LADDER)
    assert len(SR.LADDER) <= 40
    assert set(SR.CHAIN_RANKS) <= set(SR.LADDER) and set(SR.K_EDGE_RANKS) <= set(SR.LADDER)


def test_restated_dispatch_gives_the_values_the_code_documents():
    """figures the native sources state themselves (comments of kernels_factor.hip, kernels_step.hip, kernels_eigen.hip, the issue's
    table) and the restatement tests/test_gpu_eigen_spectra.py already keeps"""
    assert all(SR.factor_kernel(r) == factor_kernel_to_256(r) for r in range(1, 65))
    assert SR.factor_tile_count(61) == 256 and SR.factor_tile_count(62) == 272        # "ranks 1..61 ... one tile per thread of 256"
    assert [SR.factor_tile_count(r) for r in (1, 2, 3)] == [1, 2, 2]                   # one or two tiles in all
    assert [SR.instance_split(r) for r in (9, 10, 24, 35, 50, 51, 64)] == [(0, 0, 9), (0, 1, 0), (0, 2, 4), (1, 1, 0), (2, 0, 0), (2, 0, 1), (2, 1, 4)]
    assert [SR.regression_tiles(r) for r in (15, 16, 31, 32, 47, 48, 63, 64)] == [1, 3, 3, 6, 6, 10, 10, 15]
    assert [SR.step_begin_variant(r) for r in (31, 32, 52, 53, 64)] == ["k_step_begin", "k_step_begin_reg<52>", "k_step_begin_reg<52>",
                                                                      "k_step_begin_reg<64>", "k_step_begin_reg<64>"]
    assert SR.jacobi_shape(1) is None and SR.jacobi_shape(2) is None
    assert SR.jacobi_shape(3) == dict(n2=4, m=2, nbw=1, per=2, dummy=True)
    assert SR.jacobi_shape(20)["nbw"] == 1 and SR.jacobi_shape(21)["nbw"] == 2
    assert SR.jacobi_shape(32)["per"] == 2 and SR.jacobi_shape(33)["per"] == 3
    assert SR.jacobi_shape(64) == dict(n2=64, m=32, nbw=9, per=3, dummy=False) and SR.jacobi_shape(63)["dummy"]
    assert [SR.matvec_tpr_log2(r, 256) for r in (1, 15, 16, 31, 32, 64)] == [0, 0, 1, 1, 2, 2]
    assert SR.step_finish_plan(61)[:2] == (1, 256) and SR.step_finish_plan(62)[:2] == (2, 512)
    assert SR.projection_pad(16) == 16 and SR.projection_pad(17) == 32 and SR.posterior_model_pads(15) == (16, 16)
    assert SR.posterior_model_pads(16) == (16, 32) and SR.posterior_model_pads(64) == (64, 80)


@pytest.mark.parametrize("r", [1, 51, 52, 64])
def test_truncated_models_own_their_arrays(pkg, r):
    n_comp = SR.source_components(r)
    assert n_comp == (50 if r <= 51 else 100)
    model, target = SR.ladder_model(pkg, r)
    full, full_target = pkg.data.load_femur_model_and_target(n_comp)
    assert full.rank == n_comp + 1 and model.rank == r and model.n_points == full.n_points
    assert np.array_equal(model.basis, full.basis[:, :r]) and np.array_equal(model.variance, full.variance[:r])
    assert np.array_equal(model.ref_points, full.ref_points) and np.array_equal(model.mean_def, full.mean_def)
    assert np.array_equal(target.points, full_target.points) and np.array_equal(target.cells, full_target.cells)
    shared = SR._bundled[n_comp][0]
    arrays = lambda m: (m.basis, m.variance, m.ref_points, m.mean_def, m.cells)
    for a in arrays(model):
        assert a.flags.c_contiguous and a.flags.owndata
        assert not any(np.shares_memory(a, b) for b in arrays(shared))
    # what an IcpContext does to the arrays it is given leaves the shared model, and the next truncation, as they were
    for a in arrays(model):
        a.flags.writeable = False
    assert all(b.flags.writeable for b in arrays(shared))
    again, _ = SR.ladder_model(pkg, r)
    assert all(a.flags.writeable for a in arrays(again))


@pytest.fixture(scope="module")
def figures():
    """rank -> the worst figures, for the summary line"""
    out = {}
    yield out
    if out:
        for k in ("S", "propose", "log T"):
            r = max(out, key=lambda q: out[q][k])
            print(f"worst {k}: {out[r][k]:.2e} at rank {r}")
        r = min(out, key=lambda q: out[q]["gap"])
        print(f"smallest gap: {out[r]['gap']:.2e} at rank {r}; largest cond(M): {max(v['cond'] for v in out.values()):.2e}")


@pytest.mark.parametrize("r", SR.LADDER)
def test_reference_is_sound(pkg, oracle, figures, r):
    model, target = SR.ladder_model(pkg, r)
    om, ot = oracle.OracleModel.from_model(model), oracle.OracleMesh(target.points, target.cells)
    theta = SR.parity_theta(model)
    G = SR.gram(model)
    rng = np.random.default_rng(200 + r)
    worst = dict(S=0.0, propose=0.0, gap=1.0, cond=0.0)
    worst["log T"] = 0.0
    for direction in SR.DIRECTIONS:
        pp, _ = SR.oracle_params(oracle, pkg, target, 2 * r, direction)
        po = oracle.icp_posterior(om, ot, pp, theta)
        kept = int(po.keep.sum())
        assert po.keep.shape == (2 * r,) and kept >= 1, (r, direction)
        Np = SR.n_prime(model, po.M)
        w = np.linalg.eigvalsh(Np)
        assert np.all(np.diff(po.S) <= 0) and np.all(po.S > 0)
        err_S = float((np.abs(np.sort(po.S) - np.sort(1.0 / w)) / np.sort(1.0 / w)).max())
        gap = SR.smallest_relative_gap(Np)
        cond = float(np.linalg.cond(po.M))
        errs_p, errs_t = [], []
        for z in (np.zeros(r), rng.normal(size=r)):
            want = oracle.propose(om, ot, pp, theta, z)
            mine = SR.closed_form_propose(model, G, po.alpha, po.V, po.S, theta, z, 0.1)
            assert np.all(np.isfinite(want)) and np.array_equal(want[:10], theta[:10])
            errs_p.append(rel_err(mine[10:], want[10:]))
            if not z.any():  # z = 0 is the step towards α, up to the σ² shrinkage: the parity test's 1e-6
                step0 = rel_err(want[10:], theta[10:] + 0.1 * (po.alpha - theta[10:]))
            for a, b in ((theta, want), (want, theta)):
                lo = oracle.log_transition(om, ot, pp, a, b)
                pa = po if a is theta else oracle.icp_posterior(om, ot, pp, a)
                lm = SR.closed_form_log_transition(model, G, pa.alpha, pa.M, a, b, 0.1)
                assert np.isfinite(lo) and np.isfinite(lm)
                errs_t.append(abs(lm - lo) / abs(lo))
        other = want.copy()
        other[1] += 0.1
        assert oracle.log_transition(om, ot, pp, theta, other) == -np.inf
        print(f"rank {r} {direction}: kept {kept}/{2 * r} cond(M) {cond:.1e} S {err_S:.1e} gap {gap:.1e} "
              f"propose {max(errs_p):.1e} log T {max(errs_t):.1e} z=0 step {step0:.1e}")
        assert err_S <= 1e-12, (r, direction, err_S)
        assert max(errs_p) < 1e-7 and max(errs_t) <= 1e-8 and step0 < 1e-6, (r, direction, errs_p, errs_t, step0)
        assert gap >= 1e-5, (r, direction, gap)
        worst["S"], worst["propose"] = max(worst["S"], err_S), max(worst["propose"], max(errs_p))
        worst["log T"], worst["gap"], worst["cond"] = max(worst["log T"], max(errs_t)), min(worst["gap"], gap), max(worst["cond"], cond)
    figures[r] = worst
