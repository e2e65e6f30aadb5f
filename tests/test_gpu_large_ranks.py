"""GPU: every route the library takes at ranks 65..500, at the ranks where one of them changes (tests/large_rank_ladder.py: LADDER,
derived from the restated dispatch and pinned by tests/test_large_rank_ladder_cpu.py, which also shows the reference sound at every one
of them) — instance, posterior, propose and transition at three consecutive states, the Cholesky-root sampler up to 256 and its refusal
above, the merged step where a finish plan exists and the path the library names elsewhere, model projection at every rank and
posterior models up to their limit; short chains against the oracle at eight ranks, the on-device loop on both sides of 128 | 129,
rank 500 on its own, the refusal of 501.

Models: the first r components of femur-100 (65..101) and femur-200 (102..201) on the closed femur target, the synthetic face model on
its open target above.  References: the CPU oracle, numpy's eigh of N' = D⁻¹MD⁻¹ from the oracle's M, the numpy long forms.  The
checks are those of tests/test_gpu_small_ranks.py, "on any Case", and no bar is this module's own: REL and the literal bars of
tests/test_gpu_parity.py (1e-7 for V column by column and for proposed coefficients, 1e-8 for transition densities, 1e-6 for the
z = 0 step), check_decomposition of tests/test_gpu_eigen_spectra.py, bound_of of tests/test_gpu_model_projection.py,
check_against_long_form of tests/test_gpu_posterior_models.py, the chain test's 1e-5 / 1e-6; the root sampler's factor at the bars of
test_cholesky_root_sampler_at_large_ranks (tests/test_gpu_face.py: 1e-13 for S·diag L − 1, 1e-12 for L·Lᵀ − M, 1e-8 for the
proposal, equal transition densities) and its covariance at §9.2(e)'s 1e-12; the merged step's transition densities at the 1e-13 of
tests/test_gpu_chain.py ("the last bit or two" above rank 64), everything else of that step bit for bit.

The oracle's posterior takes 0.04..2.6 s at these ranks on a CPU (6.5 s at rank 500), and one state of (b) + (c) asks for fourteen of
them: a LargeCase computes a state's answers side by side on host threads before the checks ask for them (the oracle is a
single-threaded program per call; ctypes releases the GIL).  The figures are printed per rank; the worst are in DESIGN.md §9.3."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import large_rank_ladder as LR
import test_gpu_small_ranks as SMALL   # (the module, not its names: its parametrised fixtures and tests stay there)
from conftest import oracle_chains_parallel
from test_gpu_chain import oracle_chain_config

pytestmark = pytest.mark.gpu

ROOT_BARS = {"root diag": 1e-13, "root LLt": 1e-12, "root cov vs eigen": 1e-12, "root cov vs DM⁻¹D": 1e-12, "root propose": 1e-8}
MERGED_TAIL_REL = 1e-13


@pytest.fixture(scope="module", autouse=True)
def worst_figures():
    SMALL.WORST.clear()
    yield
    for check in sorted(SMALL.WORST):
        print(f"worst over the ladder: {check} {SMALL.WORST[check][0]:.2e} at rank {SMALL.WORST[check][1]}")
    SMALL.WORST.clear()


class AheadOracle:
    """the oracle module, with the answers of LargeCase.oracle_ahead remembered: same functions, same values"""

    def __init__(self, oracle):
        self._o, self.memo = oracle, {}

    def __getattr__(self, name):
        return getattr(self._o, name)

    @staticmethod
    def key(kind, pp, *arrays):
        return (kind, id(pp)) + tuple(np.asarray(a, dtype=np.float64).tobytes() for a in arrays)

    def icp_posterior(self, om, ot, pp, theta):
        k = self.key("posterior", pp, theta)
        return self.memo[k] if k in self.memo else self._o.icp_posterior(om, ot, pp, theta)

    def propose(self, om, ot, pp, theta, z):
        k = self.key("propose", pp, theta, z)
        return self.memo[k] if k in self.memo else self._o.propose(om, ot, pp, theta, z)

    def log_transition(self, om, ot, pp, a, b):
        k = self.key("log T", pp, a, b)
        return self.memo[k] if k in self.memo else self._o.log_transition(om, ot, pp, a, b)


class LargeCase(SMALL.Case):
    def __init__(self, pkg, oracle, model, target):
        super().__init__(pkg, oracle, model, target)
        self.oracle = AheadOracle(oracle)

    def oracle_ahead(self, pps, theta, zs, both_ways=True):
        o, memo = self.oracle._o, self.oracle.memo
        memo.clear()
        with ThreadPoolExecutor(max_workers=16) as ex:
            first = {AheadOracle.key("posterior", pp, theta): ex.submit(o.icp_posterior, self.om, self.ot, pp, theta) for pp in pps}
            want = {(id(pp), k): ex.submit(o.propose, self.om, self.ot, pp, theta, z) for pp in pps for k, z in enumerate(zs)}
            for pp in pps:
                for k, z in enumerate(zs):
                    w = want[id(pp), k].result()
                    memo[AheadOracle.key("propose", pp, theta, z)] = w
                    first[AheadOracle.key("log T", pp, theta, w)] = ex.submit(o.log_transition, self.om, self.ot, pp, theta, w)
                    if both_ways:
                        first[AheadOracle.key("log T", pp, w, theta)] = ex.submit(o.log_transition, self.om, self.ot, pp, w, theta)
            for k, f in first.items():
                memo[k] = f.result()


@pytest.fixture(scope="module", params=LR.LADDER, ids=lambda r: f"rank{r}")
def case(request, pkg, oracle):
    c = LargeCase(pkg, oracle, *LR.ladder_model(pkg, request.param))
    yield c
    assert all(v == 0 for v in c.ctx.runtime_stats().values()), c.ctx.runtime_stats()
    c.close()


# ---------------------------------------------------------------- per rank of the ladder

def test_instance(case):
    """(a)"""
    SMALL.check_instance(case, f"rank {case.r}")
    assert all(v == 0 for v in case.ctx.runtime_stats().values())


def check_rank_500(c, K, theta):
    """one posterior (b), one proposal and one density (c) per direction: check_posterior as it is, then the random z of a state
    forwards, at check_propose_transition's bars — and the pose change's −∞, which needs no oracle"""
    r = c.r
    props = c.proposals(K)
    z = SMALL.state_zs(r, 200 + r)[1]
    c.oracle_ahead([pp for _, pp in props.values()], theta, [z], both_ways=False)
    for d in LR.DIRECTIONS:
        prop, pp = props[d]
        tag = f"rank {r} {d}"
        po = SMALL.check_posterior(c, prop, pp, theta, tag, all_columns=True)
        got, corr = prop.propose(theta, z, return_correspondences=True)
        want = c.oracle.propose(c.om, c.ot, pp, theta, z)
        assert np.array_equal(got[:10], theta[:10]) and np.array_equal(corr, np.where(po.keep == 1, po.corr_id, -1)), tag
        err_p = SMALL.note("propose", SMALL.rel_err(got[10:], want[10:]), r)
        lt, lo = prop.logTransitionProbability(theta, got), c.oracle.log_transition(c.om, c.ot, pp, theta, want)
        assert np.isfinite(lt) and np.isfinite(lo), (tag, lt, lo)
        err_t = SMALL.note("log T", abs(lt - lo) / abs(lo), r)
        print(tag, f"propose {err_p:.2e} log T {err_t:.2e}")
        assert err_p < 1e-7 and err_t <= 1e-8, (tag, err_p, err_t)
        other = got.copy()
        other[1] += 0.1
        assert prop.logTransitionProbability(theta, other) == -np.inf, tag
    assert all(v == 0 for v in c.ctx.runtime_stats().values()), c.ctx.runtime_stats()
    for prop, _ in props.values():
        prop.close()


def test_posterior_propose_transition_at_three_states(case):
    """(b), (c), (d): K and the parity state of the rank (large_rank_ladder.parity_state), then two further states, each the previous
    proposal.  At 65..256 every state goes through the tridiagonal route, which takes no warm start; at 257 the generic kernel is the
    primary route with the matrix behind L2 and the warm start dropped (a_in_lds = 0).  Rank 500: one state, see check_rank_500."""
    c = case
    theta, K = LR.parity_theta(c.model), LR.parity_K(c.r)
    if c.r == LR.MAX_RANK:
        check_rank_500(c, K, theta)
    else:
        SMALL.check_posterior_propose_transition(c, K, 3, f"rank {c.r}", theta=theta)


def test_cholesky_root_sampler(case):
    """(e) up to 256: the factor the posterior's own factorisation hands out (Lout: k_posterior_factor_reg<1, 1024> to 125, <2, 1024> to
    127, k_posterior_factor_tiles<3> to 217, <4> to 253, the generic kernel to 256), the proposal through k_propose<1024> with
    matvec_tpr_log2(r, 1024) threads a row.  Above: refused, and the proposal works with the eigen sampler afterwards."""
    c = case
    if LR.root_sampler(c.r) != "refused":
        misses = SMALL.root_sampler_misses(c, ROOT_BARS)
        assert not misses, misses
        return
    r, pkg = c.r, c.pkg
    prop = pkg.NonRigidIcpProposal(c.ctx, SMALL.STEP, SMALL.SIGMA_T, SMALL.SIGMA_N, 2 * r, "ModelSampling", True)
    with pytest.raises(pkg._native.IcpNativeError, match="the Cholesky-root sampler covers ranks up to 256"):
        prop.setSampler("cholesky-root")
    theta = LR.parity_theta(c.model)
    z = np.random.default_rng(r).normal(size=r)
    post = prop.icpPosterior(theta)
    got = prop.propose(theta, z)
    G = LR.gram(c.model)
    want = LR.closed_form_propose(c.model, G, post.alpha, post.V, post.S, theta, z, SMALL.STEP)
    err = SMALL.rel_err(got[10:], want[10:])
    print(f"rank {r}: refused; the eigen sampler's proposal against the closed form on its own posterior {err:.2e}")
    assert err < 1e-7 and np.array_equal(got[:10], theta[:10])
    prop.setSampler("eigen")
    assert np.array_equal(prop.propose(theta, z), got)
    prop.close()
    assert all(v == 0 for v in c.ctx.runtime_stats().values())


def native_step_path(c, props, ev):
    hs = (C.c_void_p * len(props))(*[p.h for p in props])
    return {0: "merged", 1: "wide", 2: "per_stage"}[c.pkg._native.lib().icp_chain_step_path(ev.h, len(props), hs)]


def test_merged_step_or_the_path_in_its_place(case):
    """(f) where finish_plan gives a plan (65..116, the closed femur target): six steps against the separate calls, all six counted
    on the merged path — k_step_finish<2, 512> with both tails' matrices in LDS behind the factor (65..67), beside it (68..82), one of
    them (83..116).  Everywhere else: icp_chain_step_path names the path DISPATCH does, for the same proposals and evaluator."""
    c = case
    r, pkg = c.r, c.pkg
    closed = LR.closed_target(r)
    tp = pkg.data.decimated_point_subset(c.target, 2 * r)
    props = [pkg.NonRigidIcpProposal(c.ctx, SMALL.STEP, SMALL.SIGMA_T, SMALL.SIGMA_N, 2 * r, d, True, decimatedTargetPoints=tp)
             for d in ("TargetSampling", "ModelSampling")]
    ev = pkg.IndependentPointDistanceEvaluator(c.ctx, 0.0, 2.0, 0, 4 * r)
    path = native_step_path(c, props, ev)
    for o in props + [ev]:
        o.close()
    assert path == LR.step_path(r, closed), (r, path)
    if path == "merged":
        SMALL.check_merged_step(c, MERGED_TAIL_REL)


def test_projection_and_posterior_models(case):
    """(g) model projection at every rank (no limit of its own); posterior models up to kPmMaxRank, above it status −1 (invalid
    argument) for that item, its arrays absent, and the items beside it untouched"""
    c = case
    SMALL.check_projection(c)
    if LR.batched_limits(c.r)[0]:
        SMALL.check_posterior_models(c)
        return
    ids, y = SMALL.observations(c.model, 200, 10 + c.r)
    res = c.pkg.posterior_models(c.ctx, [ids], [y], sigma2=[0.1])
    assert res[0]["status"] == -1 and set(res[0]) == {"status"}, res[0].keys()
    assert all(v == 0 for v in c.ctx.runtime_stats().values())


# ---------------------------------------------------------------- at a few ranks

def test_rank_501_is_refused(pkg):
    model = pkg.data.synthetic_face_model(grid=LR.FACE_GRID, rank=LR.REFUSED_RANK)
    target = pkg.data.synthetic_partial_target(model, n_remove=LR.FACE_REMOVE)
    assert LR.context(model.rank) == "refused"
    with pytest.raises(pkg._native.IcpNativeError, match=r"rank must be in \[1,500\]"):
        pkg.IcpContext(model, target, device=0)


def test_posterior_models_beside_a_rank_above_the_limit(pkg):
    """one call over contexts of ranks 256 and 257: the 257 item is refused with −1, the 256 item has the bits it has alone"""
    ctxs = [pkg.IcpContext(*LR.ladder_model(pkg, r), device=0) for r in (256, 257)]
    obs = [SMALL.observations(ctx.model, 120, 500 + k) for k, ctx in enumerate(ctxs)]
    both = pkg.posterior_models(ctxs, [o[0] for o in obs], [o[1] for o in obs], sigma2=[0.2, 0.2])
    alone = pkg.posterior_models(ctxs[:1], [obs[0][0]], [obs[0][1]], sigma2=[0.2])[0]
    assert both[1]["status"] == -1 and set(both[1]) == {"status"}
    assert both[0]["status"] == 0 and SMALL.same_bits(both[0], alone)
    SMALL.check_against_long_form(ctxs[0].model, both[0], obs[0][0], obs[0][1], 0.2, None, "rank 256 beside 257")
    for ctx in ctxs:
        assert all(v == 0 for v in ctx.runtime_stats().values())
        ctx.close()


@pytest.fixture(scope="module")
def oracle_chains(pkg, oracle):
    """the oracle's chains of CHAIN_RANKS, all at once on a host thread each"""
    jobs, keep = [], {}
    for r in LR.CHAIN_RANKS:
        model, target = LR.ladder_model(pkg, r)
        setup, theta0, seed = LR.chain_setup(pkg, model, target)
        om, ot = oracle.OracleModel.from_model(model), oracle.OracleMesh(target.points, target.cells)
        keep[r] = (model, target, setup, theta0, seed)
        jobs.append((om, ot, oracle_chain_config(oracle, setup), theta0, seed, LR.CHAIN_STEPS[r]))
    return {r: (keep[r], res) for r, res in zip(LR.CHAIN_RANKS, oracle_chains_parallel(oracle, jobs))}


@pytest.mark.parametrize("r", LR.CHAIN_RANKS)
def test_chain_matches_oracle_on_the_path_dispatch_names(pkg, oracle_chains, r):
    """the femur study's chain on the closed target (65, 116: merged; 117, 129, 135: wide), BfmFittingPartial on the face model's open
    one (218, 254: wide; 257: per-stage): the oracle's decisions, states within 1e-5, log posterior values within 1e-6, every step
    on the path DISPATCH names for the rank and target"""
    (model, target, setup, theta0, seed), (acc_o, comp_o, logp_o, states_o) = oracle_chains[r]
    n_steps = LR.CHAIN_STEPS[r]
    ctx = pkg.IcpContext(model, target, device=0)
    chain = pkg.SamplingRegistration(ctx, setup, theta0, seed)
    rec = chain.run(n_steps)
    paths = ctx.step_paths()
    want_paths = {"merged": 0, "wide": 0, "per_stage": 0, "device_loop": 0}
    want_paths[LR.step_path(r, LR.closed_target(r))] = n_steps
    assert np.array_equal(rec[:, 0], np.arange(n_steps))
    assert np.array_equal(rec[:, 1].astype(np.uint8), acc_o), "accept/reject sequences differ"
    assert np.array_equal(rec[:, 2].astype(np.int32), comp_o), "mixture components differ"
    scale = np.abs(states_o[:, 10:]).max()
    err_s, err_l = np.abs(rec[:, 4 + 10:] - states_o[:, 10:]).max() / scale, np.abs(rec[:, 3] - logp_o).max() / np.abs(logp_o).max()
    print(f"rank {r}: accepted {int(acc_o.sum())}/{n_steps}, components {np.bincount(comp_o, minlength=3)}, states {err_s:.2e}, "
          f"log posterior {err_l:.2e}, paths {paths}")
    SMALL.note("chain states", err_s, r), SMALL.note("chain log posterior", err_l, r)
    assert err_s <= 1e-5 and err_l <= 1e-6
    assert paths == want_paths, (paths, want_paths)
    assert all(v == 0 for v in ctx.runtime_stats().values()), ctx.runtime_stats()
    chain.close()
    ctx.close()


@pytest.mark.parametrize("r", [128, 129])
def test_on_device_loop_on_both_sides_of_the_decide_kernels_edge(pkg, oracle, r):
    """k_mhw_decide<2> | <4> (and matvec_tpr_log2(r, ·), the tridiagonal shapes and the factor kernels, which change behind 128 as
    well, inside the loop's captured launches): two chains in icp_chains_run_on_device, every step counted by the loop, every
    decision the oracle's — test_femur200_on_device_loop_matches_oracle of tests/test_gpu_rank201.py at the rank"""
    model, target = LR.ladder_model(pkg, r)
    om, ot = oracle.OracleModel.from_model(model), oracle.OracleMesh(target.points, target.cells)
    B, n = 2, 6
    setup = pkg.femur_icp_proposal_registration(model, target, fused=2)
    ctxs = [pkg.IcpContext(model, target, device=0) for _ in range(B)]
    theta0 = [pkg.random_initial_parameters(model, 4 + b) for b in range(B)]
    chains = [pkg.SamplingRegistration(ctxs[b], setup, theta0[b], seed=900 + b) for b in range(B)]
    recs = pkg.run_chains_batched(chains, n)
    assert all(c.step_paths()["device_loop"] == n for c in ctxs), [c.step_paths() for c in ctxs]
    cfg = oracle_chain_config(oracle, setup)
    want = oracle_chains_parallel(oracle, [(om, ot, cfg, theta0[b], 900 + b, n) for b in range(B)])
    for b in range(B):
        acc_o, comp_o, logp_o, states_o = want[b]
        rec = recs[b]
        assert np.array_equal(rec[:, 1].astype(np.uint8), acc_o), f"chain {b}: accept/reject sequences differ"
        assert np.array_equal(rec[:, 2].astype(np.int32), comp_o), f"chain {b}: mixture components differ"
        err_s = np.abs(rec[:, 4 + 10:] - states_o[:, 10:]).max() / np.abs(states_o[:, 10:]).max()
        err_l = np.abs(rec[:, 3] - logp_o).max() / np.abs(logp_o).max()
        print(f"rank {r} chain {b}: accepted {int(acc_o.sum())}/{n}, states {err_s:.2e}, log posterior {err_l:.2e}")
        SMALL.note("loop states", err_s, r), SMALL.note("loop log posterior", err_l, r)
        assert err_s <= 1e-5 and err_l <= 1e-6
    for c in chains:
        c.close()
    for c in ctxs:
        assert all(v == 0 for v in c.runtime_stats().values()), c.runtime_stats()
        c.close()
