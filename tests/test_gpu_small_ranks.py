"""GPU: every route the library takes at ranks 1..64, at the ranks where one of them changes (tests/small_rank_ladder.py: LADDER, derived
from the restated dispatch and pinned by tests/test_small_rank_ladder_cpu.py, which also shows the reference sound at every one of
them) — instance, posterior, propose and transition, warm-started decompositions, the Cholesky-root sampler, the merged step, model
projection and posterior models per rank; the chain against the oracle, the smallest and largest split-K, a call that mixes ranks and
models made by gp_models at a few of them.

Models: the first r components of the bundled femur models, one context per rank.  References: the CPU oracle, numpy's eigh of
N' = D⁻¹MD⁻¹ from the oracle's M, the numpy long forms.  No bar is this module's own: REL and the literal bars of
tests/test_gpu_parity.py (1e-7 for V column by column and for proposed coefficients, 1e-8 for transition densities, 1e-6 for the z = 0
step; the root sampler's 1e-12 / 1e-13 / 1e-14 / 1e-9), check_decomposition of tests/test_gpu_eigen_spectra.py, bound_of of
tests/test_gpu_model_projection.py, check_against_long_form of tests/test_gpu_posterior_models.py, the chain test's 1e-5 / 1e-6.

V column by column against the oracle is conditioning-limited (eps·μ_max / gap): it is asserted for every column at the parity state of
each rank, where the CPU test has shown every gap to be at least 1e-5·μ_max, and at the warm-start states — the device's own
proposals, whose gaps nobody chose — for the columns whose eigenvalue is that far from both neighbours (the others are covered by
check_decomposition's projectors; over the ladder every warm-start state kept all of its columns, only K = 1 at rank 64 dropped
four and two of its 64).  The figures are printed per rank; the worst over the ladder are in DESIGN.md §9.2.

Two findings of the module's first run on an MI355X.  (1) At rank 64 the merged step's transition densities differed from the separate
calls' in the last bit: the finish launch chose the threads per row of its tails by its own 512 threads (8 at rank 64) where
k_transition_tails<256> takes 4 — fixed in launch_step_finish, test_merged_step_matches_separate_calls[rank64].  (2) The root
sampler's comparison with the eigen form missed 1e-12 at five ranks, by the Jacobi kernel's loose stopping test — tightened from 4e-6
to 5e-7: see test_cholesky_root_sampler."""
import numpy as np
import pytest

import small_rank_ladder as SR
from conftest import make_theta, oracle_chains_parallel
from test_gpu_chain import oracle_chain_config
from test_gpu_eigen_spectra import check_decomposition
from test_gpu_gp_models import run_items as run_gp_items
from test_gpu_model_projection import LongForm, bound_of, unposed
from test_gpu_parity import REL, rel_err
from test_gpu_posterior_models import check_against_long_form, observations, random_spd, run_items, same_bits

pytestmark = pytest.mark.gpu

STEP, SIGMA_T, SIGMA_N = 0.1, 10.0, 5.0  # the parity configuration
GAP = 1e-5                               # of μ_max: where the column bar of 1e-7 holds (tests/test_small_rank_ladder_cpu.py)

WORST = {}  # check -> (figure, rank): the largest figure of every check over the module's run, printed at the end


def note(check, value, r):
    value = float(value)
    if check not in WORST or value > WORST[check][0]:
        WORST[check] = (value, r)
    return value


@pytest.fixture(scope="module", autouse=True)
def worst_figures():
    WORST.clear()
    yield
    for check in sorted(WORST):
        print(f"worst over the ladder: {check} {WORST[check][0]:.2e} at rank {WORST[check][1]}")


class Case:
    """one rank: the truncated model and its target, ONE context, the oracle's handles"""

    def __init__(self, pkg, oracle, model, target):
        self.pkg, self.oracle, self.model, self.target, self.r = pkg, oracle, model, target, model.rank
        self.om, self.ot = oracle.OracleModel.from_model(model), oracle.OracleMesh(target.points, target.cells)
        self.ctx = pkg.IcpContext(model, target, device=0)

    def proposals(self, K, sampler=None):
        """-> {direction: (device proposal, oracle parameters)}"""
        out = {}
        for d in SR.DIRECTIONS:
            pp, tp = SR.oracle_params(self.oracle, self.pkg, self.target, K, d, STEP, SIGMA_T, SIGMA_N)
            prop = self.pkg.NonRigidIcpProposal(self.ctx, STEP, SIGMA_T, SIGMA_N, K, d, True, decimatedTargetPoints=tp)
            out[d] = (prop.setSampler(sampler) if sampler else prop, pp)
        return out

    def oracle_ahead(self, pps, theta, zs):
        """the oracle's answers for one state are about to be asked for (a Case whose oracle is slow may compute them side by side)"""

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module", params=SR.LADDER, ids=lambda r: f"rank{r}")
def case(request, pkg, oracle):
    c = Case(pkg, oracle, *SR.ladder_model(pkg, request.param))
    yield c
    c.close()


# ---------------------------------------------------------------- the checks, on any Case

def check_instance(c, tag):
    """(a) transformedMesh == OracleModel.instance for three seeds, for pose moves off a cached state and a shape move after them, and
    transformed_meshes (k_instance_many) gives the same bits"""
    model, ctx, om = c.model, c.ctx, c.om
    thetas = [make_theta(model, seed) for seed in range(3)]
    for t in thetas:
        assert np.array_equal(ctx.transformedMesh(t), om.instance(t)), tag
    rng = np.random.default_rng(5)
    theta = make_theta(model, 4)
    assert np.array_equal(ctx.transformedMesh(theta), om.instance(theta)), tag
    for k in range(6):
        t = theta.copy()
        t[0] = 1.0 + 0.01 * rng.normal() if k == 3 else t[0]
        t[1:4] += rng.normal(size=3)
        t[4:7] += 0.02 * rng.normal(size=3)
        t[7:10] += rng.normal(size=3) if k == 4 else 0.0
        if k == 5:
            t[10:] += 0.05 * rng.normal(size=model.rank)   # a shape move: from the basis again
        assert np.array_equal(ctx.transformedMesh(t), om.instance(t)), (tag, k)
        thetas.append(t)
        theta = t
    many = c.pkg.transformed_meshes(ctx, np.stack(thetas))
    for s, t in enumerate(thetas):
        assert np.array_equal(many[s], om.instance(t)), (tag, s)


def check_posterior(c, prop, pp, theta, tag, all_columns):
    """(b) -> the oracle's posterior"""
    r, model = c.r, c.model
    post = prop.icpPosterior(theta)
    po = c.oracle.icp_posterior(c.om, c.ot, pp, theta)
    assert np.array_equal(post.corr_id, po.corr_id), tag          # correspondences: bit-exact
    assert np.array_equal(post.keep, po.keep), tag
    assert np.array_equal(post.corr_aux, po.corr_aux), tag
    assert np.array_equal(post.corr_point, po.corr_pt), tag
    fig = {"M": rel_err(post.M, po.M), "alpha": rel_err(post.alpha, po.alpha), "S": rel_err(post.S, po.S)}
    Np = SR.n_prime(model, po.M)
    w = np.linalg.eigvalsh(Np)
    gaps = np.diff(w) / w[-1]
    gap = SR.smallest_relative_gap(Np)
    alone = np.concatenate([[True], gaps >= GAP]) & np.concatenate([gaps >= GAP, [True]])
    if all_columns:
        assert gap >= GAP, (tag, gap)  # (tests/test_small_rank_ladder_cpu.py)
        alone[:] = True
    # column j of V belongs to S[j], descending: to the j-th smallest eigenvalue of N'
    fig["V columns"] = float(np.abs(post.V - po.V)[:, alone].max()) if alone.any() else 0.0
    print(tag, {k: f"{v:.2e}" for k, v in fig.items()}, f"kept {int(po.keep.sum())}/{po.keep.size} gap {gap:.1e} columns {int(alone.sum())}/{r}")
    misses = check_decomposition(tag, Np, post.S, post.V)
    for k, v in fig.items():
        note(k, v, r)
    assert fig["M"] < REL and fig["alpha"] < REL and fig["S"] < REL, (tag, fig)
    assert fig["V columns"] < 1e-7, (tag, fig)                    # eigenvectors: conditioning ~ eps / relative gap
    assert not misses, misses
    return po


def state_zs(r, seed):
    """the two z of a state: zero and a random one"""
    return np.zeros(r), np.random.default_rng(seed).normal(size=r)


def check_propose_transition(c, prop, pp, theta, po, tag, seed):
    """(c) -> the device's proposal for the random z"""
    r, oracle = c.r, c.oracle
    worst_p, worst_t = 0.0, 0.0
    for z in state_zs(r, seed):
        got, corr = prop.propose(theta, z, return_correspondences=True)
        want = oracle.propose(c.om, c.ot, pp, theta, z)
        assert np.array_equal(got[:10], theta[:10]), tag
        worst_p = max(worst_p, rel_err(got[10:], want[10:]))
        assert np.array_equal(corr, np.where(po.keep == 1, po.corr_id, -1)), tag
        for a, b, oa, ob in ((theta, got, theta, want), (got, theta, want, theta)):   # forward, backward
            lt = prop.logTransitionProbability(a, b)
            lo = oracle.log_transition(c.om, c.ot, pp, oa, ob)
            assert np.isfinite(lt) and np.isfinite(lo), (tag, lt, lo)
            worst_t = max(worst_t, abs(lt - lo) / abs(lo))
    # z = 0: the proposal moves the coefficients towards the posterior mean by exactly stepLength
    got0 = prop.propose(theta, np.zeros(r))
    step0 = rel_err(got0[10:], theta[10:] + STEP * (po.alpha - theta[10:]))
    print(tag, f"propose {worst_p:.2e} log T {worst_t:.2e} z=0 step {step0:.2e}")
    note("propose", worst_p, r), note("log T", worst_t, r), note("z = 0 step", step0, r)
    assert worst_p < 1e-7 and worst_t <= 1e-8 and step0 < 1e-6, (tag, worst_p, worst_t, step0)
    # anything but the shape differs -> -inf
    other = got.copy()
    other[1] += 0.1
    assert prop.logTransitionProbability(theta, other) == -np.inf, tag
    return got


def check_posterior_propose_transition(c, K, n_states, tag, gaps_shown=True, theta=None):
    """(b) and (c) in both directions at the parity state (theta, where the rank's is not small_rank_ladder's), then (d) at
    n_states − 1 further states, each the previous one's proposal: the decomposition starts from the previous state's basis.
    gaps_shown: the CPU test has shown the parity state's gaps for this K"""
    props = c.proposals(K)
    theta = SR.parity_theta(c.model) if theta is None else theta
    for s in range(n_states):
        nxt = None
        c.oracle_ahead([pp for _, pp in props.values()], theta, state_zs(c.r, 200 + 10 * s + c.r))
        for d in SR.DIRECTIONS:
            prop, pp = props[d]
            t = f"{tag} {d} state {s}"
            po = check_posterior(c, prop, pp, theta, t, all_columns=gaps_shown and s == 0)
            got = check_propose_transition(c, prop, pp, theta, po, t, 200 + 10 * s + c.r)
            nxt = got if nxt is None else nxt
        theta = nxt
    assert all(v == 0 for v in c.ctx.runtime_stats().values()), (tag, c.ctx.runtime_stats())
    for prop, _ in props.values():
        prop.close()


# ---------------------------------------------------------------- per rank of the ladder

def test_instance(case):
    check_instance(case, f"rank {case.r}")


def test_posterior_propose_transition_cold_and_warm(case):
    """(b), (c), (d): K = 2r, three consecutive states"""
    check_posterior_propose_transition(case, 2 * case.r, 3, f"rank {case.r}")


ROOT_BARS = {"root diag": 1e-14, "root LLt": 1e-13, "root cov vs eigen": 1e-12, "root cov vs DM⁻¹D": 1e-12, "root propose": 1e-9}


def root_sampler_misses(c, bars=ROOT_BARS):
    """(e) the body of test_cholesky_root_sampler_has_the_posterior_covariance (tests/test_gpu_parity.py) on a Case; every figure is
    printed before any is judged -> the misses [(tag, figure, value), ...]"""
    model, r, pkg, ctx = c.model, c.r, c.pkg, c.ctx
    tp = pkg.data.decimated_point_subset(c.target, 2 * r)
    rng = np.random.default_rng(3)
    misses = []
    P = np.linalg.inv(SR.gram(model) + SR.SIGMA2 * np.eye(r))
    sl = np.sqrt(model.variance)
    for direction in SR.DIRECTIONS:
        pe = pkg.NonRigidIcpProposal(ctx, STEP, SIGMA_T, SIGMA_N, 2 * r, direction, True, decimatedTargetPoints=tp)
        pr = pkg.NonRigidIcpProposal(ctx, STEP, SIGMA_T, SIGMA_N, 2 * r, direction, True, decimatedTargetPoints=tp).setSampler("cholesky-root")
        for seed in (1, 2):
            theta = make_theta(model, seed, pose=True)
            a, b = pe.icpPosterior(theta), pr.icpPosterior(theta)
            assert np.array_equal(a.corr_id, b.corr_id) and np.array_equal(a.alpha, b.alpha) and np.array_equal(a.M, b.M)
            cov_e = (a.V * a.S[None, :]) @ a.V.T
            Lg = b.V   # root mode: the factor itself, V = L (M = L·Lᵀ, lower triangular), S = 1/diag(L)
            assert np.allclose(np.tril(Lg), Lg)
            want_cov = (sl[:, None] * np.linalg.inv(a.M)) * sl[None, :]
            W = sl[:, None] * np.linalg.inv(Lg).T
            cov_r = W @ W.T
            z = rng.normal(size=r)
            got = pr.propose(theta, z)
            L = np.linalg.cholesky(0.5 * (a.M + a.M.T))
            w = a.alpha + np.linalg.solve(L.T, z)
            cnew = w - SR.SIGMA2 * (P @ w)
            want = theta[10:] + STEP * (cnew - theta[10:])
            fig = {"root diag": np.abs(b.S * np.diag(Lg) - 1.0).max(), "root LLt": np.abs(Lg @ Lg.T - a.M).max() / np.abs(a.M).max(),
                   "root cov vs eigen": np.abs(cov_r - cov_e).max() / np.abs(cov_e).max(),
                   "root cov vs DM⁻¹D": np.abs(cov_r - want_cov).max() / np.abs(want_cov).max(),
                   "root propose": np.abs(got[10:] - want).max() / np.abs(want).max()}
            tag = f"rank {r} {direction} seed {seed}"
            print(tag, {k: f"{v:.2e}" for k, v in fig.items()})
            for k, v in fig.items():
                note(k, v, r)
                if not v <= bars[k]:
                    misses.append((tag, k, float(v)))
            assert np.array_equal(got[:10], theta[:10])
            other = pe.propose(theta, z)
            for to in (got, other):
                assert pe.logTransitionProbability(theta, to) == pr.logTransitionProbability(theta, to)
            assert np.isfinite(pr.logTransitionProbability(theta, got))
        pr.setSampler("eigen")   # switching back: the eigen form again
        cb = pr.icpPosterior(theta)
        assert np.abs(cb.S - a.S).max() <= 1e-10 * a.S.max() and np.abs(cb.V - a.V).max() <= 1e-7
        pe.close(); pr.close()
    assert all(v == 0 for v in ctx.runtime_stats().values())
    return misses


def test_cholesky_root_sampler(case):
    """(e) W = D·L⁻ᵀ of the Cholesky-root sampler has the covariance of the eigen form and of D·M⁻¹·D; the proposal is the closed form
    with that root; the transition density does not depend on the sampler.  (Ranks 1 and 2: the factor comes from the posterior's own
    factorisation, from 3 on from k_posterior_root.)

    On the first run five ranks missed W·Wᵀ against the EIGEN form's V·S·Vᵀ (bar 1e-12 of the largest entry): 1.39e-12 at rank 20,
    5.93e-12 at 26, 1.40e-12 at 33, 5.82e-12 at 49, 1.17e-12 at 64, all TargetSampling — while W·Wᵀ against D·M⁻¹·D from numpy was within
    2.7e-15 at every rank.  The eigen form missed: k_posterior_eigen_rr's loose test let |X_ij| reach 4e-6, and its first-order
    correction V·(I + X) leaves VᵀV − I = −X².  The test is 5e-7 now (kernels_eigen.hip: ICP_LOOSE_TAU): worst over the ladder 2.7e-13."""
    misses = root_sampler_misses(case)
    assert not misses, misses


def check_merged_step(c, tail_rel=0.0, Kp=None, Ke=None):
    """(f) test_chain_step_matches_separate_calls of tests/test_gpu_parity.py (independent evaluator) at the rank, on this rank's
    context and a second one for the separate calls; every third step accepted, so that steps begin while the decomposition of a newly
    accepted state is pending (k_step_begin_reg<52> / <64> from rank 32 on).  All six steps take the merged path, no fall-back runs.
    tail_rel: how far a transition density of the merged step may be from the separate call's, of its size — 0 up to rank 64: the same
    bits; above, where the finish launch sums the tails' products over its own threads, what tests/test_gpu_chain.py allows.
    Kp, Ke: sample points of the two proposals and of the evaluator, 2r and 4r unless given (tests/test_gpu_counts.py)."""
    same = lambda x, y: abs(x - y) <= tail_rel * abs(y)
    model, target, r, pkg = c.model, c.target, c.r, c.pkg
    Kp, Ke = 2 * r if Kp is None else Kp, 4 * r if Ke is None else Ke
    tp = pkg.data.decimated_point_subset(target, Kp)
    ctx_a, ctx_b = c.ctx, pkg.IcpContext(model, target, device=0)   # separate contexts: separate caches and search hints

    def mk(ctx):
        props = [pkg.NonRigidIcpProposal(ctx, STEP, SIGMA_T, SIGMA_N, Kp, d, True, decimatedTargetPoints=tp) for d in ("TargetSampling", "ModelSampling")]
        return props, pkg.IndependentPointDistanceEvaluator(ctx, 0.0, 2.0, 0, Ke)
    (props_a, ev_a), (props_b, ev_b) = mk(ctx_a), mk(ctx_b)
    before = ctx_a.step_paths()
    cur = make_theta(model, 600, pose=False)
    rng = np.random.default_rng(3)
    close = lambda x, y: np.allclose(x, y, rtol=1e-10, atol=1e-11)
    for step in range(6):
        gen = step % 3 - 1 if step else 0          # 0, 0, 1, -1, 0, 1
        z = rng.normal(size=r)
        if gen >= 0:
            prop_b = props_b[gen].propose(cur, z)
            prop_a, val, fwd, bwd = pkg.chain_step(ev_a, props_a, cur, generator=gen, z=z)
            assert close(prop_a, prop_b), step
            val, fwd, bwd = pkg.chain_eval_step(ev_a, props_a, cur, prop_b)   # both paths at the SAME state from here on
        else:
            prop_b = cur.copy()
            prop_b[10:] += 0.1 * z
            prop_a, val, fwd, bwd = pkg.chain_step(ev_a, props_a, cur, generator=-1, theta_prop=prop_b)
            assert np.array_equal(prop_a, prop_b), step
        assert val == ev_b.logValue(prop_b), step   # no eigen-decomposition behind these: bit-identical
        for i, p in enumerate(props_b):
            want_f, want_b = p.logTransitionProbability(cur, prop_b), p.logTransitionProbability(prop_b, cur)
            note("merged step's densities", max(abs(fwd[i] - want_f) / abs(want_f), abs(bwd[i] - want_b) / abs(want_b)), r)
            assert same(fwd[i], want_f), (step, i, fwd[i], want_f)
            assert same(bwd[i], want_b), (step, i, bwd[i], want_b)
        assert ev_a.logValue(prop_b) == val
        assert same(props_a[0].logTransitionProbability(cur, prop_b), fwd[0])
        pa, pb = props_a[1].icpPosterior(prop_b, with_aux=False), props_b[1].icpPosterior(prop_b, with_aux=False)
        assert np.array_equal(pa.corr_id, pb.corr_id) and np.array_equal(pa.M, pb.M) and np.array_equal(pa.alpha, pb.alpha)
        assert close(pa.S, pb.S)
        if step % 3 == 2:
            cur = prop_b   # "accept"
    paths = ctx_a.step_paths()
    taken = {k: paths[k] - before[k] for k in paths}
    print(f"rank {r} step paths {taken}")
    assert taken == {"merged": 6, "wide": 0, "per_stage": 0, "device_loop": 0}, taken
    for ctx in (ctx_a, ctx_b):
        assert all(v == 0 for v in ctx.runtime_stats().values()), ctx.runtime_stats()
    for o in props_a + props_b + [ev_a, ev_b, ctx_b]:
        o.close()


def test_merged_step_matches_separate_calls(case):
    """(f): the bits of the separate calls"""
    check_merged_step(case)


def check_projection(c):
    """(h) coefficients of instances and of noisy instances against the regularised solve (k_proj_gemm / k_proj_solve, the rank padded
    to 16)"""
    model, r, pkg, ctx = c.model, c.r, c.pkg, c.ctx
    lf = LongForm(model)
    rng = np.random.default_rng(r)
    th = [unposed(make_theta(model, 10 * r + s, shape_scale=1.0)) for s in range(4)]
    inst = pkg.transformed_meshes(ctx, th)
    noisy = inst + rng.normal(size=inst.shape)
    for kind, kw, meshes in (("points", dict(meshes=list(inst)), inst), ("thetas", dict(thetas=th), inst), ("noisy", dict(meshes=list(noisy)), noisy)):
        got = pkg.model_coefficients(ctx, **kw)
        assert got.shape == (4, r)
        for s in range(4):
            want = lf.coefficients(meshes[s])
            err = np.abs(got[s] - want).max()
            note("coefficients / bound", err / bound_of(want), r)
            assert err <= bound_of(want), (r, kind, s, err, bound_of(want))
    assert np.array_equal(ctx.coefficients(noisy[1]), pkg.model_coefficients(ctx, meshes=list(noisy))[1])
    print(f"rank {r}: worst |c - long form| / bound so far {WORST['coefficients / bound'][0]:.3e}")
    assert all(v == 0 for v in ctx.runtime_stats().values())


def check_posterior_models(c):
    """(h) posterior models at isotropic and at 3 × 3 noise against the long form (k_pm_*)"""
    model, r, pkg, ctx = c.model, c.r, c.pkg, c.ctx
    ids, y = observations(model, 200, 10 + r)
    cov = random_spd(200, 20 + r)
    res = pkg.posterior_models(ctx, [ids] * 2, [y] * 2, sigma2=[0.1, None], covariances=[None, cov])
    check_against_long_form(model, res[0], ids, y, 0.1, None, f"rank {r} sigma2=0.1")
    check_against_long_form(model, res[1], ids, y, None, cov, f"rank {r} 3x3")
    assert all(v == 0 for v in ctx.runtime_stats().values())


def test_projection_and_posterior_models(case):
    check_projection(case)
    check_posterior_models(case)


# ---------------------------------------------------------------- at a few ranks

def test_posterior_models_of_three_ranks_in_one_call(pkg):
    """(h) one call over contexts of ranks 3, 33 and 64, both noise forms: every item has the bits it has alone, and meets the long form"""
    ctxs = [pkg.IcpContext(*SR.ladder_model(pkg, r), device=0) for r in (3, 33, 64)]
    items = []
    for k in range(6):
        ctx = ctxs[k % 3]
        ids, y = observations(ctx.model, 40 + 37 * k, 300 + k)
        iso = k % 2 == 0
        items.append((ctx, ids, y, (0.1 + 0.2 * k) if iso else None, None if iso else random_spd(ids.shape[0], 400 + k)))
    whole = run_items(pkg, items, list(range(6)))
    back = run_items(pkg, items, list(range(6))[::-1])
    for k, (ctx, ids, y, s2, cov) in enumerate(items):
        assert same_bits(whole[k], run_items(pkg, items, [k])[k]) and same_bits(whole[k], back[k]), k
        check_against_long_form(ctx.model, whole[k], ids, y, s2, cov, f"mixed item {k} rank {ctx.rank}")
    for ctx in ctxs:
        ctx.close()


@pytest.fixture(scope="module")
def oracle_chains(pkg, oracle):
    """the oracle's 30-step chains of CHAIN_RANKS, all at once on a host thread each (the longest, rank 64, takes about 6 s)"""
    jobs, keep = [], {}
    for r in SR.CHAIN_RANKS:
        model, target = SR.ladder_model(pkg, r)
        setup = pkg.femur_icp_proposal_registration(model, target, fused=2)
        om, ot = oracle.OracleModel.from_model(model), oracle.OracleMesh(target.points, target.cells)
        keep[r] = (model, target, setup, om, ot)
        jobs.append((om, ot, oracle_chain_config(oracle, setup), pkg.initial_parameters(model), 1024, 30))
    return {r: (keep[r], res) for r, res in zip(SR.CHAIN_RANKS, oracle_chains_parallel(oracle, jobs))}


@pytest.mark.parametrize("r", SR.CHAIN_RANKS)
def test_chain_matches_oracle(pkg, oracle_chains, r):
    """(g) test_femur50_chain_matches_oracle of tests/test_gpu_chain.py over 30 steps: the same decisions, states within 1e-5, log
    posterior values within 1e-6"""
    (model, target, setup, om, ot), (acc_o, comp_o, logp_o, states_o) = oracle_chains[r]
    n_steps, seed = 30, 1024
    ctx = pkg.IcpContext(model, target, device=0)
    chain = pkg.SamplingRegistration(ctx, setup, pkg.initial_parameters(model), seed)
    rec = chain.run(n_steps)
    assert np.array_equal(rec[:, 0], np.arange(n_steps))
    assert np.array_equal(rec[:, 1].astype(np.uint8), acc_o), "accept/reject sequences differ"
    assert np.array_equal(rec[:, 2].astype(np.int32), comp_o), "mixture components differ"
    assert acc_o.sum() > 5 and (comp_o == 2).sum() > 0 and (comp_o == 0).sum() > 0 and (comp_o == 1).sum() > 0
    scale = np.abs(states_o[:, 10:]).max()
    err_s, err_l = np.abs(rec[:, 4 + 10:] - states_o[:, 10:]).max() / scale, np.abs(rec[:, 3] - logp_o).max() / np.abs(logp_o).max()
    print(f"rank {r}: accepted {int(acc_o.sum())}/{n_steps}, states {err_s:.2e}, log posterior {err_l:.2e}")
    note("chain states", err_s, r), note("chain log posterior", err_l, r)
    assert err_s <= 1e-5 and err_l <= 1e-6
    theta, logp, n, a = chain.state()
    assert n == n_steps and a == acc_o.sum()
    assert all(v == 0 for v in ctx.runtime_stats().values()), ctx.runtime_stats()
    chain.close()
    ctx.close()


@pytest.mark.parametrize("K", ["one", "all"])
@pytest.mark.parametrize("r", SR.K_EDGE_RANKS)
def test_smallest_and_largest_split_k(pkg, oracle, r, K):
    """(i) (b) and (c) with one sample point and with every vertex: regression_splits' smallest and largest split-K"""
    c = Case(pkg, oracle, *SR.ladder_model(pkg, r))
    oracle.set_search_backend(oracle.SEARCH_TREES)  # (bit-identical to the scans: tests/test_oracle.py; 1,622 queries a posterior)
    try:
        check_posterior_propose_transition(c, 1 if K == "one" else c.model.n_points, 1, f"rank {r} K={K}", gaps_shown=False)
    finally:
        oracle.set_search_backend(oracle.SEARCH_BRUTE)
        c.close()


GP_ITEMS = [("femur", "femur", 1, 1, 0.0), ("femur", "femur", 2, 2, 0.0), ("femur", "femur", 5, 5, 0.0)]


def test_models_made_by_gp_models_register(pkg, oracle, femur50):
    """(j) the femur-mesh items (1, 1), (2, 2) and (5, 5) of tests/test_gpu_gp_models.py from one gp_models call: each is a valid
    model description — it makes a context whose instances and ModelSampling posterior are the oracle's on the returned arrays"""
    _, target = femur50
    got = run_gp_items(pkg, GP_ITEMS, want=("variance", "basis"))
    for (_, _, m, r, _), (model, info) in zip(GP_ITEMS, got):
        assert info["rank"] == r and model.rank == r and model.n_points == target.n_points
        c = Case(pkg, oracle, model, target)
        tag = f"gp model rank {r}"
        check_instance(c, tag)
        pp, tp = SR.oracle_params(oracle, pkg, target, 2 * r, "ModelSampling", STEP, SIGMA_T, SIGMA_N)
        prop = pkg.NonRigidIcpProposal(c.ctx, STEP, SIGMA_T, SIGMA_N, 2 * r, "ModelSampling", True)
        check_posterior(c, prop, pp, make_theta(model, 100), tag, all_columns=False)
        assert all(v == 0 for v in c.ctx.runtime_stats().values())
        prop.close()
        c.close()
