"""GPU: the batched entry points at the COUNTS where their kernels and host planners take another path (tests/batched_count_ladder.py:
the N, n, K, S, S_d, D, T / V and S_sum ladders and the pair, derived from the restated dispatch and pinned by
tests/test_batched_count_ladder_cpu.py, which also shows every designed input sound) — through the Python API and the C ABI.

(a) instances over N and n, two models of different N and rank in one launch, a group closed by the model change, poses on;
(b) coefficients over N as points and as states, with and without a pose, project_out on every second item; n over the groups of 16;
    the pair (N = 1, n = 32,752 | 32,753); a non-finite item at slots 15 and 16;
(c) posterior models over N at K = min(N, 40), over K at N = 600, n = 16, 17, 33, three ranks shuffled, an indefinite covariance at
    item 16, mean-only and basis-only calls;
(d) variability in modes 0, 1, 2 over N, over S, and at S = 32,767 | 32,768 | 32,769 on the one-triangle mesh;
(e) metrics on both sides of 4,096 model and target vertices, closed and open, T and V = 2,047 | 2,048, the Dice ladder, n = 64 | 65;
(f) log values over D for the three evaluator kinds, n = 256 | 257;
(g) registration maps at 255 | 256 | 257 rows and n = 64 | 65, summaries over the S_sum ladder;
(h) the test-hooks build: a projection chunk of one mesh, posterior-model pieces of exactly 48 rows.

Every assertion is one of three kinds.  Bit equality with the one-item entry (icp_transformed_mesh, ctx.coefficients / .project,
icp_mesh_metrics, icp_posterior_variability, the one-at-a-time log value, a call of the item alone; within a call the same item at the
first and the last slot of a group and in a group of one).  An independent reference at a bar the project already has, imported:
bound_of (coefficients), check_against_long_form (posterior models), ORACLE_REL of test_gpu_variability_many and of
test_gpu_log_values_many, array_equal for instances (test_gpu_small_ranks.check_instance), indices, counts and maxima.  Reduction
sums against math.fsum within batched_count_ladder.sum_bound, (D − 1)·2⁻⁵³·Σ|term| of the reference's own terms, which holds for any
summation order; an average adds the one rounding of its division (2⁻⁵³ of the average); the Gaussian log-pdf adds 4 ulp a term
(batched_count_ladder.gauss_bound says why).  No bar is this module's own."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import batched_count_ladder as BL
import count_ladder as CL
from conftest import ROOT
from test_gpu_log_values_many import COLLECTIVE, HAUSDORFF, INDEPENDENT, ORACLE_REL as LOG_REL, make_evaluator, one_item as one_log_value
from test_gpu_mesh_metrics_many import counts as dice_counts_of, five, one_item as one_metrics
from test_gpu_model_projection import LongForm, bound_of, unposed
from test_gpu_posterior_models import WANT, check_against_long_form, same_bits
from test_gpu_registration_maps import MAPS, fold, one_item as one_maps
from test_gpu_variability_many import ORACLE_REL as VAR_REL, one_map

pytestmark = pytest.mark.gpu

WORST = {}  # check -> (figure, where)


def note(check, value, where):
    value = float(value)
    if check not in WORST or value > WORST[check][0]:
        WORST[check] = (value, where)
    return value


@pytest.fixture(scope="module", autouse=True)
def worst_figures():
    WORST.clear()
    yield
    for check in sorted(WORST):
        print(f"worst over the batched count ladders: {check} {WORST[check][0]:.2e} at {WORST[check][1]}")


def clean(ctx):
    assert all(v == 0 for v in ctx.runtime_stats().values()), ctx.runtime_stats()


class Shape:
    """one model made from a count, its context (the target: the same mesh unless one is given) and the oracle's handle"""

    def __init__(self, pkg, oracle, N, r=None, closed=True, target_mesh=None, seed=41, mesh=None):
        mesh = BL.ladder_mesh(N, closed) if mesh is None else mesh
        assert mesh[0].shape[0] == N
        self.pkg, self.oracle, self.N = pkg, oracle, N
        self.model = CL.model_on(pkg, mesh, BL.rank_of(N) if r is None else r, seed)
        self.target = CL.as_target(pkg, mesh if target_mesh is None else target_mesh)
        self.ctx = pkg.IcpContext(self.model, self.target, device=0)
        self.om = oracle.OracleModel.from_model(self.model) if oracle is not None else None

    def done(self):
        clean(self.ctx)
        self.ctx.close()


def trees(oracle, on):
    """the oracle's KD-tree / BVH back end for the large searches (bit-identical to the scans: tests/test_oracle.py)"""
    oracle.set_search_backend(oracle.SEARCH_TREES if on else oracle.SEARCH_BRUTE)


# ---------------------------------------------------------------- the C ABI where the Python API is narrower

def _dp(pkg, arrs):
    dp = pkg._native.c_double_p
    return (dp * max(1, len(arrs)))(*[a.ctypes.data_as(dp) if a is not None else None for a in arrs])


def _cp(ctxs):
    return (ctypes.c_void_p * len(ctxs))(*[c.h for c in ctxs])


def instances_abi(pkg, ctxs, thetas):
    """icp_model_instances_many over contexts whose models may differ in N -> list of [N_b, 3]"""
    th = [np.ascontiguousarray(t, dtype=np.float64) for t in thetas]
    outs = [np.full((c.N, 3), -7.0) for c in ctxs]
    rc = pkg._native.lib().icp_model_instances_many(len(ctxs), _cp(ctxs), _dp(pkg, th), _dp(pkg, outs))
    assert rc == 0, rc
    return outs


def coefficients_abi(pkg, ctx, points, thetas, poses, project):
    """icp_model_coefficients_many with project_out given per item (project[b] true) -> (coeffs [n, r], [proj or None], status, rc)"""
    n = len(points)
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    pts, th, po = [f(a) for a in points], [f(a) for a in thetas], [f(a) for a in poses]
    coeffs, status = np.full((n, ctx.rank), -7.0), np.full(n, 99, dtype=np.int32)
    proj = [np.full((ctx.N, 3), -7.0) if project[b] else None for b in range(n)]
    nat = pkg._native
    rc = nat.lib().icp_model_coefficients_many(n, _cp([ctx] * n), _dp(pkg, pts), _dp(pkg, th), _dp(pkg, po), coeffs.ctypes.data_as(nat.c_double_p),
                                               _dp(pkg, proj), status.ctypes.data_as(nat.c_int_p))
    return coeffs, proj, status, rc


# ---------------------------------------------------------------- (a) instances

INSTANCE_NS = [(N, None) for N in BL.N_LADDER] + [(BL.RANK40_N["instances"], BL.RANKS[1])]
INSTANCE_ITEMS = (1, 7, 8, 9, 17)


@pytest.mark.parametrize("N,r", INSTANCE_NS, ids=[f"N{N}" + (f"-rank{r}" if r else "") for N, r in INSTANCE_NS])
def test_instances_over_n_and_items(pkg, oracle, N, r):
    """calls of 1, 7, 8, 9 and 17 states, poses on: every row is icp_transformed_mesh's and the oracle's instance, bit for bit; the
    same state at slot 0, at slot 7 (the last of a full group) and at slot 8 (a group of one) gives the same rows"""
    s = Shape(pkg, oracle, N, r)
    th = BL.states(s.model, 1000 + N, 17)
    want = [s.ctx.transformedMesh(t) for t in th]
    for b in range(17):
        assert np.array_equal(want[b], s.om.instance(th[b])), (N, b)
    for n in INSTANCE_ITEMS:
        got = pkg.transformed_meshes(s.ctx, th[:n])
        assert got.shape == (n, N, 3)
        for b in range(n):
            assert np.array_equal(got[b], want[b]), (N, n, b)
    again = pkg.transformed_meshes(s.ctx, np.concatenate([th[:7], th[:1], th[:1]]))
    assert np.array_equal(again[7], want[0]) and np.array_equal(again[8], want[0]) and np.array_equal(again[0], want[0]), N
    s.done()


def test_instances_of_two_models_in_one_launch(pkg, oracle):
    """models of N = 65 (rank 12) and N = 9 (rank 5) alternating: groups of one, the grid sized by the larger model, the smaller one's
    workgroups past its N returning at once; then 9 + 9 items: full group, group of one closed by the model change, full group, one"""
    a, b = Shape(pkg, oracle, 65), Shape(pkg, oracle, 9, r=5, seed=43)
    for order in ([a, b] * 5, [b, a] * 5, [a] * 9 + [b] * 9, [b] * 9 + [a] * 9):
        th = [BL.state(x.model, 300 + k) for k, x in enumerate(order)]
        got = instances_abi(pkg, [x.ctx for x in order], th)
        for k, x in enumerate(order):
            assert got[k].shape == (x.N, 3)
            assert np.array_equal(got[k], x.ctx.transformedMesh(th[k])), k
            assert np.array_equal(got[k], x.om.instance(th[k])), k
    a.done()
    b.done()


# ---------------------------------------------------------------- (b) coefficients

def mixed_projection_items(s, seed, n=6):
    """item b: as points (even) or as a state (odd), with a pose to take off where b % 4 >= 2, noisy (not in the span) where it is
    given as points without a pose -> (points, thetas, poses, the mesh the long form sees)"""
    rng = np.random.default_rng(seed)
    th = BL.states(s.model, seed, n, scale=1.0)
    pts, ths, poses, seen = [], [], [], []
    for b in range(n):
        as_theta, with_pose = b % 2 == 1, b % 4 >= 2
        posed = s.ctx.transformedMesh(th[b])
        if with_pose:   # the pose comes off: the long form sees the unposed instance
            seen.append(s.ctx.transformedMesh(unposed(th[b])))
            mesh = posed
        else:           # no pose to take off: the mesh as it stands is taken to be in model space
            mesh = posed if as_theta else posed + rng.normal(size=posed.shape)
            seen.append(mesh)
        pts.append(None if as_theta else mesh)
        ths.append(th[b] if as_theta else None)
        poses.append(th[b][:10].copy() if with_pose else None)
    return pts, ths, poses, seen


COEFF_NS = [(N, None) for N in BL.N_LADDER] + [(BL.RANK40_N["coefficients"], BL.RANKS[1])]


@pytest.mark.parametrize("N,r", COEFF_NS, ids=[f"N{N}" + (f"-rank{r}" if r else "") for N, r in COEFF_NS])
def test_coefficients_over_n(pkg, oracle, N, r):
    """six mixed items in one call, project_out on every second one: coefficients within bound_of of the numpy long form, each row the
    bits of the item alone, a projection the bits of icp_transformed_mesh([pose or identity | c])"""
    s = Shape(pkg, oracle, N, r)
    lf = LongForm(s.model)
    pts, ths, poses, seen = mixed_projection_items(s, 2000 + N)
    n = len(pts)
    project = [b % 2 == 0 for b in range(n)]
    got, proj, status, rc = coefficients_abi(pkg, s.ctx, pts, ths, poses, project)
    assert rc == 0 and not status.any()
    ident = np.zeros(10)
    ident[0] = 1.0
    for b in range(n):
        want = lf.coefficients(seen[b])
        err = np.abs(got[b] - want).max()
        note("coefficients / bound_of", err / bound_of(want), f"N {N} item {b}")
        assert err <= bound_of(want), (N, b, err, bound_of(want))
        alone = pkg.model_coefficients(s.ctx, meshes=[pts[b]], thetas=[ths[b]], poses=[poses[b]])
        assert np.array_equal(alone[0], got[b]), (N, b)
        if pts[b] is not None:
            assert np.array_equal(s.ctx.coefficients(pts[b], pose=poses[b]), got[b]), (N, b)
        if project[b]:
            pose = poses[b] if poses[b] is not None else ident
            assert np.array_equal(proj[b], s.ctx.transformedMesh(np.concatenate([pose, got[b]]))), (N, b)
            if pts[b] is not None:
                assert np.array_equal(s.ctx.project(pts[b], pose=poses[b]), proj[b]), (N, b)
    print(f"N {N}: slabs {BL.proj_slabs(N)} of {BL.proj_slab_rows(N)} rows, last trip {BL.proj_last_trip(N)}")
    s.done()


@pytest.mark.parametrize("N", [7, 86])
def test_coefficients_over_items(pkg, oracle, N):
    """n = 1, 15, 16, 17, 33 noisy meshes: every row the bits of the item alone and within bound_of of the long form; the same mesh at
    slot 0, at slot 15 (the last of a group) and at slot 16 (the first of the next); a NaN vertex at slot 15, then at slot 16: that
    item has status −3 and NaN, its neighbours keep their bits"""
    s = Shape(pkg, oracle, N)
    lf = LongForm(s.model)
    rng = np.random.default_rng(N)
    th = BL.states(s.model, 3000 + N, 33, pose=False, scale=1.0)
    meshes = [m + rng.normal(size=m.shape) for m in pkg.transformed_meshes(s.ctx, th)]
    meshes[15], meshes[16] = meshes[0].copy(), meshes[0].copy()
    alone = [s.ctx.coefficients(m) for m in meshes]
    for b in range(33):
        want = lf.coefficients(meshes[b])
        note("coefficients / bound_of", np.abs(alone[b] - want).max() / bound_of(want), f"N {N} alone {b}")
        assert np.abs(alone[b] - want).max() <= bound_of(want), (N, b)
    assert np.array_equal(alone[15], alone[0]) and np.array_equal(alone[16], alone[0])
    for n in (1, 15, 16, 17, 33):
        got, proj = pkg.model_coefficients(s.ctx, meshes=meshes[:n], want_project=True)
        for b in range(n):
            assert np.array_equal(got[b], alone[b]), (N, n, b)
        assert np.array_equal(proj[0], s.ctx.project(meshes[0])) and np.array_equal(proj[n - 1], s.ctx.project(meshes[n - 1])), (N, n)
    for bad in (15, 16):
        pts = [m.copy() for m in meshes]
        pts[bad][N // 2, 1] = np.nan
        got, proj, status, rc = coefficients_abi(pkg, s.ctx, pts, [None] * 33, [None] * 33, [True] * 33)
        assert rc == -3 and status[bad] == -3 and np.count_nonzero(status) == 1, (bad, rc, status)
        assert np.isnan(got[bad]).all() and np.isnan(proj[bad]).all()
        for b in range(33):
            if b != bad:
                assert np.array_equal(got[b], alone[b]), (N, bad, b)
    s.done()


@pytest.mark.parametrize("N,n", BL.PAIRS, ids=[f"N{N}-n{n}" for N, n in BL.PAIRS])
def test_projection_at_the_chunks_item_cap(pkg, oracle, N, n):
    """n one-vertex meshes: 32,752 fill one chunk, the 32,753rd opens a second one — without a test hook.  Coefficients: the items on
    both sides of the boundary, the first and the last equal the one-item call, every 997th is within bound_of of the long form.
    Instances (the same cap closes a round): the same items equal icp_transformed_mesh"""
    s = Shape(pkg, oracle, N)
    lf = LongForm(s.model)
    rng = np.random.default_rng(n)
    meshes = s.model.ref_points[None] + 5.0 * rng.normal(size=(n, N, 3))
    got = pkg.model_coefficients(s.ctx, meshes=list(meshes))
    look = sorted({0, 1, BL.K_PROJ_MAX_CHUNK_ITEMS - 1, min(BL.K_PROJ_MAX_CHUNK_ITEMS, n - 1), n - 1})
    for b in look:
        assert np.array_equal(got[b], s.ctx.coefficients(meshes[b])), (n, b)
    for b in list(range(0, n, 997)) + look:
        want = lf.coefficients(meshes[b])
        note("coefficients / bound_of", np.abs(got[b] - want).max() / bound_of(want), f"N {N} n {n} item {b}")
        assert np.abs(got[b] - want).max() <= bound_of(want), (n, b)
    th = np.zeros((n, 10 + s.model.rank))
    th[:, 0] = 1.0
    th[:, 1:4] = rng.normal(size=(n, 3))
    th[:, 10:] = 0.5 * rng.normal(size=(n, s.model.rank))
    inst = pkg.transformed_meshes(s.ctx, th)
    for b in look:
        assert np.array_equal(inst[b], s.ctx.transformedMesh(th[b])) and np.array_equal(inst[b], s.om.instance(th[b])), (n, b)
    s.done()


# ---------------------------------------------------------------- (c) posterior models

def pm_pair(pkg, s, K, seed):
    """one observation set under both noise forms, in one call -> (results, ids, y, sigma2, cov)"""
    ids, y, s2, cov = BL.pm_case_inputs(s.model, K, seed)
    res = pkg.posterior_models(s.ctx, [ids] * 2, [y] * 2, sigma2=[s2, None], covariances=[None, cov])
    return res, ids, y, s2, cov


def note_pm(figures, where):
    for k, (err, tol) in figures.items():
        note(f"posterior model {k} / bar", err / tol, where)


@pytest.mark.parametrize("N,r", BL.PM_CASES, ids=[f"N{N}-rank{r}" for N, r in BL.PM_CASES])
def test_posterior_models_over_n(pkg, oracle, N, r):
    """K = min(N, 40) observations, sigma2 and full covariances: alpha, mean, basis, variances and point variances against the long
    form at check_against_long_form's bars; a call for the mean alone (the piece starts at column tile r / 16), for the basis alone
    and for the point variances alone gives the bits of the full call"""
    s = Shape(pkg, oracle, N, r)
    K = BL.pm_K(N)
    res, ids, y, s2, cov = pm_pair(pkg, s, K, BL.PM_SEED[(N, r)])
    note_pm(check_against_long_form(s.model, res[0], ids, y, s2, None, f"N {N} rank {r} K {K} sigma2"), f"N {N} rank {r} sigma2")
    note_pm(check_against_long_form(s.model, res[1], ids, y, None, cov, f"N {N} rank {r} K {K} 3x3"), f"N {N} rank {r} 3x3")
    for want in (("mean",), ("basis",), ("point_variance",), ("alpha", "variance")):
        part = pkg.posterior_models(s.ctx, [ids] * 2, [y] * 2, sigma2=[s2, None], covariances=[None, cov], want=want)
        for k in range(2):
            assert part[k]["status"] == 0 and all(np.array_equal(part[k][w], res[k][w]) for w in want), (N, r, want, k)
    alone = pkg.posterior_models(s.ctx, [ids], [y], covariances=[cov])[0]
    assert same_bits(alone, res[1]), (N, r)
    print(f"N {N} rank {r}: k_pm_gemm rows {BL.pm_gemm_rows(N)}, point-variance waves {BL.pm_point_variance_waves(N)}, mean-only t0 {BL.pm_mean_only_t0(r)}")
    s.done()


@pytest.mark.parametrize("r", BL.RANKS)
def test_posterior_models_over_k(pkg, oracle, r):
    """N = 600, every K of the ladder in one call per noise form (items of 1 to 64 splits side by side, empty leaves included):
    against the long form, and every item the bits of the item alone"""
    s = Shape(pkg, oracle, 600, r)
    sets = [BL.pm_case_inputs(s.model, K, BL.PM_K_SEED[(r, K)]) for K in BL.K_LADDER]
    for form in ("sigma2", "3x3"):
        s2 = [x[2] if form == "sigma2" else None for x in sets]
        cov = [None if form == "sigma2" else x[3] for x in sets]
        res = pkg.posterior_models(s.ctx, [x[0] for x in sets], [x[1] for x in sets], sigma2=s2, covariances=cov)
        for k, K in enumerate(BL.K_LADDER):
            tag = f"rank {r} K {K} {form} (splits {CL.regression_splits(K)} x {CL.regression_kchunk(K)}, empty {CL.empty_leaves(K)})"
            note_pm(check_against_long_form(s.model, res[k], sets[k][0], sets[k][1], s2[k], cov[k], tag), tag)
            alone = pkg.posterior_models(s.ctx, [sets[k][0]], [sets[k][1]], sigma2=[s2[k]], covariances=[cov[k]])[0]
            assert same_bits(alone, res[k]), tag
    s.done()


def pm_items(ctxs, specs):
    """batched_count_ladder's item lists on contexts of their models -> [(ctx, ids, y, sigma2, cov)]"""
    return [(ctxs[i], ids, y, s2, cov) for i, ids, y, s2, cov in specs]


def run_pm(pkg, items):
    return pkg.posterior_models([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], sigma2=[i[3] for i in items],
                                covariances=[i[4] for i in items], want=WANT)


def test_posterior_models_over_items(pkg, oracle):
    """16, 17 and 33 items of one small model (N = 7): from the 17th on an item works in r-space slots an earlier one has used
    (`q % slots`: Mpart, M, V, Bm, work) and its decomposition's record lies behind the first group's.  Every item is the item
    alone; items 16 and 32 carry item 0's observations and give item 0's bits; every item of the call of 33 meets the long form"""
    s = Shape(pkg, oracle, BL.ITEMS_N)
    models, specs = BL.items_of_one_model(pkg)
    assert np.array_equal(models[0].basis, s.model.basis)
    items = pm_items([s.ctx], specs)
    alone = [run_pm(pkg, [it])[0] for it in items]
    for n in (16, 17, 33):
        got = run_pm(pkg, items[:n])
        for k in range(n):
            assert got[k]["status"] == 0 and same_bits(got[k], alone[k]), (n, k)
        if n > 16:
            assert same_bits(got[16], got[0])
        if n > 32:
            assert same_bits(got[32], got[0])
            for k, (c, ids, y, s2, cov) in enumerate(items):
                note_pm(check_against_long_form(s.model, got[k], ids, y, s2, cov, f"33 items, item {k}"), f"33 items, item {k}")
    s.done()


def test_posterior_models_of_three_ranks_shuffled(pkg, oracle):
    """17 items over models of ranks 12, 15 and 40 in a shuffled order: the slots are sized for the largest rank of the call and the
    second group's single item takes over slot 0; every item is the item alone and meets the long form"""
    shapes = [Shape(pkg, oracle, N, r) for N, r in BL.THREE_RANKS]
    models, specs = BL.items_of_three_ranks(pkg)
    assert all(np.array_equal(m.basis, x.model.basis) for m, x in zip(models, shapes))
    items = pm_items([x.ctx for x in shapes], specs)
    assert {it[0].rank for it in items} == {12, 15, 40}
    got = run_pm(pkg, items)
    for k, it in enumerate(items):
        assert got[k]["status"] == 0 and same_bits(got[k], run_pm(pkg, [it])[0]), k
        c, ids, y, s2, cov = it
        note_pm(check_against_long_form(c.model, got[k], ids, y, s2, cov, f"three ranks, item {k} rank {c.rank}"), f"three ranks, item {k}")
    for x in shapes:
        x.done()


def test_indefinite_covariance_in_the_second_group(pkg, oracle):
    """17 items, the 17th with an indefinite covariance: it alone is NaN with status −3; the sixteen before it keep the bits of the
    call without it — then the same with a good 18th item behind it, which takes the slot the live items' count gives it"""
    s = Shape(pkg, oracle, 7)
    items = pm_items([s.ctx], BL.pm_item_list([s.model], 18, 1100))
    c, ids, y, _, _ = items[16]
    bad_cov = BL.spd_blocks(ids.shape[0], 3)
    bad_cov[1] = np.diag([1.0, -1.0, 1.0])
    clean_run = run_pm(pkg, items[:16] + items[17:])
    for n in (17, 18):
        withbad = items[:16] + [(c, ids, y, None, bad_cov)] + items[17:n]
        got = run_pm(pkg, withbad)
        assert got[16]["status"] == -3 and all(np.isnan(got[16][w]).all() for w in WANT)
        for k in range(16):
            assert got[k]["status"] == 0 and same_bits(got[k], clean_run[k]), (n, k)
        if n == 18:
            assert got[17]["status"] == 0 and same_bits(got[17], clean_run[16])
    s.done()


# ---------------------------------------------------------------- (d) variability

def has_normals(N):
    """mode 1 and 2 need every vertex in a triangle with an area: the one-triangle mesh and the closed meshes"""
    return N == 3 or N >= 9


VAR_NS = [(N, None) for N in BL.SMALL_N] + [(BL.RANK40_N["variability"], BL.RANKS[1])]


def check_maps(pkg, oracle, s, sets, modes, refs, tag, with_oracle=True):
    got = pkg.posterior_variability_maps(s.ctx, sets, mode=modes, theta_refs=refs)
    for th, mode, ref, g in zip(sets, modes, refs, got):
        assert g.shape == (s.N,) and np.array_equal(g, one_map(pkg, s.ctx, th, mode, ref)), (tag, mode, th.shape[0])
        if with_oracle:
            want = oracle.posterior_variability(s.om, th, mode=mode, theta_ref=ref)
            scale = np.abs(want).max()
            err = np.abs(g - want).max()
            note("variability / oracle bar", err / (VAR_REL * scale) if scale > 0 else 0.0, f"{tag} mode {mode} S {th.shape[0]}")
            assert err <= VAR_REL * scale, (tag, mode, th.shape[0], err, scale)
    return got


@pytest.mark.parametrize("N,r", VAR_NS, ids=[f"N{N}" + (f"-rank{r}" if r else "") for N, r in VAR_NS])
def test_variability_over_n(pkg, oracle, N, r):
    """S = 9 samples (a full group and a group of one), every mode the mesh allows, in one call with the same set first and last:
    the one-map entry's bits, the oracle within its bar"""
    s = Shape(pkg, oracle, N, r)
    th = BL.states(s.model, 4000 + N, 9)
    modes = [0, 1, 2, 0] if has_normals(N) else [0, 0]
    refs = [th[1] if m == 1 else None for m in modes]
    got = check_maps(pkg, oracle, s, [th] * len(modes), modes, refs, f"N {N}")
    assert np.array_equal(got[0], got[-1])
    s.done()


def test_variability_over_s(pkg, oracle):
    """S = 2, 3, 7, 8, 9 at N = 65, all modes, all in one call (15 maps of one round)"""
    s = Shape(pkg, oracle, 65)
    small = [S for S in BL.S_LADDER if S < 100]
    sets = [BL.states(s.model, 5000 + 10 * S, S) for S in small for _ in range(3)]
    modes = [0, 1, 2] * len(small)
    check_maps(pkg, oracle, s, sets, modes, [t[0] if m == 1 else None for t, m in zip(sets, modes)], "N 65")
    s.done()


BIG_S = [S for S in BL.S_LADDER if S > 100]


@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("S", BIG_S)
def test_variability_at_the_rounds_sample_cap(pkg, oracle, S, r):
    """the one-triangle mesh: S = 32,767 is whole, 32,768 takes the two-sweep route in one segment (mode 1: two, its reference mesh
    holds a place of the round), 32,769 two segments with first / last apart.  Every mode: the one-map entry's bits; modes 0 and 1
    also the bits of a float64 numpy restatement of the two loops in sample order over the samples' icp_transformed_mesh rows"""
    s = Shape(pkg, oracle, 3, r)
    rng = np.random.default_rng(S + r)
    th = np.zeros((S, 10 + r))
    th[:, 0] = 1.0
    th[:, 1:4] = rng.normal(size=(S, 3))
    th[:, 4:7] = 0.02 * rng.normal(size=(S, 3))
    th[:, 7:10] = s.model.ref_points.mean(axis=0)
    th[:, 10:] = 0.5 * rng.normal(size=(S, r))
    print(f"S {S}: plan {[BL.var_plan(S, m) for m in (0, 1, 2)]}")
    got = check_maps(pkg, oracle, s, [th] * 3, [0, 1, 2], [th[5], th[5], None], f"N 3 rank {r}", with_oracle=False)
    x = pkg.transformed_meshes(s.ctx, th)
    for b in (0, 1, S // 2, S - 2, S - 1):
        assert np.array_equal(x[b], s.ctx.transformedMesh(th[b])), b
    assert np.array_equal(got[0], BL.variability_restatement(x, 0)), (S, r)
    assert np.array_equal(got[1], BL.variability_restatement(x, 1, s.ctx.vertexNormals(th[5]))), (S, r)
    assert np.all(got[2] >= 0) and np.all(np.isfinite(got[2]))
    s.done()


# ---------------------------------------------------------------- (e) metrics

def metrics_reference(oracle, s, theta):
    """-> (d² model -> target, d² target -> model, kept flags or None) from the oracle's searches"""
    x = s.om.instance(theta)
    tp = np.ascontiguousarray(s.target.points, dtype=np.float64)
    cp, _, d2 = oracle.closest_point_on_surface(x, tp, s.target.cells)
    _, _, d2t = oracle.closest_point_on_surface(tp, x, s.model.cells)
    flags = oracle.OracleMesh(tp, s.target.cells).boundary()
    keep = None
    if np.any(flags != 0):
        idx, _ = oracle.nearest_vertex(cp, tp)
        keep = flags[idx] == 0
    return d2, d2t, keep


def check_average(got, terms, check, where):
    """an average: Σ within sum_bound of fsum, then ONE division, correctly rounded: 2⁻⁵³ of the quotient more"""
    D = terms.shape[0]
    exact = math.fsum(terms.tolist()) / D
    bound = BL.sum_bound(terms) / D + 2.0 ** -53 * abs(exact)
    err = abs(got - exact)
    note(check, err / bound if bound > 0 else 0.0, where)
    assert err <= bound, (where, got, exact, err, bound)


def check_metrics(pkg, oracle, s, thetas, tag, big):
    m = pkg.registration_metrics(s.ctx, thetas, dice_samples=0)
    assert not m["status"].any()
    trees(oracle, big)
    try:
        for b, th in enumerate(thetas):
            assert np.array_equal(five(m, b), one_metrics(pkg, s.ctx, th), equal_nan=True), (tag, b)
            d2, d2t, keep = metrics_reference(oracle, s, th)
            dm, dt = np.sqrt(d2), np.sqrt(d2t)
            check_average(m["avg"][b], dm, "metrics avg / sum bound", f"{tag} item {b}")
            assert m["hausdorff"][b] == max(dm.max(), dt.max()), (tag, b)
            kept = dm if keep is None else dm[keep]
            assert m["kept"][b] == kept.shape[0], (tag, b, m["kept"][b], kept.shape[0])
            if kept.shape[0] > 0:
                check_average(m["average2surface_boundary_aware"][b], kept, "metrics boundary-aware avg / sum bound", f"{tag} item {b}")
                assert m["max_boundary_aware"][b] == kept.max(), (tag, b)
    finally:
        trees(oracle, False)
    return m


STATS_SIDES = [(N, V, closed) for N in (4096, 4097) for V in (4096, 4097) for closed in (True, False)]


def target_mesh_of(V, closed):
    return CL.closed_mesh(V, 41.0, 15.5) if closed and V >= 9 else BL.ladder_mesh(V, closed=False) if V >= 4 else BL.ladder_mesh(V)


@pytest.mark.parametrize("N,V,closed", STATS_SIDES, ids=[f"N{N}-V{V}-{'closed' if c else 'open'}" for N, V, c in STATS_SIDES])
def test_metrics_on_both_sides_of_the_reductions_switch(pkg, oracle, N, V, closed):
    """model and target vertices on both sides of 4,096 (k_met_stats<256 | 1024>, the model's and the target's list each by its own
    count), a closed target and one with a rim, four states (two sums of another order agree in every bit about every other time):
    the five slots are icp_mesh_metrics' bits, the sums within the order-free bound of fsum over the oracle's distances, maxima and
    the kept count exact"""
    s = Shape(pkg, oracle, N, target_mesh=target_mesh_of(V, closed))
    m = check_metrics(pkg, oracle, s, BL.states(s.model, 6000 + N + V, 4), f"N {N} V {V} {'closed' if closed else 'open'}", big=True)
    assert closed == bool(np.all(m["kept"] == N))
    if not closed:
        assert np.all(m["kept"] > 0) and np.all(m["kept"] < N)
    s.done()


@pytest.mark.parametrize("count,n", [("T", 2047), ("T", 2048), ("V", 2047), ("V", 2048)], ids=lambda v: str(v))
def test_metrics_at_the_hint_stride_edge(pkg, oracle, count, n):
    """the hint of a search is the nearest of every max(1, n / 1024)-th element: stride 1 at 2,047 searched triangles or vertices,
    2 at 2,048 — the mesh is model and target (open: the nearest-vertex search runs too)"""
    mesh = CL.cut_mesh(T=n) if count == "T" else CL.cut_mesh(V=n)
    s = Shape(pkg, oracle, mesh[0].shape[0], seed=47, mesh=mesh)
    assert (mesh[1].shape[0] if count == "T" else mesh[0].shape[0]) == n
    print(f"{count} = {n}: T {mesh[1].shape[0]} stride {BL.hint_step(mesh[1].shape[0])}, V {mesh[0].shape[0]} stride {BL.hint_step(mesh[0].shape[0])}")
    check_metrics(pkg, oracle, s, BL.states(s.model, 6500 + n, 2), f"{count} {n}", big=True)
    s.done()


@pytest.fixture(scope="module")
def dice_case(pkg, oracle):
    case = BL.DiceCase(pkg, oracle)
    case.ctx = pkg.IcpContext(case.model, case.target, device=0)
    yield case
    clean(case.ctx)
    case.ctx.close()


@pytest.mark.parametrize("S_d", BL.SD_LADDER)
def test_dice_over_the_sample_ladder(pkg, dice_case, S_d):
    """a closed model of 129 vertices against a closed target of 257: the three counts are the CPU restatement's, range by range
    added up (the CPU test shows every range of 32,769 and 65,537 adds to each count), Dice is 2·nAB / (nA + nB)"""
    seed = BL.DICE_SEED.get(S_d, 1024)
    m = pkg.registration_metrics(dice_case.ctx, dice_case.theta[None, :], dice_samples=S_d, seed=seed)
    if S_d == 0:
        assert np.isnan(m["dice"][0]) and np.isnan(m["n_inside_both"][0])
        return
    parts = dice_case.by_range(S_d, seed)
    want = tuple(sum(p[k] for p in parts) for k in (2, 3, 4))
    assert dice_counts_of(m, 0) == want, (S_d, dice_counts_of(m, 0), want)
    assert np.array_equal(m["dice"][0], 2.0 * want[2] / (want[0] + want[1]) if want[0] + want[1] > 0 else np.nan, equal_nan=True)
    assert np.array_equal(five(m, 0), one_metrics(pkg, dice_case.ctx, dice_case.theta))


def test_dice_sample_behind_a_full_range(pkg, dice_case):
    """the same seed at 32,768 and 32,769 samples: the counts differ by the one sample of the second range (s0 = 32,768), which the
    restatement puts inside both meshes"""
    seed = BL.DICE_SEED[32769]
    a = pkg.registration_metrics(dice_case.ctx, dice_case.theta[None, :], dice_samples=32768, seed=seed)
    b = pkg.registration_metrics(dice_case.ctx, dice_case.theta[None, :], dice_samples=32769, seed=seed)
    last = dice_case.by_range(32769, seed)[1]
    assert last[:2] == (32768, 1) and last[2:] == (1, 1, 1)
    assert tuple(y - x for x, y in zip(dice_counts_of(a, 0), dice_counts_of(b, 0))) == last[2:]


@pytest.mark.parametrize("n", [64, 65])
def test_metrics_over_items(pkg, oracle, dice_case, n):
    """64 items are one chunk, the 65th opens a second: every item is icp_mesh_metrics', Dice of 257 samples the restatement's for
    the first and the last item of the call (at n = 64 the first and the last of the one chunk, at 65 the first of each chunk)"""
    th = BL.states(dice_case.model, 7000, n)
    th[0] = dice_case.theta
    th[n - 1] = dice_case.theta
    m = pkg.registration_metrics(dice_case.ctx, th, dice_samples=257, seed=1024)
    assert not m["status"].any()
    for b in range(n):
        assert np.array_equal(five(m, b), one_metrics(pkg, dice_case.ctx, th[b])), (n, b)
    want = tuple(sum(p[k] for p in dice_case.by_range(257, 1024)) for k in (2, 3, 4))
    assert dice_counts_of(m, 0) == want and dice_counts_of(m, n - 1) == want


# ---------------------------------------------------------------- (f) log values

def eval_params(pkg, oracle, s, kind, mode, D):
    if kind == HAUSDORFF:
        return oracle.evaluator_params(oracle.EVAL_HAUSDORFF, 2, p0=1.0)
    tp = pkg.data.decimated_point_subset(s.target, D)
    if kind == INDEPENDENT:
        return oracle.evaluator_params(oracle.EVAL_INDEPENDENT, mode, n_model_ids=min(D, s.N), target_pts=tp, p0=0.0, p1=2.0)
    return oracle.evaluator_params(oracle.EVAL_COLLECTIVE, mode, n_model_ids=min(D, s.N), target_pts=tp, p0=0.1, p1=0.3, p2=1.0)


def check_log_items(pkg, oracle, s, items, theta, tag):
    """items = [(kind, mode, D)] on one context and one state, in ONE call: value, aux and status are the one-at-a-time entry's; the
    value is the oracle's within the existing bar -> the call's result"""
    evs = [make_evaluator(pkg, s.ctx, *it) for it in items]
    got = pkg.log_values(evs, np.stack([theta] * len(items)), return_aux=True)
    for e in evs:
        e.close()
    ot = oracle.OracleMesh(np.ascontiguousarray(s.target.points, dtype=np.float64), s.target.cells)
    for i, it in enumerate(items):
        v, aux, st = one_log_value(pkg, s.ctx, *it, theta)
        assert st == got["status"][i] == 0, (tag, it)
        assert got["value"][i] == v and np.array_equal(got["aux"][i], aux), (tag, it, got["value"][i], v)
        want, rc = oracle.evaluator_log_value(s.om, ot, eval_params(pkg, oracle, s, *it), theta)
        assert rc == 0
        err = abs(v - want) / abs(want)
        note(f"log value / oracle bar, kind {it[0]}", err / LOG_REL[it[0]], f"{tag} {it}")
        assert err <= LOG_REL[it[0]], (tag, it, v, want)
    return got


@pytest.fixture(scope="module")
def log_shapes(pkg, oracle):
    """4,097 model vertices against a closed and an open target of 4,097"""
    out = {c: Shape(pkg, oracle, 4097, target_mesh=target_mesh_of(4097, c)) for c in (True, False)}
    yield out
    for s in out.values():
        s.done()


def test_log_values_over_the_distance_ladder(pkg, oracle, log_shapes):
    """the D ladder as the evaluators' point count, closed target, all in one call: the independent evaluator in both directions
    (eval_gauss at 256 threads), the collective one model -> target and target -> model (eval_stats at 256 | 1024).  The sums —
    aux[0], aux[1] of the independent one, the average of the collective one — within the order-free bound of fsum over the
    oracle's distances, the maximum and the counts exact"""
    s = log_shapes[True]
    items = [(kind, mode, D) for D in BL.D_LADDER for kind, mode in ((INDEPENDENT, 2), (COLLECTIVE, 0), (COLLECTIVE, 1))]
    tp_all = np.ascontiguousarray(s.target.points, dtype=np.float64)
    trees(oracle, True)
    try:
        for theta in BL.states(s.model, 8000, 3):   # (three states: sums of another order agree in every bit about every other time)
            got = check_log_items(pkg, oracle, s, items, theta, "closed")
            x = s.om.instance(theta)
            for i, (kind, mode, D) in enumerate(items):
                d2m = oracle.closest_point_on_surface(x[:D], tp_all, s.target.cells)[2]
                d2t = oracle.closest_point_on_surface(pkg.data.decimated_point_subset(s.target, D), x, s.model.cells)[2]
                aux = got["aux"][i]
                if kind == INDEPENDENT:
                    for side, d2 in ((0, d2m), (1, d2t)):
                        terms = BL.gauss_logpdf_terms(d2, 0.0, 2.0)
                        err, bound = abs(aux[side] - math.fsum(terms.tolist())), BL.gauss_bound(terms)
                        note("Σ log-pdf / bound", err / bound, f"D {D} side {side}")
                        assert err <= bound, (D, side, err, bound)
                else:
                    d = np.sqrt(d2m if mode == 0 else d2t)
                    check_average(aux[0], d, "log values avg / sum bound", f"D {D} mode {mode}")
                    assert aux[1] == d.max() and aux[2 + mode] == D, (D, mode, aux)
    finally:
        trees(oracle, False)


def kept_distances(oracle, s, x, D, mode):
    """the distances the collective evaluator keeps on a target with a boundary, restated from oracle calls (icp_oracle.c, the
    collective branch of the evaluator): mode 0 — model points 0..D−1 against the target's surface, dropped where the nearest target
    vertex of the surface point is a boundary vertex; mode 1 — D target-side points against the instance's surface, dropped where
    the nearest MODEL vertex of the surface point, taken as an index into the TARGET's flags (sic), is flagged"""
    tp = np.ascontiguousarray(s.target.points, dtype=np.float64)
    flags = oracle.OracleMesh(tp, s.target.cells).boundary()
    if mode == 0:
        cp, _, d2 = oracle.closest_point_on_surface(x[:D], tp, s.target.cells)
        idx, _ = oracle.nearest_vertex(cp, tp)
        return np.sqrt(d2[flags[idx] == 0])
    cp, _, d2 = oracle.closest_point_on_surface(s.pkg.data.decimated_point_subset(s.target, D), x, s.model.cells)
    idx, _ = oracle.nearest_vertex(cp, x)
    drop = (idx < tp.shape[0]) & (flags[np.minimum(idx, tp.shape[0] - 1)] != 0)
    return np.sqrt(d2[~drop])


def test_log_values_boundary_aware_across_the_switch(pkg, oracle, log_shapes):
    """the open target: the collective evaluator drops points by their nearest vertex's flag on both sides of 256 and of 4,096
    distances — the one-at-a-time entry's bits and the oracle's value; in the two one-sided modes the boundary-aware average within
    the order-free bound of fsum over the kept distances, the maximum and the kept count exact"""
    s = log_shapes[False]
    items = [(COLLECTIVE, mode, D) for D in (255, 256, 257, 4096, 4097) for mode in (0, 1, 2)]
    theta = BL.state(s.model, 8100)
    trees(oracle, True)
    try:
        got = check_log_items(pkg, oracle, s, items, theta, "open")
        x = s.om.instance(theta)
        for aux, (_, mode, D) in zip(got["aux"], items):
            if mode == 2:
                continue
            kept = kept_distances(oracle, s, x, D, mode)
            assert aux[2 + mode] == kept.shape[0] and kept.shape[0] > 0, (D, mode, aux, kept.shape)
            check_average(aux[0], kept, "log values boundary-aware avg / sum bound", f"open D {D} mode {mode}")
            assert aux[1] == kept.max(), (D, mode, aux)
    finally:
        trees(oracle, False)
    assert any(a[2] < D for a, (_, m, D) in zip(got["aux"], items) if m == 0)   # (points were dropped: the flags were read)


HAUSDORFF_DS = [D for D in BL.D_LADDER if D >= 3]   # (one and two vertices make no triangle with an area)


@pytest.mark.parametrize("D", HAUSDORFF_DS)
def test_hausdorff_over_the_fold_ladder(pkg, oracle, D):
    """the Hausdorff evaluator reduces all N model and all V target distances (eval_max, folds of 1,024): N = V = D; the two maxima
    are exactly the roots of the oracle's largest squared distances"""
    s = Shape(pkg, oracle, D, target_mesh=target_mesh_of(D, True))
    theta = BL.state(s.model, 8200 + D)
    trees(oracle, D > 1000)
    try:
        got = check_log_items(pkg, oracle, s, [(HAUSDORFF, 2, 0)], theta, f"N = V = {D}")
        d2, d2t, _ = metrics_reference(oracle, s, theta)
    finally:
        trees(oracle, False)
    aux = got["aux"][0]
    assert aux[1] == np.sqrt(d2.max()) and aux[2] == np.sqrt(d2t.max()) and aux[0] == max(aux[1], aux[2]), (D, aux)
    print(f"D {D}: eval_max {BL.max_shape(D)}")
    s.done()


@pytest.mark.parametrize("n", [256, 257])
def test_log_values_over_items(pkg, oracle, n):
    """256 items of a 9-vertex model are one chunk, the 257th opens a second; the items' model-side points are one packed query list
    of 9·n queries: every item the one-at-a-time entry's"""
    s = Shape(pkg, oracle, 9, target_mesh=target_mesh_of(9, True))
    th = BL.states(s.model, 8300, n)
    cfgs = [(INDEPENDENT, 2, 9), (COLLECTIVE, 2, 9), (HAUSDORFF, 2, 0)]
    evs = [make_evaluator(pkg, s.ctx, *c) for c in cfgs]
    got = pkg.log_values([evs[b % 3] for b in range(n)], th, return_aux=True)
    for e in evs:
        e.close()
    for b in range(n):
        v, aux, st = one_log_value(pkg, s.ctx, *cfgs[b % 3], th[b])
        assert st == got["status"][b] and got["value"][b] == v and np.array_equal(got["aux"][b], aux), (n, b)
    s.done()


# ---------------------------------------------------------------- (g) registration maps and distance summaries

@pytest.mark.parametrize("K", [255, 256, 257])
def test_maps_over_rows(pkg, oracle, K):
    """N = V = K rows on both sides of kMapBlock, an open target (the flags' round runs): three items, every row the one-item
    route's, the distances the roots of its squared distances"""
    s = Shape(pkg, oracle, K, target_mesh=target_mesh_of(K, False))
    th = BL.states(s.model, 9000 + K, 3)
    got = pkg.registration_maps(s.ctx, th)
    for b in range(3):
        want = one_maps(pkg, s.ctx, s.target, th[b])
        assert got[b]["status"] == 0
        for key in ("m2t_point", "m2t_triangle", "m2t_on_boundary", "t2m_point", "t2m_triangle"):
            assert np.array_equal(got[b][key], want[key]), (K, b, key)
        assert np.array_equal(got[b]["m2t_distance"], np.sqrt(want["m2t_d2"])) and np.array_equal(got[b]["t2m_distance"], np.sqrt(want["t2m_d2"]))
    assert any(m["m2t_on_boundary"].any() for m in got)
    s.done()


@pytest.fixture(scope="module")
def small_maps(pkg, oracle):
    s = Shape(pkg, oracle, 9, target_mesh=target_mesh_of(12, False))
    yield s
    s.done()


@pytest.mark.parametrize("n", [64, 65])
def test_maps_over_items(pkg, small_maps, n):
    """64 items are one chunk, the 65th opens a second: the items on both sides of the boundary, the first and the last are the
    one-item route's; the last item alone gives the same rows"""
    s = small_maps
    th = BL.states(s.model, 9100, n)
    got = pkg.registration_maps(s.ctx, th)
    for b in (0, 1, 62, 63, n - 1):
        want = one_maps(pkg, s.ctx, s.target, th[b])
        for key in ("m2t_point", "m2t_triangle", "m2t_on_boundary", "t2m_point", "t2m_triangle"):
            assert np.array_equal(got[b][key], want[key]), (n, b, key)
        assert np.array_equal(got[b]["m2t_distance"], np.sqrt(want["m2t_d2"])), (n, b)
    alone = pkg.registration_maps(s.ctx, th[n - 1:])
    assert all(np.array_equal(alone[0][k], got[n - 1][k]) for k in MAPS)


def test_summaries_over_the_set_ladder(pkg, small_maps):
    """sets of 1, 2, 3, 64, 65, 128 and 129 samples in one call (392 items, seven chunks: sets that end inside a chunk, that span two
    and — 128 behind an offset, 129 — three, with a middle segment that carries through the other half of the ping-pong buffer):
    every row is the left-to-right numpy fold of registration_maps' distances; each set alone gives the same bits"""
    s = small_maps
    sets = [BL.states(s.model, 9200 + 200 * k, S) for k, S in enumerate(BL.SSUM_LADDER)]
    got = pkg.distance_summaries(s.ctx, sets)
    for m, th in enumerate(sets):
        maps = pkg.registration_maps(s.ctx, th, want=("m2t_distance", "t2m_distance"))
        alone = pkg.distance_summaries(s.ctx, [th])[0]
        assert got[m]["status"] == 0
        for side in ("m2t", "t2m"):
            mean, mx = fold(np.stack([v[side + "_distance"] for v in maps]))
            assert np.array_equal(got[m][side + "_mean"], mean), (th.shape[0], side)
            assert np.array_equal(got[m][side + "_max"], mx), (th.shape[0], side)
            assert np.array_equal(alone[side + "_mean"], mean) and np.array_equal(alone[side + "_max"], mx), (th.shape[0], side)
    print("segments alone:", {S: BL.summary_segments(S) for S in BL.SSUM_LADDER if S > 3})


# ---------------------------------------------------------------- (h) the test-hooks build

def _hooks_check():
    """(run as a program with the test-hooks library loaded) coefficients and projections at N = 7 with a chunk buffer of ONE mesh,
    posterior models at N = 17 and 33 with a chunk buffer that makes every piece exactly kPmRowQuantum = 48 rows (51 rows: 48 + 3;
    99: 48 + 48 + 3): the bits of the default buffers"""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    for k in ("ICP_TEST_PROJECTION_CHUNK_DOUBLES", "ICP_TEST_POSTERIOR_MODELS_CHUNK_DOUBLES"):
        os.environ.pop(k, None)
    s = Shape(pkg, None, 7)
    rng = np.random.default_rng(1)
    th = BL.states(s.model, 100, 17)
    meshes = [m + rng.normal(size=m.shape) for m in pkg.transformed_meshes(s.ctx, th)]
    want = pkg.model_coefficients(s.ctx, meshes=meshes, want_project=True)
    want_t = pkg.model_coefficients(s.ctx, thetas=list(th), poses=[t[:10] for t in th], want_project=True)
    os.environ["ICP_TEST_PROJECTION_CHUNK_DOUBLES"] = str(3 * 7)
    got = pkg.model_coefficients(s.ctx, meshes=meshes, want_project=True)
    got_t = pkg.model_coefficients(s.ctx, thetas=list(th), poses=[t[:10] for t in th], want_project=True)
    assert all(np.array_equal(a, b) for a, b in zip(want + want_t, got + got_t))
    os.environ.pop("ICP_TEST_PROJECTION_CHUNK_DOUBLES")
    s.done()
    for N in (17, 33):
        s = Shape(pkg, None, N)
        items = pm_items([s.ctx], BL.pm_item_list([s.model], 3, 1300 + N, K_of=lambda m: m.n_points))
        want = run_pm(pkg, items)
        r = s.model.rank
        per_q = BL.K_PM_ROW_QUANTUM * (r + 1) + BL.K_PM_ROW_QUANTUM // 3
        cap = BL.K_PM_ROW_QUANTUM * (r + 2)          # what the library raises a smaller buffer to: one quantum fits, two do not
        assert per_q <= cap < 2 * per_q
        os.environ["ICP_TEST_POSTERIOR_MODELS_CHUNK_DOUBLES"] = str(cap)
        got = run_pm(pkg, items)
        os.environ.pop("ICP_TEST_POSTERIOR_MODELS_CHUNK_DOUBLES")
        assert all(a["status"] == 0 and same_bits(a, b) for a, b in zip(want, got)), N
        s.done()
    print("batched counts hooks check ok")


def test_forced_chunks_of_one_mesh_and_pieces_of_one_quantum():
    """Test-hooks build, one child process: a projection chunk of one mesh and posterior-model pieces of exactly 48 rows give the bits
    of the default buffers"""
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=300,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "batched counts hooks check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


if __name__ == "__main__":
    _hooks_check()
