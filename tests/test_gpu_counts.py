"""GPU: the searches, the posterior's regression and the merged step at the COUNTS where the library takes another path
(tests/count_ladder.py: K, T, V and N ladders and the pairs, derived from the restated dispatch and pinned by
tests/test_count_ladder_cpu.py, which also shows the oracle sound on every designed input) — through the C ABI, against the oracle.

(a) the four per-method searches without hints over the T and V ladders (one context a shape, the same mesh as model and as target),
    over the K ladder, and at the pairs: the shrinking stride, the second batch, the vertex filter's second LDS tile;
(b) the same queries on a fresh context and behind the largest call: the same bits and the same counts;
(c) finite bounds: proposals' posteriors and evaluators' log values over sequences of states on curved, tied, degenerate, far and
    scaled scenes, every K of the ladder up to 513, both directions;
(d) M and α over the regression's K, two ranks, against the oracle and the numpy long form;
(e) the merged step against the separate calls over N and over K = K_t, chains against the oracle's, the on-device loop;
(f) meshes of one vertex, two vertices and one triangle.

No bar is this module's own: indices, points and d² are array_equal; M, α and log values take REL = 1e-9 of tests/test_gpu_parity.py;
the merged step is check_merged_step of tests/test_gpu_small_ranks.py, the chains the 1e-5 / 1e-6 of tests/test_gpu_chain.py.

Two things the per-method entry points do not reach, by the code: closestPointOnModel makes the model's spheres first
(ensure_model_spheres) and searches in the resident-sphere form like closestPointOnTarget — the form that makes spheres inside the
filter belongs to the merged step's reverse direction, which (e) runs with a symmetric evaluator against the oracle's chain; and
without a hint `count.surface_exact_tests` is K·T whether the lists overflowed or not (count_ladder's docstring), so at T = 4096 | 4097
the witness shows that every triangle was looked at on both sides, not which route looked."""
import contextlib
import types

import numpy as np
import pytest

import count_ladder as CL
from conftest import make_theta, oracle_chains_parallel
from test_gpu_chain import oracle_chain_config
from test_gpu_parity import REL, rel_err
from test_gpu_small_ranks import check_merged_step

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
        print(f"worst over the count ladders: {check} {WORST[check][0]:.2e} at {WORST[check][1]}")


@contextlib.contextmanager
def trees(oracle):
    """the oracle's KD-tree / BVH back end for the large K (bit-identical to the scans: tests/test_oracle.py,
    tests/test_count_ladder_cpu.py)"""
    oracle.set_search_backend(oracle.SEARCH_TREES)
    try:
        yield
    finally:
        oracle.set_search_backend(oracle.SEARCH_BRUTE)


def clean(ctx):
    assert all(v == 0 for v in ctx.runtime_stats().values()), ctx.runtime_stats()


def counts(ctx, fn):
    """-> (fn(), {counter: executed tests}) with the searches' counters on"""
    ctx.profile_start(count_searches=True)
    try:
        out = fn()
    finally:
        stats = ctx.profile_stop()
    return out, {k[len("count."):]: v["calls"] for k, v in stats.items() if k.startswith("count.")}


class Shape:
    """one mesh, as a model of rank 3 and as the target of the same context"""

    def __init__(self, pkg, oracle, mesh, seed=5, translation=None):
        self.pkg, self.oracle, self.mesh = pkg, oracle, mesh
        V = mesh[0].shape[0]
        self.model, self.target = CL.model_on(pkg, mesh, min(3, 3 * V), seed), CL.as_target(pkg, mesh)
        self.V, self.T = V, mesh[1].shape[0]
        self.ctx = pkg.IcpContext(self.model, self.target, device=0)
        self.om = oracle.OracleModel.from_model(self.model)
        self.theta = np.zeros(10 + self.model.rank)
        self.theta[0], self.theta[1:4] = 1.0, (1.5, -2.0, 0.5)
        self.theta[10:] = 0.3 * np.random.default_rng(seed).normal(size=self.model.rank)
        if translation is not None:   # a pure translation of the reference: exact on integer coordinates
            self.theta[1:4], self.theta[10:] = translation, 0.0
        self.x = self.om.instance(self.theta)

    def close(self):
        self.ctx.close()


def same_surface(got, want, tag):
    (cp, tri, d2), (ocp, otri, od2) = got, want
    assert np.array_equal(tri, otri), tag
    assert np.array_equal(d2, od2), tag
    won = otri >= 0                       # (a query no triangle answers — every distance NaN — has index −1 and d² = +inf on both sides)
    assert np.array_equal(cp[won], ocp[won]), tag


def same_vertex(got, want, tag):
    assert np.array_equal(got[0], want[0]), tag
    assert np.array_equal(got[1], want[1]), tag


def check_searches(s, q, tag, surface=True, vertex=True, model_side=True):
    """the four per-method searches of the queries q against the oracle's scans of the same meshes"""
    o, ctx, (pts, cells) = s.oracle, s.ctx, s.mesh
    if model_side:
        assert np.array_equal(ctx.transformedMesh(s.theta), s.x), tag   # the mesh the model-side references are taken on
    if surface:
        same_surface(ctx.closestPointOnTarget(q), o.closest_point_on_surface(q, pts, cells), tag + " closestPointOnTarget")
        if model_side:
            same_surface(ctx.closestPointOnModel(s.theta, q), o.closest_point_on_surface(q, s.x, cells), tag + " closestPointOnModel")
    if vertex:
        same_vertex(ctx.closestTargetVertex(q), o.nearest_vertex(q, pts), tag + " closestTargetVertex")
        if model_side:
            same_vertex(ctx.closestModelVertex(s.theta, q), o.nearest_vertex(q, s.x), tag + " closestModelVertex")


# ---------------------------------------------------------------- (a) without hints, (f) degenerate counts

SHAPES = [("T", T) for T in CL.T_LADDER] + [("V", V) for V in CL.V_LADDER]


@pytest.mark.parametrize("count,n", SHAPES, ids=[f"{c}{n}" for c, n in SHAPES])
def test_unhinted_searches_over_the_element_ladders(pkg, oracle, count, n):
    """every T and V of the ladders (N = V: the same mesh is the model), 37 and 5 queries; the witness: every query looked at every
    element, on both sides of 4096 | 4097 as well (which of the two routes looked the counter cannot say: the plan printed beside it is
    DISPATCH's, not the device's) — the meshes of one and two vertices and of one triangle are (f)"""
    s = Shape(pkg, oracle, CL.ladder_mesh(count, n))
    assert (s.T if count == "T" else s.V) == n
    tag = f"{count}={n} (V {s.V}, T {s.T})"
    with trees(oracle) if n > 1000 else contextlib.nullcontext():
        check_searches(s, CL.random_queries(s.mesh, 37, 100 + n), tag)
        q5 = CL.random_queries(s.mesh, 5, 200 + n)
        want_s, want_v = oracle.closest_point_on_surface(q5, *s.mesh), oracle.nearest_vertex(q5, s.mesh[0])
    got, c = counts(s.ctx, lambda: (s.ctx.closestPointOnTarget(q5), s.ctx.closestTargetVertex(q5)))
    same_surface(got[0], want_s, tag)
    same_vertex(got[1], want_v, tag)
    plan_t, plan_v = CL.search_plan(5, s.T), CL.search_plan(5, s.V)
    print(tag, "plan", plan_t, plan_v, "counts", c)
    assert c["surface_exact_tests"] == 5 * s.T and c["vertex_exact_tests"] == 5 * s.V, (tag, c)
    clean(s.ctx)
    s.close()


def test_posterior_on_a_model_and_a_target_of_one_triangle(pkg, oracle):
    """(f): every vertex is on the boundary, every correspondence dropped — M = I, α = 0, and the correspondences the oracle's"""
    s = Shape(pkg, oracle, CL.cut_mesh(T=1))
    ot = oracle.OracleMesh(*s.mesh)
    for direction in CL.DIRECTIONS:
        tp = s.mesh[0] + 0.25
        prop = pkg.NonRigidIcpProposal(s.ctx, CL.STEP, CL.SIGMA_T, CL.SIGMA_N, 3, direction, True, decimatedTargetPoints=tp)
        pp = (oracle.proposal_params(CL.STEP, CL.SIGMA_T, CL.SIGMA_N, oracle.MODEL_SAMPLING, True, n_model_ids=3) if direction == "ModelSampling"
              else oracle.proposal_params(CL.STEP, CL.SIGMA_T, CL.SIGMA_N, oracle.TARGET_SAMPLING, True, target_pts=tp))
        post, po = prop.icpPosterior(s.theta), oracle.icp_posterior(s.om, ot, pp, s.theta)
        assert np.array_equal(post.corr_id, po.corr_id) and np.array_equal(post.keep, po.keep) and np.array_equal(post.corr_point, po.corr_pt)
        assert not po.keep.any() and np.array_equal(post.M, np.eye(3)) and not post.alpha.any()
        prop.close()
    clean(s.ctx)
    s.close()


TIED_GRIDS = {"listed": (13, 17), "overflowed": (47, 47)}   # 384 triangles: a list; 4,232 > kCandStrideMax: the scan through the spheres


@pytest.mark.parametrize("degenerate", [False, True], ids=["plain", "degenerate"])
@pytest.mark.parametrize("route", list(TIED_GRIDS))
def test_unhinted_searches_on_tied_placements(pkg, oracle, route, degenerate):
    """the tie rule where the winner shows: the four tied placements over the interior vertices of a flat integer grid — six, two and
    two triangles, one, two and four vertices at exactly the same distance — through closestPointOnTarget / closestTargetVertex and,
    the model a pure integer translation of the same grid, closestPointOnModel / closestModelVertex; with the three degenerate
    triangles at the lowest indices the point triangle and the segment's corner join the ties and must win them.  Triangle and vertex
    ids, d² and points are the oracle's (whose winner the CPU test shows to be the lowest index of every tie), on a mesh short enough
    for lists (surface_resolve's first loop) and on one that overflows them (its second)."""
    a, b = TIED_GRIDS[route]
    mesh = CL.with_degenerates(CL.flat_grid(a, b)) if degenerate else CL.flat_grid(a, b)
    t = np.array([2.0, -3.0, 1.0])
    s = Shape(pkg, oracle, mesh, translation=t)
    assert CL.search_plan(8, s.T)[0][2] == (route == "listed")
    assert np.array_equal(s.x, mesh[0] + t)
    step = 1 if route == "listed" else 5
    q = np.concatenate([CL.tied_queries(a, b, o)[::step] for o in CL.TIED.values()])
    if degenerate:   # … and above and on the segment's corner and the point triangle's vertex, whichever vertices the stride took
        own = mesh[0][[mesh[1][0, 0], mesh[1][1, 0]]]
        q = np.concatenate([q, own + np.array([0.0, 0.0, 0.5]), own])
    tri, _, mult, _ = CL.surface_reference(q[:64], mesh)
    assert (mult >= 6).all()                                                     # (the first 64: above a vertex)
    tag = f"tied, {route}, degenerate={degenerate}"
    check_searches(s, q, tag + " target", model_side=False)
    s.mesh = (s.x, mesh[1])                                                      # the same scene, moved: the model's instance
    o, qm = oracle, q + t
    assert np.array_equal(s.ctx.transformedMesh(s.theta), s.x), tag
    same_surface(s.ctx.closestPointOnModel(s.theta, qm), o.closest_point_on_surface(qm, s.x, mesh[1]), tag + " closestPointOnModel")
    same_vertex(s.ctx.closestModelVertex(s.theta, qm), o.nearest_vertex(qm, s.x), tag + " closestModelVertex")
    if degenerate:
        _, won, _ = o.closest_point_on_surface(q, *mesh)
        assert (won == 1).sum() >= 1 and (won == 0).sum() >= 1, tag              # the point triangle and the segment's corner win ties
    clean(s.ctx)
    s.close()


@pytest.fixture(scope="module")
def mid(pkg, oracle):
    s = Shape(pkg, oracle, CL.cut_mesh(T=600))
    yield s
    s.close()


def test_unhinted_searches_over_the_k_ladder(mid):
    for K in CL.K_LADDER:
        check_searches(mid, CL.random_queries(mid.mesh, K, 300 + K), f"K={K}")
    clean(mid.ctx)


@pytest.mark.parametrize("kind,n,K", CL.PAIRS, ids=[f"{k}-{n}-K{K}" for k, n, K in CL.PAIRS])
def test_unhinted_searches_at_the_pairs(pkg, oracle, kind, n, K):
    """the shapes whose edge hangs on two counts: the stride shrinking, the second batch, the vertex filter's second group and tile"""
    s = Shape(pkg, oracle, CL.cut_mesh(T=n) if kind == "surface" else CL.cut_mesh(V=n))
    plan = CL.search_plan(K, s.T if kind == "surface" else s.V)
    print(kind, n, K, "plan", plan, "vertex chunk", CL.vertex_chunk_shape(s.V, K))
    with trees(oracle):
        check_searches(s, CL.random_queries(s.mesh, K, 400 + K % 1000), f"{kind} n={n} K={K}", surface=kind == "surface", vertex=kind == "vertex")
    clean(s.ctx)
    s.close()


# ---------------------------------------------------------------- (b) history

def test_a_grown_scratch_changes_neither_bits_nor_route(pkg, oracle):
    """DISPATCH (stride_after): a call gets the plan of a fresh context whatever came before — 5 queries against 4,097 triangles
    overflow their lists of 4,096 on a fresh context and behind the call of 16,381 queries alike"""
    mesh = CL.cut_mesh(T=4097)
    s = Shape(pkg, oracle, mesh)
    q5, big = CL.random_queries(mesh, 5, 7), CL.random_queries(mesh, 16381, 8)
    assert CL.stride_after(5, 4097, [(16381, 4097)]) == CL.search_plan(5, 4097) == [(5, 4096, False)]
    fresh, c_fresh = counts(s.ctx, lambda: (s.ctx.closestPointOnTarget(q5), s.ctx.closestTargetVertex(q5)))
    s.ctx.closestPointOnTarget(big)
    s.ctx.closestTargetVertex(big)
    later, c_later = counts(s.ctx, lambda: (s.ctx.closestPointOnTarget(q5), s.ctx.closestTargetVertex(q5)))
    for a, b in zip(fresh[0] + fresh[1], later[0] + later[1]):
        assert np.array_equal(a, b)
    assert c_fresh == c_later, (c_fresh, c_later)
    with trees(oracle):
        same_surface(later[0], oracle.closest_point_on_surface(q5, *mesh), "behind the largest call")
    clean(s.ctx)
    s.close()


# ---------------------------------------------------------------- (c) finite bounds

SCENES = CL.hinted_scenes()


class SceneCase:
    def __init__(self, pkg, oracle, scene):
        self.pkg, self.oracle, self.scene = pkg, oracle, scene
        self.model, self.target = scene.model(pkg), CL.as_target(pkg, scene.target_mesh)
        self.om, self.ot = oracle.OracleModel.from_model(self.model), oracle.OracleMesh(*scene.target_mesh)
        self.T, self.V, self.N = self.target.n_cells, self.target.n_points, self.model.n_points

    def context(self):
        return self.pkg.IcpContext(self.model, self.target, device=0)

    def proposal(self, ctx, direction, K):
        """-> (device proposal, oracle parameters)"""
        o, sc = self.oracle, self.scene
        st, sn = sc.noise()
        prop = self.pkg.NonRigidIcpProposal(ctx, CL.STEP, st, sn, K, direction, True, decimatedTargetPoints=sc.tp[:K])
        if direction == "ModelSampling":
            return prop, o.proposal_params(CL.STEP, st, sn, o.MODEL_SAMPLING, True, n_model_ids=K)
        return prop, o.proposal_params(CL.STEP, st, sn, o.TARGET_SAMPLING, True, target_pts=sc.tp[:K])


def check_hinted_posterior(c, prop, pp, theta, tag):
    post, po = prop.icpPosterior(theta), c.oracle.icp_posterior(c.om, c.ot, pp, theta)
    assert np.array_equal(post.corr_id, po.corr_id), tag
    assert np.array_equal(post.keep, po.keep), tag
    assert np.array_equal(post.corr_aux, po.corr_aux), tag
    assert np.array_equal(post.corr_point, po.corr_pt), tag
    eM, ea = note("M, hinted", rel_err(post.M, po.M), tag), note("alpha, hinted", rel_err(post.alpha, po.alpha), tag)
    assert eM < REL and ea < REL, (tag, eM, ea)
    return po


@pytest.mark.parametrize("name", [n for n in SCENES if n != "tied"])
def test_hinted_posteriors_over_the_k_ladder(pkg, oracle, name):
    """every K of the ladder up to 513, both directions, four states each on ONE context: the second state on searches from the
    winners of the one before (the surface hints are the context's, the vertex hints the proposal's); every (K, state) has a θ of
    its own — memoisation is by exact θ.  The witness, at K = 513 on every scene: the searches of states 1.. execute
    less than a quarter of K·T exact triangle tests and K·V (K·N) vertex tests — a bounded search lists what lies within the distance to
    the previous winner, a few dozen elements of the 1,740 and 930 (600); at 2²⁶ the
    triangle tests are asserted strictly below K·T instead (see below).  A posterior shows a correspondence's point, not the triangle that
    won it: of a surface tie under a finite bound these cases see that the point is right, not that the lowest index won."""
    c = SceneCase(pkg, oracle, SCENES[name])
    ctx = c.context()
    # the slack of the f32 tests, 3·2⁻²³ of |x| + |y| + |z|, is 0.007 mm at 2¹³, 0.84 mm at 2²⁰ and 54 mm — five cells — at 2²⁶: there the
    # surface lists are long, but still lists (strictly below K·T); the vertex filter's exact test is f64 and keeps the quarter
    quarter_surface = np.abs(c.scene.shift).max() < 2.0 ** 25
    for direction in CL.DIRECTIONS:
        for K in CL.HINTED_KS:
            prop, pp = c.proposal(ctx, direction, K)
            n_states = len(c.scene.states_of(direction))
            total = {}
            for s in range(n_states):
                theta = c.scene.theta(s, bump=K / 1024.0, direction=direction)
                tag = f"{c.scene.name} {direction} K={K} state {s}"
                if K == 513 and s >= 1:
                    _, got = counts(ctx, lambda: check_hinted_posterior(c, prop, pp, theta, tag))
                    for k, v in got.items():
                        total[k] = total.get(k, 0) + v
                else:
                    check_hinted_posterior(c, prop, pp, theta, tag)
            if K == 513:
                print(f"{c.scene.name} {direction} K=513, states 1..{n_states - 1}: {total}; K·T {K * c.T}, K·V {K * c.V}, K·N {K * c.N} a state")
                if direction == "ModelSampling":
                    assert 0 < total["surface_exact_tests"] < (n_states - 1) * K * c.T // (4 if quarter_surface else 1), total
                    assert 0 < total["vertex_exact_tests"] < (n_states - 1) * K * c.V // 4, total
                else:
                    assert 0 < total["vertex_exact_tests"] < (n_states - 1) * K * c.N // 4, total
            prop.close()
    clean(ctx)
    ctx.close()


@pytest.mark.parametrize("direction", CL.DIRECTIONS)
def test_hinted_posteriors_on_tied_placements(pkg, oracle, direction):
    """the flat grids: one winner, then six triangles (four vertices) tied with the hint the highest-indexed of them — the others
    must pass the filter at their bound exactly and the lowest must win: seen through corr_id for the vertices; for the triangles a
    posterior shows only the point, which the tied triangles share, so the surface tie rule under a finite bound is NOT covered here
    (test_unhinted_searches_on_tied_placements covers it without a bound) —, then the other tied placements; a context of its own per
    direction and K, every model vertex (every cell centre) and 64 of them"""
    c = SceneCase(pkg, oracle, SCENES["tied"])
    for K in ((c.N, 64) if direction == "ModelSampling" else (c.scene.tp.shape[0], 64)):
        ctx = c.context()
        prop, pp = c.proposal(ctx, direction, K)
        for s in range(len(c.scene.states_of(direction))):
            theta = c.scene.theta(s, direction=direction)
            tag = f"tied {direction} K={K} state {s}"
            if s == 1:
                po, got = counts(ctx, lambda: check_hinted_posterior(c, prop, pp, theta, tag))
                print(tag, got, "K·T", K * c.T, "K·N", K * c.N)
                if direction == "ModelSampling":
                    assert 0 < got["surface_exact_tests"] < K * c.T // 4, got
                else:
                    assert 0 < got["vertex_exact_tests"] < K * c.N // 4, got
            else:
                po = check_hinted_posterior(c, prop, pp, theta, tag)
            assert po.keep.sum() >= K // 4, tag
        prop.close()
        clean(ctx)
        ctx.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_hinted_log_values(pkg, oracle, name):
    """evaluators in both directions over the scenes' states, K = 65 and 257: the log value to 1e-9"""
    c = SceneCase(pkg, oracle, SCENES[name])
    ctx = c.context()
    o, sc = oracle, c.scene
    sigma = 2.0 * sc.scale
    for mode, omode in ((pkg.ModelToTargetEvaluation, o.MODEL_TO_TARGET), (pkg.TargetToModelEvaluation, o.TARGET_TO_MODEL)):
        direction = "ModelSampling" if mode == pkg.ModelToTargetEvaluation else "TargetSampling"
        for K in (65, 257):
            K = min(K, sc.tp.shape[0], c.N)
            tp = sc.tp[:K]
            ev = pkg.IndependentPointDistanceEvaluator(ctx, 0.0, sigma, mode, K, decimatedTargetPoints=tp, numDecimatedModelPoints=K)
            ep = o.evaluator_params(o.EVAL_INDEPENDENT, omode, n_model_ids=K, target_pts=tp, p0=0.0, p1=sigma)
            for s in range(len(sc.states_of(direction))):
                theta = sc.theta(s, bump=0.0 if sc.flat else (K + 2048) / 1024.0, direction=direction)
                lv, (lvo, rc) = ev.logValue(theta), o.evaluator_log_value(c.om, c.ot, ep, theta)
                assert rc == 0 and np.isfinite(lvo)
                err = note("log value, hinted", abs(lv - lvo) / abs(lvo), f"{sc.name} mode {mode} K={K} state {s}")
                assert err <= REL, (name, mode, K, s, lv, lvo)
            ev.close()
    clean(ctx)
    ctx.close()


# ---------------------------------------------------------------- (d) regression over K

@pytest.mark.parametrize("r", CL.RANKS)
def test_regression_over_k(pkg, oracle, r):
    """M and α at both sides of every edge of the regression's split (REGRESSION_KS and N = 600), both directions — ModelSampling keeps
    every correspondence, TargetSampling drops the first and last of every other leaf and the last of all (the CPU test shows the oracle
    keeps exactly those) — against the oracle and the numpy long form"""
    case = CL.regression_case(pkg, r)
    model = CL.model_on(pkg, (case.model.ref_points, case.model.cells), r, 11)
    assert np.array_equal(model.basis, case.model.basis)
    ctx = pkg.IcpContext(model, CL.as_target(pkg, case.target_mesh), device=0)
    om, ot = oracle.OracleModel.from_model(case.model), oracle.OracleMesh(*case.target_mesh)
    for K in CL.REGRESSION_KS + (case.model.n_points,):
        theta = case.theta.copy()
        theta[1] += K / 1024.0
        normals = om.vertex_normals(om.instance(theta))
        for direction in CL.DIRECTIONS:
            pp, want_keep, tp = case.params(oracle, direction, K)
            prop = pkg.NonRigidIcpProposal(ctx, CL.STEP, CL.SIGMA_T, CL.SIGMA_N, K, direction, True, decimatedTargetPoints=tp)
            post, po = prop.icpPosterior(theta), oracle.icp_posterior(om, ot, pp, theta)
            tag = f"rank {r} K={K} {direction}"
            assert np.array_equal(post.corr_id, po.corr_id) and np.array_equal(post.keep, po.keep), tag
            assert np.array_equal(post.corr_point, po.corr_pt), tag
            assert po.keep.all() if want_keep is None else np.array_equal(po.keep, want_keep), tag
            M, alpha = CL.regression_long_form(case.model, theta, po.corr_id, po.corr_pt, po.keep, normals)
            fig = {"M": rel_err(post.M, po.M), "alpha": rel_err(post.alpha, po.alpha), "M, long form": rel_err(post.M, M),
                   "alpha, long form": rel_err(post.alpha, alpha)}
            print(tag, f"kept {int(po.keep.sum())}/{K} leaves {CL.regression_splits(K)} × {CL.regression_kchunk(K)}, empty {CL.empty_leaves(K)}",
                  {k: f"{v:.1e}" for k, v in fig.items()})
            for k, v in fig.items():
                note(k, v, tag)
                assert v < REL, (tag, fig)
            prop.close()
    clean(ctx)
    ctx.close()


# ---------------------------------------------------------------- (e) the merged step and launch 1

TARGET_TORUS = dict(N=700, R=41.0, r0=15.5)


def torus_case(pkg, N, r=CL.RANKS[0]):
    """a closed model of N vertices inside a closed target of 700 (the merged step needs a closed target: icp_chain_step_path)"""
    model = CL.model_on(pkg, CL.closed_mesh(N), r, 21)
    target = CL.as_target(pkg, CL.closed_mesh(TARGET_TORUS["N"], TARGET_TORUS["R"], TARGET_TORUS["r0"]))
    return types.SimpleNamespace(pkg=pkg, model=model, target=target, r=r, ctx=pkg.IcpContext(model, target, device=0))


@pytest.mark.parametrize("N", CL.MERGED_NS)
def test_merged_step_over_n(pkg, oracle, N):
    """launch 1's ⌈N / 128⌉ workgroups and the one-per-vertex launches' ⌈N / 256⌉: the instance is the oracle's, six merged steps give
    the bits of the separate calls"""
    c = torus_case(pkg, N)
    om = oracle.OracleModel.from_model(c.model)
    for seed in range(3):
        theta = make_theta(c.model, seed)
        assert np.array_equal(c.ctx.transformedMesh(theta), om.instance(theta)), (N, seed)
    print(f"N={N}: launch 1 grid {CL.step_begin_grid(N, CL.query_kpad(2 * c.r))}")
    check_merged_step(c)
    c.ctx.close()


@pytest.mark.parametrize("K", CL.MERGED_KS)
def test_merged_step_over_k(pkg, K):
    """K = K_t = the evaluator's points on both sides of 256 | 257: the second workgroup of launch 1's vertex part, of the surface
    filter's queries and of the one-per-correspondence launches, and the summing launch (32 splits and more)"""
    c = torus_case(pkg, 600)
    assert CL.regression_splits(K) >= CL.STEP_REDUCE_SPLITS
    print(f"K={K}: launch 1 grid {CL.step_begin_grid(600, CL.query_kpad(K))}, surface chunks {CL.split_surface_queries(CL.query_kpad(K))}")
    check_merged_step(c, Kp=K, Ke=K)
    c.ctx.close()


CHAINS = {"N=129": dict(N=129, K=None, mode=0), "N=600, K=257, symmetric": dict(N=600, K=257, mode=2)}
CHAIN_STEPS = 20


def chain_setup(pkg, model, target, cfg):
    return pkg.femur_icp_proposal_registration(model, target, n_icp_points=cfg["K"], n_eval_points=cfg["K"], eval_mode=cfg["mode"], fused=2)


@pytest.fixture(scope="module")
def oracle_chains(pkg, oracle):
    jobs, keep = [], {}
    for name, cfg in CHAINS.items():
        c = torus_case(pkg, cfg["N"])
        setup = chain_setup(pkg, c.model, c.target, cfg)
        om, ot = oracle.OracleModel.from_model(c.model), oracle.OracleMesh(c.target.points, c.target.cells)
        keep[name] = (c, setup)
        for seed in (1024, 1025):
            jobs.append((om, ot, oracle_chain_config(oracle, setup), pkg.random_initial_parameters(c.model, seed - 1024), seed, CHAIN_STEPS))
    res = oracle_chains_parallel(oracle, jobs)
    out = {name: (keep[name], res[2 * i], res[2 * i + 1]) for i, name in enumerate(CHAINS)}
    yield out
    for (c, _), _, _ in out.values():
        c.ctx.close()


def same_chain(rec, want, tag):
    acc_o, comp_o, logp_o, states_o = want
    assert np.array_equal(rec[:, 1].astype(np.uint8), acc_o), f"{tag}: accept/reject sequences differ"
    assert np.array_equal(rec[:, 2].astype(np.int32), comp_o), f"{tag}: mixture components differ"
    scale = np.abs(states_o[:, 10:]).max()
    assert scale > 0 and acc_o.sum() > 0, tag
    err_s, err_l = np.abs(rec[:, 4 + 10:] - states_o[:, 10:]).max() / scale, np.abs(rec[:, 3] - logp_o).max() / np.abs(logp_o).max()
    print(f"{tag}: accepted {int(acc_o.sum())}/{len(acc_o)}, components {np.bincount(comp_o, minlength=3)}, states {err_s:.2e}, log posterior {err_l:.2e}")
    note("chain states", err_s, tag), note("chain log posterior", err_l, tag)
    assert err_s <= 1e-5 and err_l <= 1e-6, (tag, err_s, err_l)


@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_matches_oracle(pkg, oracle_chains, name):
    """20 steps of the femur study's chain on the tori, every step merged: the oracle's decisions, states within 1e-5, log posterior
    values within 1e-6; the second shape has 257 points on every side and a symmetric evaluator, whose reverse direction searches the
    new instance with spheres made inside the filter"""
    (c, setup), want, _ = oracle_chains[name]
    chain = pkg.SamplingRegistration(c.ctx, setup, pkg.random_initial_parameters(c.model, 0), 1024)
    rec = chain.run(CHAIN_STEPS)
    paths = c.ctx.step_paths()
    same_chain(rec, want, name)
    assert paths == {"merged": CHAIN_STEPS, "wide": 0, "per_stage": 0, "device_loop": 0}, paths
    clean(c.ctx)
    chain.close()


LOOP_CHAINS = 24  # the host takes chains of the merged step at ranks up to 64 into the loop from 24 on (run_on_device, icp_host.cpp)


def test_on_device_loop_matches_oracle(pkg, oracle, oracle_chains):
    """the chain of the first shape, 24 of them from 24 starts, inside icp_chains_run_on_device: every step counted by the loop, every
    decision the oracle's"""
    name = "N=129"
    (c, setup), want0, want1 = oracle_chains[name]
    om, ot = oracle.OracleModel.from_model(c.model), oracle.OracleMesh(c.target.points, c.target.cells)
    theta0 = [pkg.random_initial_parameters(c.model, b) for b in range(LOOP_CHAINS)]
    cfg = oracle_chain_config(oracle, setup)
    want = oracle_chains_parallel(oracle, [(om, ot, cfg, theta0[b], 1024 + b, CHAIN_STEPS) for b in range(LOOP_CHAINS)])
    for a, b in zip(want[0] + want[1], want0 + want1):
        assert np.array_equal(a, b)
    ctxs = [pkg.IcpContext(c.model, c.target, device=0) for _ in range(LOOP_CHAINS)]
    chains = [pkg.SamplingRegistration(ctxs[b], setup, theta0[b], seed=1024 + b) for b in range(LOOP_CHAINS)]
    recs = pkg.run_chains_batched(chains, CHAIN_STEPS)
    assert all(x.step_paths()["device_loop"] == CHAIN_STEPS for x in ctxs), [x.step_paths() for x in ctxs]
    for b in range(LOOP_CHAINS):
        same_chain(recs[b], want[b], f"{name} in the loop, chain {b}")
    for ch in chains:
        ch.close()
    for x in ctxs:
        clean(x)
        x.close()
