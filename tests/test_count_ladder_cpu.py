"""CPU: the count ladders of tests/count_ladder.py hold both sides of every edge of the restated dispatch, its meshes have the counts
they are made from, the oracle's searches are sound on every designed input — against a numpy statement of the same operations that
shares no code with it —, the hinted sequences of tests/test_gpu_counts.py do what that module says they do, and the long form of a
proposal's regression is the oracle's M and α — without a GPU."""
import numpy as np
import pytest

import count_ladder as CL
from test_gpu_parity import REL, rel_err


# ---------------------------------------------------------------- ladders

@pytest.mark.parametrize("count", ["K", "T", "V", "N"])
def test_ladder_holds_both_sides_of_every_edge(count):
    table, ladder = CL.DISPATCH[count], getattr(CL, f"{count}_LADDER")
    assert ladder == tuple(sorted(set(ladder))) and {1, 2, 3} <= set(ladder)
    for name, (fn, lo, hi) in table.items():
        es = CL.edges(fn, lo, hi)
        print(f"{count}: {name}: changes behind {es}")
        assert es, name  # (a decision without an edge does not belong in DISPATCH)
        for c in es:
            assert c in ladder and c + 1 in ladder, (name, c)
    assert ladder == CL.derived_ladder(table)
    assert all(CL.stands_for(c, table) or c in (1, 2, 3) for c in ladder)
    assert ladder[-1] <= 4097  # capped at what the edges need


def test_pairs_hold_both_sides_of_every_edge_on_two_counts():
    got = CL.derived_pairs()
    print(got)
    for name, (kind, n, fn, lo, hi) in CL.PAIR_DISPATCH.items():
        assert CL.edges(fn, lo, hi), name
    assert got == CL.PAIRS
    assert CL.REGRESSION_KS == (1, 7, 8, 9, 16, 17, 248, 249, 511, 512, 513, 567, 568, 576, 577)
    fn, lo, hi = CL.K_DISPATCH["regression_splits, kchunk, empty leaves, kStepReduceSplits"]
    for c in CL.edges(fn, lo, hi):
        assert c in CL.REGRESSION_KS and c + 1 in CL.REGRESSION_KS, c
    assert set(CL.MERGED_NS) >= {c for c in CL.N_LADDER if c >= 127} and set(CL.MERGED_KS) == {255, 256, 257}
    assert set(CL.HINTED_KS) == {K for K in CL.K_LADDER if K <= 520}


def test_restated_dispatch_gives_the_values_the_code_documents():
    assert [CL.query_kpad(K) for K in (1, 4, 5, 1622)] == [4, 4, 8, 1624]
    assert [CL.cand_stride(n) for n in (0, 1, 511, 512, 58000)] == [1, 1, 511, 512, 512]
    # the femur target (3,240 triangles, fewer than kCandStrideMax): a list as long as the mesh, an exact scan in the listed form
    assert CL.search_plan(308, 3240) == [(308, 3240, True)]
    assert CL.search_plan(5, 4096) == [(5, 4096, True)] and CL.search_plan(5, 4097) == [(5, 4096, False)]
    assert CL.search_plan(16380, 4097)[0][1] == 4096 and CL.search_plan(16381, 4097)[0][1] == 4095
    assert CL.search_plan(131068, 520) == [(131068, 512, False)]
    assert CL.search_plan(131069, 520) == [(131068, 512, False), (1, 520, True)]   # "more queries than that are batched"
    assert CL.split_surface_queries(308) == (2, 256)                                  # "two workgroups ... for the 308 queries of the femur step"
    assert CL.split_surface_queries(308, chains=16) == (1, 308)
    assert CL.split_queries(CL.vblocks(1622), CL.query_kpad(1622)) == (136, 12)        # kchunk 12 at V = 1,622: one LDS tile
    assert CL.vertex_chunk_shape(2560, 13184) == (1, 2) and CL.vertex_chunk_shape(2560, 13185) == (2, 2)
    assert CL.vertex_chunk_shape(2560, 6592) == (1, 1) and CL.vertex_chunk_shape(2560, 6593) == (1, 2)
    assert [CL.regression_splits(K) for K in (1, 8, 9, 104, 248, 249, 512, 513, 100000)] == [1, 1, 2, 13, 31, 32, 64, 64, 64]
    assert [CL.regression_kchunk(K) for K in (8, 9, 512, 513, 567, 568, 576, 577)] == [8, 5, 8, 9, 9, 9, 9, 10]
    assert [CL.empty_leaves(K) for K in (512, 513, 567, 568, 576, 577)] == [0, 7, 1, 0, 0, 6]
    assert all(CL.empty_leaves(K) == 0 for K in range(1, 513)) and all(CL.empty_leaves(K) > 0 for K in range(513, 568))
    assert [CL.step_begin_grid(N, 256) for N in (127, 128, 129, 256, 257)] == [2, 2, 3, 3, 4]
    assert CL.step_begin_grid(600, 260) == 5 + 2
    assert [CL.live_waves(T, 128) for T in (1, 128, 129, 512, 513)] == [1, 1, 2, 4, 1]


def test_stride_and_batches_do_not_depend_on_the_contexts_history():
    """the reading of count_ladder's docstring: whatever calls came before, a call gets the plan of a fresh context"""
    shapes = [(K, T) for K in CL.K_LADDER + (5, 37) for T in CL.T_LADDER] + [(K, n) for _, n, K in CL.PAIRS]
    histories = [[(16381, 4097)], [(131069, 520)], [(3, 2)], [(16381, 4097), (131069, 520), (13185, 2560)]]
    for K, n in shapes:
        for h in histories:
            assert CL.stride_after(K, n, h) == CL.search_plan(K, n), (K, n, h)


# ---------------------------------------------------------------- meshes

def check_mesh(mesh, V, T):
    pts, cells = mesh
    assert pts.shape == (V, 3) and cells.shape == (T, 3) and pts.dtype == np.float64 and cells.dtype == np.int32
    assert np.isfinite(pts).all() and (T == 0 or (cells.min() >= 0 and cells.max() < V))


def test_cut_meshes_have_the_counts_they_are_made_from():
    for T in CL.T_LADDER + (520, 600):
        pts, cells = CL.cut_mesh(T=T)
        check_mesh((pts, cells), pts.shape[0], T)
        assert np.unique(cells).shape[0] == pts.shape[0]                      # every vertex used
        assert np.unique(np.sort(cells, axis=1), axis=0).shape[0] == T       # no triangle twice
    for V in CL.V_LADDER + (2560,):
        if V < 3:
            continue
        pts, cells = CL.cut_mesh(V=V)
        check_mesh((pts, cells), V, cells.shape[0])
        assert cells.shape[0] >= 1
        assert np.unique(pts, axis=0).shape[0] == V
    pts, cells = CL.cut_mesh(V=40, T=7)
    check_mesh((pts, cells), 40, 7)
    assert [CL.cut_mesh(T=T)[0].shape[0] for T in (1, 2, 3, 4)] == [3, 4, 5, 6]


def test_torus_meshes_are_closed():
    for N in CL.MERGED_NS + (700,):
        pts, cells = CL.closed_mesh(N)
        check_mesh((pts, cells), N, 2 * N)
        e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]]), axis=1)
        _, counts = np.unique(e, axis=0, return_counts=True)
        assert (counts == 2).all(), N                                        # every edge in exactly two triangles: no boundary
        d = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]])
        assert np.unique(d, axis=0).shape[0] == d.shape[0], N                # every directed edge once: consistently oriented
        assert np.unique(cells).shape[0] == N


# ---------------------------------------------------------------- the oracle's searches against numpy

def same_as_numpy(oracle, q, mesh, tag):
    """-> (triangle, multiplicity): winner and d² bit-equal, closest point bit-equal where a triangle won"""
    cp, tri, d2 = oracle.closest_point_on_surface(q, mesh[0], mesh[1])
    t_np, d_np, mult, cp_np = CL.surface_reference(q, mesh)
    assert np.array_equal(tri, t_np), tag
    assert np.array_equal(d2, d_np), tag
    assert np.array_equal(cp, cp_np), tag
    idx, dv = oracle.nearest_vertex(q, mesh[0])
    i_np, dv_np, vmult = CL.vertex_reference(q, mesh[0])
    assert np.array_equal(idx, i_np) and np.array_equal(dv, dv_np), tag
    return tri, mult, idx, vmult


def test_oracle_is_sound_on_tied_queries(oracle):
    a, b = 9, 9
    mesh = CL.flat_grid(a, b)
    want = {"above a vertex shared by six triangles": (6, 1), "above an edge midpoint": (2, 2),
            "above a cell centre, on the diagonal, equidistant from four vertices": (2, 4), "in the plane, on a vertex": (6, 1)}
    cells = mesh[1]
    for name, offset in CL.TIED.items():
        q = CL.tied_queries(a, b, offset)
        tri, mult, idx, vmult = same_as_numpy(oracle, q, mesh, name)
        print(name, "triangles tied", np.unique(mult), "vertices tied", np.unique(vmult))
        assert (mult == want[name][0]).all() and (vmult == want[name][1]).all(), name
        # the lowest index of the tie wins: of the triangles at the winner's distance none has a smaller index
        pts = mesh[0]
        o = CL.closest_point_triangle_np(q[:, None, :], pts[cells[:, 0]][None], pts[cells[:, 1]][None], pts[cells[:, 2]][None])
        d = ((q[:, None, :] - o) ** 2).sum(axis=2)
        assert np.array_equal(tri, np.array([np.flatnonzero(row == row.min())[0] for row in d]))
    # one winner, and it is the highest-indexed triangle of the six the first placement ties
    q1 = CL.tied_queries(a, b, CL.BEFORE_TIE["triangles"])
    tri1, mult1, _, _ = same_as_numpy(oracle, q1, mesh, "before the tie")
    q = CL.tied_queries(a, b, CL.TIED["above a vertex shared by six triangles"])
    pts = mesh[0]
    o = CL.closest_point_triangle_np(q[:, None, :], pts[cells[:, 0]][None], pts[cells[:, 1]][None], pts[cells[:, 2]][None])
    d = ((q[:, None, :] - o) ** 2).sum(axis=2)
    assert (mult1 == 1).all() and np.array_equal(tri1, np.array([np.flatnonzero(row == row.min())[-1] for row in d]))


def test_oracle_is_sound_on_degenerate_triangles(oracle):
    for flat in (True, False):
        base = CL.flat_grid(9, 9) if flat else CL.curved_grid(9, 9)
        mesh = CL.with_degenerates(base)
        sd = 0.6 if flat else 6.0
        q = np.concatenate([CL.random_queries(base, 160, 3, sd=sd)] + ([CL.tied_queries(9, 9, o) for o in CL.TIED.values()] if flat else []))
        tri, mult, _, _ = same_as_numpy(oracle, q, mesh, f"degenerate flat={flat}")
        n_deg = int((tri < 3).sum())
        print(f"flat={flat}: {q.shape[0]} queries agree with numpy, {n_deg} won by a degenerate triangle, NaN distances "
              f"{int(np.isnan(CL.closest_point_triangle_np(q[:, None, :], *[mesh[0][mesh[1][:3, k]][None] for k in range(3)])).any(axis=2).sum())}")
        assert (tri >= 0).all()
        if flat:
            assert n_deg >= 4   # the point triangle ties the six around its vertex and is listed before them; so does the segment's corner


def test_oracle_winners_do_not_move_with_the_scene(oracle):
    """integer coordinates and integer shifts: the shifted scene is the same scene exactly"""
    mesh = CL.with_degenerates(CL.flat_grid(9, 9))
    q = np.concatenate([CL.tied_queries(9, 9, o) for o in CL.TIED.values()])
    _, tri0, d0 = oracle.closest_point_on_surface(q, mesh[0], mesh[1])
    for sh in CL.FAR_SHIFTS:
        assert np.array_equal(sh, np.round(sh))
        cp, tri, d2 = oracle.closest_point_on_surface(q + sh, mesh[0] + sh, mesh[1])
        assert np.array_equal(tri, tri0) and np.array_equal(d2, d0)
    for sc in CL.SCALES:
        cp, tri, d2 = oracle.closest_point_on_surface(q * sc, mesh[0] * sc, mesh[1])
        assert np.array_equal(tri, tri0) and np.array_equal(d2, d0 * sc * sc)


def test_oracle_is_sound_at_the_ladders_edges(oracle):
    for T in (1, 2, 3, 128, 129, 513):
        mesh = CL.cut_mesh(T=T)
        same_as_numpy(oracle, CL.random_queries(mesh, 37, T), mesh, f"T={T}")
    oracle.set_search_backend(oracle.SEARCH_TREES)
    try:  # the trees the large shapes are answered with give the scans' bits
        mesh = CL.cut_mesh(T=4097)
        q = CL.random_queries(mesh, 300, 5)
        t_np, d_np, _, cp_np = CL.surface_reference(q, mesh)
        cp, tri, d2 = oracle.closest_point_on_surface(q, mesh[0], mesh[1])
        assert np.array_equal(tri, t_np) and np.array_equal(d2, d_np) and np.array_equal(cp, cp_np)
    finally:
        oracle.set_search_backend(oracle.SEARCH_BRUTE)


# ---------------------------------------------------------------- the hinted sequences

def scene_posteriors(pkg, oracle, scene, direction, K, states=None):
    model = scene.model(pkg)
    om, ot = oracle.OracleModel.from_model(model), oracle.OracleMesh(*scene.target_mesh)
    st, sn = scene.noise()
    if direction == "ModelSampling":
        pp = oracle.proposal_params(CL.STEP, st, sn, oracle.MODEL_SAMPLING, True, n_model_ids=K)
    else:
        pp = oracle.proposal_params(CL.STEP, st, sn, oracle.TARGET_SAMPLING, True, target_pts=scene.tp[:K])
    n = len(scene.states_of(direction)) if states is None else states
    return [oracle.icp_posterior(om, ot, pp, scene.theta(s, direction=direction)) for s in range(n)], om, ot


def test_hinted_sequences_change_their_winners(pkg, oracle):
    """curved scenes: between consecutive states a good part of the winners changes (a hint that is the next winner everywhere would
    test nothing), and correspondences are kept"""
    scenes = CL.hinted_scenes()
    for name in ("curved", "degenerate"):
        for direction in CL.DIRECTIONS:
            posts, _, _ = scene_posteriors(pkg, oracle, scenes[name], direction, 513)
            for s in range(1, len(posts)):
                a, b = posts[s - 1], posts[s]
                key = (lambda p: p.corr_aux) if direction == "ModelSampling" else (lambda p: p.corr_id)
                changed = float((key(a) != key(b)).mean())
                moved = float((np.abs(a.corr_pt - b.corr_pt).max(axis=1) > 0).mean()) if direction == "ModelSampling" else changed
                print(f"{name} {direction} state {s}: winners changed {changed:.2f}, points moved {moved:.2f}, kept {int(b.keep.sum())}/513")
                assert moved >= 0.2 and b.keep.sum() >= 100, (name, direction, s)


def test_degenerate_scene_has_degenerate_winners(pkg, oracle):
    """the target of the degenerate scene carries its point triangle and its segment's corner on two spikes: in state 1 model
    vertices have each of them as their closest point, tied with the triangles around it and listed before them — and the segment's NaN
    distances are candidates of the others.  (A posterior does not show the winning triangle; it shows the point, which the tie
    shares.  What this scene asks of the device: the same points with NaN candidates in the lists and a degenerate hint.)"""
    sc = CL.hinted_scenes()["degenerate"]
    om = oracle.OracleModel.from_model(sc.model(pkg))
    pts, cells = sc.target_mesh
    wins = []
    for s in range(len(sc.states)):
        x = om.instance(sc.theta(s))
        tri, d2, mult, cp = CL.surface_reference(x, (pts, cells))
        _, otri, od2 = oracle.closest_point_on_surface(x, pts, cells)
        assert np.array_equal(tri, otri) and np.array_equal(d2, od2)
        won = tri < 2
        o = CL.closest_point_triangle_np(x[:, None, :], *[pts[cells[:1, k]][None] for k in range(3)])
        print(f"state {s}: point triangle wins {int((tri == 1).sum())}, the segment's corner {int((tri == 0).sum())}, ties {np.unique(mult[won])}, "
              f"segment NaN for {int(np.isnan(o).any(axis=2).sum())} of {x.shape[0]}")
        assert (mult[won] >= 2).all() and np.isnan(o).any(), s
        wins.append((int((tri == 0).sum()), int((tri == 1).sum())))
    assert wins[1][0] >= 1 and wins[1][1] >= 1, wins      # state 1: both win, and are the hints state 2 starts from


def test_tied_sequence_puts_the_hint_at_the_highest_index_of_the_tie(pkg, oracle):
    scene = CL.hinted_scenes()["tied"]
    a, b = CL.FLAT
    mesh = scene.target_mesh
    N = a * b
    interior = CL.interior_vertices(a, b)
    # ModelSampling: the surface search of model vertex k under states 0 (one winner) and 1 (six tied)
    model = scene.model(pkg)
    om = oracle.OracleModel.from_model(model)
    x0, x1 = om.instance(scene.theta(0)), om.instance(scene.theta(1))
    assert np.array_equal(x1, mesh[0] + np.array(CL.TIED["above a vertex shared by six triangles"]))   # exact: integer coordinates
    t0, _, m0, _ = CL.surface_reference(x0[interior], mesh)
    pts, cells = mesh
    o = CL.closest_point_triangle_np(x1[interior][:, None, :], pts[cells[:, 0]][None], pts[cells[:, 1]][None], pts[cells[:, 2]][None])
    d = ((x1[interior][:, None, :] - o) ** 2).sum(axis=2)
    ties = [np.flatnonzero(row == row.min()) for row in d]
    assert (m0 == 1).all() and all(len(t) == 6 for t in ties)
    assert np.array_equal(t0, np.array([t[-1] for t in ties]))                # the hint state 1 starts from: the highest of the six
    _, tri1, _ = oracle.closest_point_on_surface(x1[interior], pts, cells)
    assert np.array_equal(tri1, np.array([t[0] for t in ties]))               # and the lowest wins
    # TargetSampling: sample point k against the model's vertices under the vertex states 0 (one winner) and 1 (four tied)
    tp = scene.tp
    for s in (0, 2):
        xa, xb = om.instance(scene.theta(s, direction="TargetSampling")), om.instance(scene.theta(s + 1, direction="TargetSampling"))
        ia, _, ma = CL.vertex_reference(tp, xa)
        dd = ((tp[:, None, :] - xb[None, :, :]) ** 2).sum(axis=2)
        tv = [np.flatnonzero(row == row.min()) for row in dd]
        assert (ma == 1).all() and all(len(t) == 4 for t in tv)
        assert np.array_equal(ia, np.array([t[-1] for t in tv]))
        ib, _ = oracle.nearest_vertex(tp, xb)
        assert np.array_equal(ib, np.array([t[0] for t in tv]))
    assert N == 221 and tp.shape[0] == (a - 1) * (b - 1)


def test_far_and_scaled_scenes_are_the_curved_scene(pkg, oracle):
    """power-of-two scaling is exact: the scaled scenes' correspondences are the curved scene's, their points scaled bit for bit"""
    scenes = CL.hinted_scenes()
    base, _, _ = scene_posteriors(pkg, oracle, scenes["curved"], "ModelSampling", 257, states=2)
    for sc in CL.SCALES:
        got, _, _ = scene_posteriors(pkg, oracle, scenes[f"scaled {sc:g}"], "ModelSampling", 257, states=2)
        for p, g in zip(base, got):
            assert np.array_equal(p.corr_aux, g.corr_aux) and np.array_equal(p.keep, g.keep)
            assert np.array_equal(p.corr_pt * sc, g.corr_pt)
    for e in (13, 20, 26):
        got, _, _ = scene_posteriors(pkg, oracle, scenes[f"far 2^{e}"], "ModelSampling", 257, states=2)
        same = float(np.mean([np.mean(p.corr_aux == g.corr_aux) for p, g in zip(base, got)]))
        print(f"shift 2^{e}: {same:.3f} of the curved scene's nearest target vertices")
        assert same >= 0.9 and all(g.keep.sum() >= 100 for g in got)


# ---------------------------------------------------------------- the regression's long form

@pytest.mark.parametrize("r", CL.RANKS)
@pytest.mark.parametrize("K", [1, 9, 513, 577])
def test_regression_long_form_is_the_oracles(pkg, oracle, r, K):
    case = CL.regression_case(pkg, r)
    om, ot = oracle.OracleModel.from_model(case.model), oracle.OracleMesh(*case.target_mesh)
    normals = om.vertex_normals(om.instance(case.theta))
    for direction in CL.DIRECTIONS:
        pp, want_keep, _ = case.params(oracle, direction, K)
        po = oracle.icp_posterior(om, ot, pp, case.theta)
        if want_keep is not None:
            assert np.array_equal(po.keep, want_keep), (direction, K)        # dropped at the leaf ends, as designed
            assert K == 1 or (po.keep[-1] == 0 and po.keep.sum() >= K // 2)
        else:
            assert po.keep.all()
        M, alpha = CL.regression_long_form(case.model, case.theta, po.corr_id, po.corr_pt, po.keep, normals)
        eM, ea = rel_err(po.M, M), rel_err(po.alpha, alpha)
        print(f"rank {r} K={K} {direction}: kept {int(po.keep.sum())}/{K} M {eM:.1e} alpha {ea:.1e}")
        assert eM < REL and ea < REL
