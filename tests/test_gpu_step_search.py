"""GPU: the per-query search of the lone-chain merged step (k_step_search / k_step_search_twin: launches 2 and 3 in one, through the
static target's resident patch balls and corner records) against the filter + resolve launches it replaces (ICP_STEP_SEARCH=split)
and against the per-method entry points.

Whatever route the searches take, a step's values are the same bits: the proposed state, the likelihood, the transition densities,
the correspondences' points, ids and keep flags, and the hints the searches leave (the winning triangle of every model id, the
nearest model vertex of every target sample).  Small synthetic meshes, at the counts where the new kernel changes its path:

* target triangle counts 1, 127, 128, 129 (a partial patch, an exact one, a one-triangle tail patch) and 8,200 (65 patches: a second
  round of ball tests); the same 8,200 with the triangle list shuffled (the sphere list is put into patches by the library whatever the
  file order: the case checks exactly that);
* a first step of a fresh context (every hint -1: the bound is infinite, every patch survives, the list overflows into the full scan)
  and a model vertex moved far off the surface;
* a model vertex at the centre of the target sphere: every patch is within its bound, more than the eight fetched together;
* exact ties: a model vertex straight above a target vertex shared by six triangles whose ids are scattered over the list, and every
  triangle of that fan duplicated at the end of the list — the lowest id must win (checked against the CPU oracle too);
* one degenerate target triangle (two equal corners) and one with a NaN corner, beside finite ones in the same patch;
* vertex search: models of 3, 63, 64, 65 and 70 vertices (70: a pole of 68 triangles, the normal's fall-back), duplicated model
  vertices (tie -> lowest index), a proposal with ONE target point;
* an evaluator count that is no multiple of 4 and larger than the proposal's (queries without a correspondence);
* a twin pass (both lanes) and one lane at a time, and a chain of the project's own harness long enough to accept and reject.

A child process per route runs every case (steps are launched ahead only while the process has one live context)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

R_TARGET, R_MODEL, RANK = 42.0, 40.0, 4


def sphere_grid(n_triangles, radius=R_TARGET):
    """a latitude / longitude sphere with at least n_triangles triangles, cut to the first n_triangles -> (points, cells)"""
    nlon = 8
    while 2 * nlon * (nlon // 2) < n_triangles:
        nlon += 2
    nlat = nlon // 2
    th = np.pi * (np.arange(nlat + 1) / nlat * 0.96 + 0.02)  # (no poles: every cell a proper quad)
    ph = 2.0 * np.pi * np.arange(nlon) / nlon
    pts = np.stack([radius * np.outer(np.sin(th), np.cos(ph)), radius * np.outer(np.sin(th), np.sin(ph)),
                    radius * np.outer(np.cos(th), np.ones(nlon))], axis=2).reshape(-1, 3)
    cells = []
    for i in range(nlat):
        for j in range(nlon):
            a, b, c, d = i * nlon + j, i * nlon + (j + 1) % nlon, (i + 1) * nlon + j, (i + 1) * nlon + (j + 1) % nlon
            cells += [(a, c, b), (b, c, d)]
    return pts, np.array(cells[:n_triangles], dtype=np.int32)


def bipyramid_model(n, rng, radius=R_MODEL):
    """a closed mesh of n vertices (a ring of n - 2 and two poles; n = 3: one triangle) with a random rank-4 basis"""
    if n == 3:
        pts = radius * np.array([[1.0, 0.0, 0.1], [-0.5, 0.8, 0.1], [-0.5, -0.8, 0.1]])
        cells = np.array([[0, 1, 2]], dtype=np.int32)
    else:
        m = n - 2
        ang = 2.0 * np.pi * np.arange(m) / m
        # (the ring wanders in z so that the queries spread over the target)
        ring = np.stack([radius * np.cos(ang) * 0.9, radius * np.sin(ang) * 0.9, 0.35 * radius * np.sin(3.0 * ang)], axis=1)
        pts = np.concatenate([ring, [[0.0, 0.0, radius], [0.0, 0.0, -radius]]])
        cells = np.array([(j, (j + 1) % m, m) for j in range(m)] + [((j + 1) % m, j, m + 1) for j in range(m)], dtype=np.int32)
    basis = rng.normal(size=(3 * n, RANK)) * 0.6
    return pts, cells, basis


CASES = {
    # name: target triangles, model vertices, proposal K, evaluator K, extras
    "t1": dict(T=1, N=65, K=8, Kev=16),
    "t127": dict(T=127, N=65, K=8, Kev=16),
    "t128": dict(T=128, N=65, K=8, Kev=16),
    "t129": dict(T=129, N=65, K=8, Kev=16),
    "t8200": dict(T=8200, N=65, K=8, Kev=16, far=3, centre=5),
    "t8200-shuffled": dict(T=8200, N=65, K=8, Kev=16, shuffle=True, centre=5),
    "ties": dict(T=2000, N=65, K=8, Kev=16, fan=True),
    "degenerate": dict(T=300, N=65, K=8, Kev=16, degenerate=True),
    "n3": dict(T=129, N=3, K=3, Kev=3, boundary_aware=False),  # (one triangle: every vertex on the boundary)
    "n63": dict(T=129, N=63, K=8, Kev=16),
    "n64": dict(T=129, N=64, K=8, Kev=16, twins=(7, 9)),
    "n70": dict(T=2000, N=70, K=70, Kev=70),
    "one-target-point": dict(T=2000, N=65, K=1, Kev=7),
    "odd-counts": dict(T=2000, N=65, K=5, Kev=7),
}


def build_case(pkg, name):
    """-> (model, target, target sample points of the TargetSampling proposal, spec)"""
    spec = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    tpts, tcells = sphere_grid(spec["T"])
    if name == "t1":  # (the one triangle below the model's pole instead of at the rim)
        tpts = np.concatenate([tpts, [[30.0, 0.0, 41.0], [-20.0, 25.0, 41.5], [-20.0, -25.0, 40.5]]])
        tcells = np.array([[len(tpts) - 3, len(tpts) - 2, len(tpts) - 1]], dtype=np.int32)
    mpts, mcells, basis = bipyramid_model(spec["N"], rng)
    still = []  # model vertices the basis does not move
    if "far" in spec:
        mpts[spec["far"]] = [900.0, 300.0, -200.0]
        still.append(spec["far"])
    if "centre" in spec:
        mpts[spec["centre"]] = [0.013, -0.007, 0.021]
        still.append(spec["centre"])
    if spec.get("shuffle"):
        tcells = tcells[rng.permutation(len(tcells))]
    if spec.get("fan"):
        # an interior grid vertex of the target and the six triangles around it: their ids are swapped with ids spread over the list,
        # then all six are appended once more (duplicates with higher ids)
        v = int(np.bincount(tcells.ravel()).argmax())
        fan = np.nonzero((tcells == v).any(axis=1))[0]
        assert len(fan) == 6
        for f, to in zip(fan, (1900, 3, 1205, 411, 1711, 64)):
            tcells[[f, to]] = tcells[[to, f]]
        fan = np.nonzero((tcells == v).any(axis=1))[0]
        tcells = np.concatenate([tcells, tcells[fan[::-1]]])
        mpts[2] = tpts[v] * 1.04  # straight above the shared vertex (the sphere is convex: its Voronoi region)
        still.append(2)
        spec = dict(spec, fan_ids=fan, fan_vertex=v)
    if spec.get("degenerate"):
        tcells[40] = [tcells[40][0], tcells[40][1], tcells[40][1]]
        tpts = np.concatenate([tpts, [[np.nan, 1.0, 2.0]]])
        tcells[41] = [tcells[41][0], len(tpts) - 1, tcells[41][2]]
    if "twins" in spec:
        a, b = spec["twins"]
        mpts[b] = mpts[a]
        basis[3 * b:3 * b + 3] = basis[3 * a:3 * a + 3]
    for s in still:
        basis[3 * s:3 * s + 3] = 0.0
    model = pkg.data.StatisticalMeshModel(mpts, mcells, np.zeros_like(mpts), basis, np.array([4.0, 3.0, 2.0, 1.0]))
    target = pkg.data.TriangleMesh(tpts, tcells)
    used = np.unique(tcells)
    used = used[np.isfinite(tpts[used]).all(axis=1)]
    tp = tpts[used[np.linspace(0, len(used) - 1, spec["K"]).astype(int)]] * 1.01
    if "twins" in spec:  # a target sample at equal distance from the two coincident model vertices
        tp[0] = mpts[spec["twins"][0]] * 1.03
    return model, target, tp, spec


def _objects(pkg, ctx, spec, tp):
    ba = spec.get("boundary_aware", True)
    props = [pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, spec["K"], pkg.TargetSampling, ba, decimatedTargetPoints=tp),
             # (not boundary-aware: the cut targets are open, and a boundary-aware ModelSampling proposal on an open target needs the
             # nearest-vertex pass of the wide step)
             pkg.NonRigidIcpProposal(ctx, 0.1, 10.0, 5.0, spec["K"], pkg.ModelSampling, False, decimatedTargetPoints=tp,
                                     numDecimatedModelPoints=min(spec["K"], ctx.N))]
    ev = pkg.IndependentPointDistanceEvaluator(ctx, 0.0, 2.0, pkg.ModelToTargetEvaluation, spec["Kev"], decimatedTargetPoints=tp,
                                               numDecimatedModelPoints=min(spec["Kev"], ctx.N))
    return ev, props


def search_hints(pkg, ctx, prop, n_surface, n_vertex):
    import ctypes as C
    s, v = np.zeros(max(n_surface, 1), dtype=np.int32), np.zeros(max(n_vertex, 1), dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    pkg._native.check(pkg._native.lib().icp_ctx_search_hints(ctx.h, prop.h if prop is not None else None, n_surface, s.ctypes.data_as(ip),
                                                             n_vertex, v.ctypes.data_as(ip)), "icp_ctx_search_hints")
    return s[:n_surface].copy(), v[:n_vertex].copy()


def drive(pkg, name, twin, n_rounds=4):
    """The first step of a fresh context, then rounds of two proposals A, B from a moving state: A is 'rejected', B 'accepted' (the
    decisions are fixed, so every route steps through the same states); twin: A and B are launched ahead as the two lanes of one pass.
    -> per step: the step's values, both proposals' correspondences of the proposed state, the hints left behind."""
    model, target, tp, spec = build_case(pkg, name)
    rng = np.random.default_rng(5)
    ctx = pkg.IcpContext(model, target, device=0)
    ev, props = _objects(pkg, ctx, spec, tp)
    cur = pkg.initial_parameters(model)
    cur[10:] = 0.3 * rng.normal(size=RANK)
    n_surf = min(max(spec["Kev"], spec["K"]), ctx.N)
    out, lanes = [], []

    def step(gen, z):
        th, lv, fwd, bwd = pkg.chain_step(ev, props, cur, gen, z=z)
        th = np.array(th, dtype=np.float64)
        rec = dict(theta=th, lv=lv, fwd=np.array(fwd), bwd=np.array(bwd))
        rec["hint_surf"], rec["hint_vert"] = search_hints(pkg, ctx, props[0], n_surf, spec["K"])
        for i, p in enumerate(props):  # (the step's own memo entries: what its searches and correspondence records wrote)
            post = p.icpPosterior(th, with_aux=False)
            rec["corr%d" % i] = (post.corr_id.copy(), post.corr_point.copy(), post.keep.copy())
        out.append(rec)
        return th

    for it in range(n_rounds):
        ga, za, gb, zb = it % 2, rng.normal(size=RANK), (it + 1) % 2, rng.normal(size=RANK)
        if twin and it > 0:  # (round 0: the fresh context's first step goes alone, unhinted)
            lanes.append(pkg.chain_step_prelaunch2(ev, props, cur, ga, za, gb, zb))
        step(ga, za)
        cur = step(gb, zb)
    stats = dict(twin=ctx.twin_stats(), paths=ctx.step_paths(), x_last=ctx.transformedMesh(cur), lanes=lanes)
    ev.close(); [p.close() for p in props]
    ctx.close()
    return out, stats


def per_method(pkg, name, thetas):
    """the same proposed states through the per-method entry points on a context that never takes a merged step"""
    model, target, tp, spec = build_case(pkg, name)
    ctx = pkg.IcpContext(model, target, device=0)
    ev, props = _objects(pkg, ctx, spec, tp)
    out = []
    for th in thetas:
        rec = dict(lv=ev.logValue(th))
        for i, p in enumerate(props):
            post = p.icpPosterior(th, with_aux=False)
            rec["corr%d" % i] = (post.corr_id.copy(), post.corr_point.copy(), post.keep.copy())
        out.append(rec)
    ev.close(); [p.close() for p in props]
    ctx.close()
    return out


def harness_chain(pkg, steps, fused):
    """the project's own chain (proposal mixture, Metropolis-Hastings decisions) on the 8,200-triangle case -> records, statistics"""
    model, target, _, _ = build_case(pkg, "t8200")
    setup = pkg.femur_icp_proposal_registration(model, target, n_icp_points=8, n_eval_points=15, fused=fused)
    for p in setup.icp:
        if p["direction"] == 0:
            p["boundary_aware"] = False  # (as _objects)
    ctx = pkg.IcpContext(model, target, device=0)
    chain = pkg.SamplingRegistration(ctx, setup, pkg.initial_parameters(model), 1024)
    rec = chain.run(steps)
    stats = dict(twin=ctx.twin_stats(), paths=ctx.step_paths(), runtime=pkg._native.runtime_stats())
    chain.close(); ctx.close()
    return rec, stats


_CHILD = r"""
import pickle, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as graft
import test_gpu_step_search as t
pkg = graft.load_package()
mode = {mode!r}
res = dict()
if mode == "per-method":
    thetas = pickle.load(open({thetas!r}, "rb"))
    res["cases"] = dict((name, t.per_method(pkg, name, thetas[name])) for name in t.CASES)
    res["chain"] = t.harness_chain(pkg, 60, 0)
else:
    res["cases"] = dict((name, t.drive(pkg, name, twin=True)) for name in t.CASES)
    res["one-lane"] = dict((name, t.drive(pkg, name, twin=False)) for name in ("t129", "t8200", "ties"))
    res["chain"] = t.harness_chain(pkg, 60, 2)
pickle.dump(res, open({out!r}, "wb"))
"""

_SWITCHES = ("ICP_STEP_SEARCH", "ICP_NO_TWIN", "ICP_NO_SPECULATION", "ICP_SPECULATION", "ICP_NO_PIPELINE", "ICP_LIBRARY_PATH")


def _child(tmp, tag, mode, env, thetas=""):
    out = str(tmp / (tag + ".pkl"))
    base = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    script = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), mode=mode, thetas=thetas, out=out)
    done = subprocess.run([sys.executable, "-c", script], env={**base, **env}, timeout=170, capture_output=True, text=True)
    assert done.returncode == 0, "%s: the child ended with %d\n%s" % (tag, done.returncode, done.stderr[-3000:])
    return pickle.load(open(out, "rb"))


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("step_search")
    got = {"fused": _child(tmp, "fused", "steps", {}), "split": _child(tmp, "split", "steps", {"ICP_STEP_SEARCH": "split"}),
           "fused-no-twin": _child(tmp, "fused-no-twin", "steps", {"ICP_NO_TWIN": "1"})}
    thetas = str(tmp / "thetas.pkl")
    pickle.dump({name: [s["theta"] for s in steps] for name, (steps, _) in got["fused"]["cases"].items()}, open(thetas, "wb"))
    got["per-method"] = _child(tmp, "per-method", "per-method", {}, thetas)
    return got


def _same_step(a, b, tag, hints=True):
    for key in ("theta", "lv", "fwd", "bwd") + (("hint_surf", "hint_vert") if hints else ()):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), (tag, key)
    for key in ("corr0", "corr1"):
        for x, y, what in zip(a[key], b[key], ("id", "point", "keep")):
            assert np.array_equal(x, y, equal_nan=True), (tag, key, what)


@pytest.mark.parametrize("name", list(CASES))
def test_fused_search_is_the_split_search(routes, name):
    """every step of the case: values, correspondences and hints of the one launch equal those of filter + resolve, bit for bit; all
    steps took the merged path, and twin passes were issued where the driver asked for them"""
    (fs, fstat), (ss, sstat) = routes["fused"]["cases"][name], routes["split"]["cases"][name]
    assert len(fs) == len(ss) == 8
    for k, (a, b) in enumerate(zip(fs, ss)):
        _same_step(a, b, "%s step %d" % (name, k))
    assert np.array_equal(fstat["x_last"], sstat["x_last"])
    for st in (fstat, sstat):
        assert st["paths"]["merged"] >= 8 and st["paths"]["per_stage"] == 0 and st["paths"]["wide"] == 0, st["paths"]
        assert st["lanes"] == [2, 2, 2] and st["twin"]["passes"] == 3 and st["twin"]["lane1_used"] == 3, (st["lanes"], st["twin"])
    # the hints are winners: a surface hint names a triangle of the target (or none where nothing is finite), a vertex hint a vertex
    T = CASES[name]["T"] + (6 if CASES[name].get("fan") else 0)
    for s in fs:
        assert ((s["hint_surf"] >= -1) & (s["hint_surf"] < T)).all() and ((s["hint_vert"] >= 0) & (s["hint_vert"] < CASES[name]["N"])).all()
        assert (s["hint_surf"] >= 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_fused_search_is_the_per_method_search(routes, name):
    """the proposed states of the fused run through icpPosterior / logValue of a context that never takes a merged step: the same
    correspondences and the same likelihood"""
    fs, _ = routes["fused"]["cases"][name]
    pm = routes["per-method"]["cases"][name]
    assert len(pm) == len(fs)
    for k, (a, b) in enumerate(zip(fs, pm)):
        assert a["lv"] == b["lv"], (name, k, a["lv"], b["lv"])
        for key in ("corr0", "corr1"):
            for x, y, what in zip(a[key], b[key], ("id", "point", "keep")):
                assert np.array_equal(x, y, equal_nan=True), (name, k, key, what)


@pytest.mark.parametrize("name", ["t129", "t8200", "ties"])
def test_twin_and_one_lane_passes_agree(routes, name):
    """the same calls without anything launched ahead (one-lane launches, k_step_search) and with ICP_NO_TWIN=1: the same steps;
    no twin pass where none was asked for.  (The hints are compared between runs of one kind only: the second lane of a twin pass
    reads the hints and leaves them as they are, a step launched by itself writes its winners.)"""
    ref, _ = routes["fused"]["cases"][name]
    one, ostat = routes["fused"]["one-lane"][name]
    assert ostat["twin"] == {"passes": 0, "lane1_used": 0, "lane1_dropped": 0}, ostat
    for k, (a, b) in enumerate(zip(ref, one)):
        _same_step(a, b, "%s step %d, one lane" % (name, k), hints=False)
    off, _ = routes["fused-no-twin"]["cases"][name]
    for k, (a, b) in enumerate(zip(ref, off)):
        _same_step(a, b, "%s step %d, ICP_NO_TWIN" % (name, k), hints=False)
    split_one, _ = routes["split"]["one-lane"][name]
    for k, (a, b) in enumerate(zip(one, split_one)):
        _same_step(a, b, "%s step %d, one lane, split" % (name, k))


def test_lowest_id_wins_the_ties(routes, oracle, pkg):
    """the model vertex above the shared target vertex: twelve triangles (the fan and its duplicates) at exactly the same distance,
    their ids scattered over the sphere list — the hint left by every step is the lowest of them, and the CPU oracle's winner for
    every model id of the last state; the coincident model vertices of case n64: the target sample between them is given the lower"""
    model, target, tp, spec = build_case(pkg, "ties")
    steps, stat = routes["fused"]["cases"]["ties"]
    lowest = int(spec["fan_ids"].min())
    assert lowest == 3
    for s in steps:
        assert s["hint_surf"][2] == lowest, s["hint_surf"][:4]
    # the last step was the accepted one, its lane's hints were written only if it ran as lane 0 — the one-lane run writes every step's
    one, ostat = routes["fused"]["one-lane"]["ties"]
    _, tri, _ = oracle.closest_point_on_surface(ostat["x_last"][:len(one[-1]["hint_surf"])], target.points, target.cells)
    assert np.array_equal(one[-1]["hint_surf"], tri)
    a, b = CASES["n64"]["twins"]
    for s in routes["fused"]["cases"]["n64"][0]:
        assert s["hint_vert"][0] == min(a, b), s["hint_vert"]


def test_harness_chain_records(routes):
    """60 steps of the project's own chain on the 65-patch target: accepted and rejected steps, twin passes issued (second lanes are
    used in the driven cases above: this chain accepts too often for that); the records of the one launch, of filter + resolve and of
    ICP_NO_TWIN=1 are equal bit for bit.  The per-method chain (fused=0) decomposes its posteriors in another order of warm and cold
    starts, its proposals agree to rounding: the same decisions and leaves, states and log values within the bounds
    tests/test_gpu_chain.py sets for the three ways of stepping against the oracle (1e-5 of the largest coefficient, 1e-6 of the largest
    log value) — the searches themselves are compared bit for bit in test_fused_search_is_the_per_method_search."""
    ref, st = routes["fused"]["chain"]
    acc = int(ref[:, 1].sum())
    print("accepted", acc, st)
    assert ref.shape[0] == 60 and 5 <= acc <= 55
    assert st["twin"]["passes"] > 0, st
    assert st["paths"]["merged"] >= 60 and st["paths"]["per_stage"] == 0, st
    assert all(v == 0 for v in st["runtime"].values()), st
    for tag in ("split", "fused-no-twin"):
        rec, other = routes[tag]["chain"]
        assert np.array_equal(rec, ref), tag
    rec, _ = routes["per-method"]["chain"]
    assert np.array_equal(rec[:, :3], ref[:, :3]), "decisions or leaves differ"
    d_state, d_lv = np.abs(rec[:, 14:] - ref[:, 14:]).max(), np.abs(rec[:, 3] - ref[:, 3]).max()
    print("per-method chain: states differ by", d_state, "log values by", d_lv)
    assert d_state <= 1e-5 * np.abs(ref[:, 14:]).max() and d_lv <= 1e-6 * np.abs(ref[:, 3]).max()
    assert routes["fused-no-twin"]["chain"][1]["twin"]["passes"] == 0
