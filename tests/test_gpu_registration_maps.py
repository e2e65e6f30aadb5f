"""GPU: per-vertex registration maps and their chain summaries (icp_registration_maps_many, icp_distance_summaries_many) against the
one-item route (transformedMesh -> closestPointOnTarget / closestTargetVertex + boundary flags / closestPointOnModel), the CPU oracle
and icp_mesh_metrics; batch and chunk invariance, wanted subsets, the summaries' left-to-right fold, and failures.  femur-50
(N = M = 1,622) on the bundled target and on open patches of it."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, make_theta, open_patch_target

pytestmark = pytest.mark.gpu

ICP_ERR_INVALID_ARG, ICP_ERR_NOT_FINITE, ICP_ERR_BUSY = -1, -3, -6  # include/icp_proposal.h
MAPS = ("m2t_point", "m2t_triangle", "m2t_distance", "m2t_on_boundary", "t2m_point", "t2m_triangle", "t2m_distance")
SUMMARIES = ("m2t_mean", "m2t_max", "t2m_mean", "t2m_max")
B = 12


def states(model, first, n):
    return np.stack([make_theta(model, first + b, shape_scale=0.4) for b in range(n)])


def one_item(pkg, ctx, target, theta):
    """the per-state route: four one-item calls, the boundary flags taken on the host"""
    x = ctx.transformedMesh(theta)
    cp, tri, d2 = ctx.closestPointOnTarget(x)
    flags = np.asarray(pkg.data.boundary_vertex_flags(target)).astype(np.uint8)
    onb = np.zeros(x.shape[0], dtype=np.uint8)
    if flags.any():
        idx, _ = ctx.closestTargetVertex(cp)
        onb = flags[idx]
    cpt, trit, d2t = ctx.closestPointOnModel(theta, target.points)
    return {"m2t_point": cp, "m2t_triangle": tri, "m2t_d2": d2, "m2t_on_boundary": onb, "t2m_point": cpt, "t2m_triangle": trit,
            "t2m_d2": d2t}


def ulps(got, want):
    """|got - want| in units of want's last place (0 where both are equal)"""
    return np.abs(got - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny))


def fold(d):
    """(((d0 + d1) + d2) + ...) / S and the maximum, per vertex, of the rows of d [S, K]"""
    acc = d[0].copy()
    for s in range(1, d.shape[0]):
        acc = acc + d[s]
    return acc / d.shape[0], d.max(axis=0)


def same_maps(a, b, keys=MAPS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys) and a["status"] == b["status"]


def three_patches(pkg, target):
    p1, c1 = open_patch_target(target)
    p2, c2 = open_patch_target(target, n_remove=400)
    return [target, pkg.data.TriangleMesh(p1, c1), pkg.data.TriangleMesh(p2, c2)]


@pytest.fixture(scope="module")
def scene(pkg, femur50):
    """contexts on the closed target and on two open patches; 12 states; their maps, once, by the batched call (per context) and by
    the one-item route — shared by the tests below and left unchanged"""
    model, target = femur50
    targets = three_patches(pkg, target)
    ctxs = [pkg.IcpContext(model, t, device=0) for t in targets]
    th = states(model, 60, B)
    full = [pkg.registration_maps(c, th) for c in ctxs[:2]]
    ref = [[one_item(pkg, c, t, th[b]) for b in range(B)] for c, t in zip(ctxs[:2], targets[:2])]
    yield {"model": model, "targets": targets, "ctxs": ctxs, "th": th, "full": full, "ref": ref}
    for c in ctxs:
        c.close()


def test_same_bits_as_the_one_item_route(scene):
    """Every row equals the four one-item calls' bit for bit; the distances are sqrt(d²) of those calls within one ulp (the device's
    f64 square root is correctly or faithfully rounded: it and numpy's correctly rounded one are neighbours at worst).  Measured on an
    MI355X: 0 ulp everywhere, so equality is asserted."""
    N = scene["model"].n_points
    worst = 0.0
    for k, target in enumerate(scene["targets"][:2]):
        for b in range(B):
            got, want = scene["full"][k][b], scene["ref"][k][b]
            assert got["status"] == 0
            for key in ("m2t_point", "m2t_triangle", "m2t_on_boundary", "t2m_point", "t2m_triangle"):
                assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (k, b, key)
                assert np.array_equal(got[key], want[key]), (k, b, key)
            for key, d2 in (("m2t_distance", want["m2t_d2"]), ("t2m_distance", want["t2m_d2"])):
                u = ulps(got[key], np.sqrt(d2)).max()
                worst = max(worst, u)
                assert u <= 1.0, (k, b, key, u)
            assert got["m2t_distance"].shape == (N,) and got["t2m_distance"].shape == (target.n_points,)
    print(f"largest |distance - sqrt(d2)| = {worst} ulp")
    assert worst == 0.0
    assert not any(m["m2t_on_boundary"].any() for m in scene["full"][0])      # closed target: no flag
    assert all(0 < m["m2t_on_boundary"].sum() < N for m in scene["full"][1])  # open target: the boundary round ran


def test_against_the_oracle(pkg, oracle, femur50_oracle, scene):
    """The standard tests/test_gpu_parity.py holds the one-item searches to: triangles, squared distances and points equal to the
    oracle's bit for bit (the instance included: the oracle searches its own om.instance(theta)); flags from oracle.nearest_vertex and
    OracleMesh.boundary()."""
    om, _ = femur50_oracle
    model = scene["model"]
    for k, target in enumerate(scene["targets"][:2]):
        tp = np.ascontiguousarray(target.points, dtype=np.float64)
        flags = oracle.OracleMesh(tp, target.cells).boundary()
        assert np.array_equal(flags != 0, np.asarray(pkg.data.boundary_vertex_flags(target)) != 0)
        for b in (0, 5, 11):
            got = scene["full"][k][b]
            x = om.instance(scene["th"][b])
            cp, tri, d2 = oracle.closest_point_on_surface(x, tp, target.cells)
            assert np.array_equal(got["m2t_triangle"], tri) and np.array_equal(got["m2t_point"], cp), (k, b)
            assert ulps(got["m2t_distance"], np.sqrt(d2)).max() <= 1.0, (k, b)
            idx, _ = oracle.nearest_vertex(cp, tp)
            assert np.array_equal(got["m2t_on_boundary"], flags[idx]), (k, b)
            cpt, trit, d2t = oracle.closest_point_on_surface(tp, x, model.cells)
            assert np.array_equal(got["t2m_triangle"], trit) and np.array_equal(got["t2m_point"], cpt), (k, b)
            assert ulps(got["t2m_distance"], np.sqrt(d2t)).max() <= 1.0, (k, b)


def test_agrees_with_mesh_metrics(pkg, scene):
    """icp_mesh_metrics reduces the same rows: maxima and counts exactly, the average within 1e-12 (only the order of the sum differs)"""
    N = scene["model"].n_points
    for k, ctx in enumerate(scene["ctxs"][:2]):
        for b in range(B):
            got = scene["full"][k][b]
            m = pkg.evaluate_reconstruction_to_ground_truth(ctx, scene["th"][b])
            keep = got["m2t_on_boundary"] == 0
            assert m["hausdorff"] == max(got["m2t_distance"].max(), got["t2m_distance"].max()), (k, b)
            assert m["kept"] == keep.sum(), (k, b)
            assert m["max_boundary_aware"] == got["m2t_distance"][keep].max(), (k, b)
            mean = got["m2t_distance"].mean()
            assert abs(m["average2surface"] - mean) <= 1e-12 * mean, (k, b)
            if k == 1:
                assert 0 < m["kept"] < N


def batch_of_40(pkg, model, ctxs):
    th = states(model, 400, 40)
    return th, [ctxs[b % 3] for b in range(40)]


def test_batch_invariance(pkg, scene):
    """40 items on three contexts in one call, then as calls of 1 and 7 items in shuffled order: identical arrays"""
    th, cx = batch_of_40(pkg, scene["model"], scene["ctxs"])
    whole = pkg.registration_maps(cx, th)
    assert all(m["status"] == 0 for m in whole)
    perm = np.random.default_rng(3).permutation(40)
    i, size = 0, 1
    while i < 40:
        sel = perm[i:i + size]
        part = pkg.registration_maps([cx[b] for b in sel], th[sel])
        for b, m in zip(sel, part):
            assert same_maps(m, whole[b]), b
        i += size
        size = 8 - size  # 1, 7, 1, 7, …


def chunks_of(doubles, cap):
    """the chunks abi_registration_maps.inl lays out for items of `doubles` staging doubles each under a staging of `cap`"""
    sizes, rows = [0], 0
    for d in doubles:
        if sizes[-1] > 0 and rows + d > cap:
            sizes.append(0)
            rows = 0
        sizes[-1] += 1
        rows += d
    return sizes


def _chunk_check():
    """(run as a program with the test-hooks library loaded) the 40-item batch and the summaries of a 33-sample set between two
    others under ICP_TEST_MAPS_CHUNK_DOUBLES: the bits of the default staging."""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    model, target = pkg.data.load_femur_model_and_target(50)
    ctxs = [pkg.IcpContext(model, t, device=0) for t in three_patches(pkg, target)]
    N = model.n_points
    th, cx = batch_of_40(pkg, model, ctxs)
    sets = [states(model, 700, 5), states(model, 800, 33), states(model, 900, 2)]
    os.environ.pop("ICP_TEST_MAPS_CHUNK_DOUBLES", None)
    want = pkg.registration_maps(cx, th)
    want_s = pkg.distance_summaries(ctxs[1], sets)
    cap = 13 * 12 * N
    sizes = chunks_of([6 * (N + c.target.n_points) for c in cx], cap)
    assert len(sizes) >= 3 and sizes[-1] < sizes[0], sizes        # several chunks, a partial last one
    sizes_s = chunks_of([6 * (N + ctxs[1].target.n_points)] * 40, cap)
    assert len(sizes_s) >= 3 and sizes_s[0] < 33, sizes_s         # the 33-sample set spans chunks
    os.environ["ICP_TEST_MAPS_CHUNK_DOUBLES"] = str(cap)
    got = pkg.registration_maps(cx, th)
    for b in range(40):
        assert same_maps(got[b], want[b]), b
    got_s = pkg.distance_summaries(ctxs[1], sets)
    d = np.stack([m["m2t_distance"] for m in pkg.registration_maps(ctxs[1], sets[1], want=("m2t_distance",))])
    mean, mx = fold(d)
    assert np.array_equal(got_s[1]["m2t_mean"], mean) and np.array_equal(got_s[1]["m2t_max"], mx)
    for m in range(3):
        for k in SUMMARIES:
            assert np.array_equal(got_s[m][k], want_s[m][k]), (m, k)
    os.environ["ICP_TEST_MAPS_CHUNK_DOUBLES"] = "1"               # one item a chunk: every set but the last spans chunks
    got_1 = pkg.distance_summaries(ctxs[1], sets)
    for m in range(3):
        for k in SUMMARIES:
            assert np.array_equal(got_1[m][k], want_s[m][k]), (m, k)
    for c in ctxs:
        c.close()
    print("chunk check ok")


def test_forced_small_chunks_give_the_same_bits():
    """Test-hooks build: a staging of about 13 items (the 40-item batch in four chunks, the last one partial; a 33-sample set split
    between chunks) and of one item gives every map and summary the bits of the default."""
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "chunk check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


def test_wanted_subsets(pkg, scene):
    """asking for less gives the same bits: one array alone, one direction alone, the flags alone"""
    ctx, th, full = scene["ctxs"][1], scene["th"], scene["full"][1]
    for want in (("m2t_distance",), ("t2m_distance", "t2m_triangle"), ("m2t_on_boundary",), ("m2t_point", "t2m_point")):
        got = pkg.registration_maps(ctx, th, want=want)
        for b in range(B):
            assert sorted(got[b]) == sorted(want + ("status",))
            assert same_maps(got[b], full[b], keys=want), (want, b)
    one = ctx.distanceMap(th[3])
    assert same_maps(one, full[3])


def test_summaries_are_the_left_to_right_fold(pkg, scene):
    """S = 1, S = 2, two sets sharing a context, a set on another context; then the sets in reversed order: every row is the numpy
    fold of registration_maps' distances, sample after sample"""
    ctxs, th = scene["ctxs"], scene["th"]
    sets = [th[:1], th[1:3], th[3:12], th[2:9]]
    cx = [ctxs[0], ctxs[1], ctxs[1], ctxs[2]]
    got = pkg.distance_summaries(cx, sets)
    for m, (c, s) in enumerate(zip(cx, sets)):
        maps = pkg.registration_maps(c, s, want=("m2t_distance", "t2m_distance"))
        for side in ("m2t", "t2m"):
            mean, mx = fold(np.stack([v[side + "_distance"] for v in maps]))
            assert got[m]["status"] == 0
            assert np.array_equal(got[m][side + "_mean"], mean), (m, side)
            assert np.array_equal(got[m][side + "_max"], mx), (m, side)
    assert np.array_equal(got[0]["m2t_mean"], got[0]["m2t_max"])  # (one sample)
    back = pkg.distance_summaries(cx[::-1], sets[::-1])
    for m in range(4):
        for k in SUMMARIES:
            assert np.array_equal(back[3 - m][k], got[m][k]), (m, k)
    only = pkg.distance_summaries(cx, sets, want=("t2m_max",))
    assert all(sorted(o) == ["status", "t2m_max"] and np.array_equal(o["t2m_max"], g["t2m_max"]) for o, g in zip(only, got))


def test_summaries_from_logs(pkg, scene):
    """loggers.distance_summaries_from_logs == the direct call on the states samples_from_log picks"""
    model, ctxs = scene["model"], scene["ctxs"]
    logs = []
    for k in range(2):
        th = states(model, 1000 + 100 * k, 30)
        logs.append([{"index": i, "status": bool(i % 3 != 1), "rigid": [float(v) for v in t[1:10]], "coeff": [float(v) for v in t[10:]]}
                     for i, t in enumerate(th)])
    out = pkg.loggers.distance_summaries_from_logs(ctxs[:2], logs, take_every_n=4, total=30, burn_in=3)
    for k in range(2):
        picked = pkg.loggers.samples_from_log(logs[k], take_every_n=4, total=30, burn_in=3)
        assert out["indices"][k] == [i for _, i in picked] and len(picked) >= 5
        th = np.stack([pkg.loggers.JSONAcceptRejectLogger.sample_to_model_parameters(s) for s, _ in picked])
        direct = pkg.distance_summaries(ctxs[k], [th])[0]
        for key in SUMMARIES:
            assert np.array_equal(out["summaries"][k][key], direct[key]), (k, key)


def test_failures(pkg, scene):
    """An item whose pose scale and coefficients overflow its mesh (1e300 each: every coordinate is ±inf or NaN) gets status -3, NaN
    rows, triangles -1 and flags 0, its neighbours the bits of a call without it; a set holding it likewise.  A context in a batch in
    flight: ICP_ERR_BUSY.  Contexts of two models: refused.  Nothing is written in the last two."""
    model, ctxs, th = scene["model"], scene["ctxs"], scene["th"]
    bad = th[1].copy()
    bad[0] = 1e300
    bad[10:] = 1e300
    got = pkg.registration_maps([ctxs[1], ctxs[1], ctxs[0]], np.stack([th[0], bad, th[2]]))
    assert [m["status"] for m in got] == [0, ICP_ERR_NOT_FINITE, 0]
    assert same_maps(got[0], scene["full"][1][0]) and same_maps(got[2], scene["full"][0][2])
    for key in ("m2t_point", "m2t_distance", "t2m_point", "t2m_distance"):
        assert np.all(np.isnan(got[1][key])), key
    assert np.all(got[1]["m2t_triangle"] == -1) and np.all(got[1]["t2m_triangle"] == -1) and not got[1]["m2t_on_boundary"].any()
    with pytest.raises(pkg._native.IcpNativeError) as e:
        ctxs[1].distanceMap(bad)
    assert e.value.status == ICP_ERR_NOT_FINITE
    sums = pkg.distance_summaries(ctxs[1], [th[:3], np.stack([th[0], bad, th[2]]), th[3:5]])
    assert [s["status"] for s in sums] == [0, ICP_ERR_NOT_FINITE, 0]
    assert all(np.all(np.isnan(sums[1][k])) for k in SUMMARIES) and all(np.all(np.isfinite(sums[m][k])) for m in (0, 2) for k in SUMMARIES)
    alone = pkg.distance_summaries(ctxs[1], [th[:3]])[0]
    assert all(np.array_equal(sums[0][k], alone[k]) for k in SUMMARIES)

    nat, lib = pkg._native, pkg._native.lib()
    N, r = model.n_points, model.rank
    dist = [np.full(N, 7.0), np.full(N, 7.0)]
    status = np.full(2, 99, dtype=np.int32)
    dp = nat.c_double_p

    def call(cx, thetas):
        c_ctx = (ctypes.c_void_p * 2)(*[c.h for c in cx])
        c_th = (dp * 2)(*[t.ctypes.data_as(dp) for t in thetas])
        c_out = (dp * 2)(*[d.ctypes.data_as(dp) for d in dist])
        return lib.icp_registration_maps_many(2, c_ctx, c_th, None, None, c_out, None, None, None, None, status.ctypes.data_as(nat.c_int_p))

    def call_sets(cx, thetas):
        c_ctx = (ctypes.c_void_p * 2)(*[c.h for c in cx])
        c_th = (dp * 2)(*[t.ctypes.data_as(dp) for t in thetas])
        c_out = (dp * 2)(*[d.ctypes.data_as(dp) for d in dist])
        ns = np.ones(2, dtype=np.int32)
        return lib.icp_distance_summaries_many(2, c_ctx, ns.ctypes.data_as(nat.c_int_p), c_th, c_out, None, None, None,
                                               status.ctypes.data_as(nat.c_int_p))
    m200, t200 = pkg.data.load_femur_model_and_target(200)
    c200 = pkg.IcpContext(m200, t200, device=0)
    busy_ctx = pkg.IcpContext(model, scene["targets"][0], device=0)
    tp = pkg.data.decimated_point_subset(scene["targets"][0], 2 * r)
    busy_ev = pkg.IndependentPointDistanceEvaluator(busy_ctx, 0.0, 2.0, pkg.ModelToTargetEvaluation, 4 * r, decimatedTargetPoints=tp)
    busy_prop = pkg.NonRigidIcpProposal(busy_ctx, 0.1, 10.0, 5.0, 2 * r, pkg.ModelSampling, True, decimatedTargetPoints=tp)
    try:
        two = [th[0].copy(), th[1].copy()]
        assert call([ctxs[0], c200], [two[0], np.zeros(10 + m200.rank)]) == ICP_ERR_INVALID_ARG   # two models
        assert call_sets([ctxs[0], c200], [two[0], np.zeros(10 + m200.rank)]) == ICP_ERR_INVALID_ARG
        tk = pkg.BatchedStepTicket([busy_ev], [[busy_prop]], [two[0]], [0], z=[np.random.default_rng(2).normal(size=r)])
        assert call([ctxs[0], busy_ctx], two) == ICP_ERR_BUSY
        assert call_sets([ctxs[0], busy_ctx], two) == ICP_ERR_BUSY
        tk.abandon()
        assert all(np.all(d == 7.0) for d in dist) and np.all(status == 99)
        assert call([ctxs[0], busy_ctx], two) == 0 and np.all(status == 0)
        assert np.array_equal(dist[0], scene["full"][0][0]["m2t_distance"]) and np.array_equal(dist[1], scene["full"][0][1]["m2t_distance"])
    finally:
        busy_ev.close(); busy_prop.close(); busy_ctx.close(); c200.close()


if __name__ == "__main__":
    _chunk_check()
