"""GPU: uniform surface samples with nearest vertices and a kernel's total variance (icp_surface_samples_many,
icp_kernel_total_variance_many, api.surface_samples, api.total_variance, data.surface_samples / approx_total_variance / fit_samples;
DESIGN.md §5.19) — every comparison with the numpy long form (tests/surface_samples_long_form.py) is bit for bit unless it says
otherwise."""
import os
import subprocess
import sys

import numpy as np
import pytest

import face_kernel_long_form as FK
import surface_samples_long_form as LF
from surface_samples_long_form import make, raw_call, same, assert_item

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, BLOCK, VTILE = LF.SCAN_TILE, LF.BLOCK, LF.VERTEX_TILE


def long_form_of(item, vertex_ids=True):
    return LF.long_form(item["points"], item["cells"], item["n"], item["seed"], vertex_ids)


def check(pkg, items, what):
    rc, got = raw_call(pkg, items, expect=(0, LF.NO_AREA))
    lfs = [long_form_of(it) for it in items]
    for b, (g, lf) in enumerate(zip(got, lfs)):
        assert_item(g, lf, (what, b))
    return got, lfs


ONE = (np.array([[0.0, 0.0, 0.0], [3.0, 0.5, 0.0], [1.0, 2.0, 0.25]]), [[0, 1, 2]])


@pytest.mark.gpu
def test_smallest_shapes(pkg):
    """T = 1 at the block edges of the pick and of the nearest-vertex search; strips of T triangles around the scan tile's edges, the
    areas growing along the strip"""
    items = [make(*ONE, n, seed=n) for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)]
    items += [make(*LF.strip(T), 700 if T < 3 * TILE else 30000, seed=T) for T in (TILE - 1, TILE, TILE + 1, 3 * TILE + 1)]
    got, lfs = check(pkg, items, "smallest")
    assert all(g["status"] == 0 for g in got)
    assert [int(g["info"][0]) for g in got] == [1] * 5 + [TILE - 1, TILE, TILE + 1, 3 * TILE + 1]
    # every tile of the largest strip is drawn from; its last tile holds one triangle (the long form: 8 of the 30,000 draws)
    assert np.unique(got[8]["cells"] // TILE).size == 4 and (got[8]["cells"] == 3 * TILE).sum() == 8


def degenerate_items():
    pts, cells = LF.strip(40)
    rep, col = [[4, 4, 5]], [[1, 2, 3]]  # a repeated corner; three corners on the strip's lower row: collinear
    run = np.tile(np.array(rep + col, dtype=np.int32), (TILE // 2 + 10, 1))  # more than a whole scan tile of them
    return [make(pts, np.concatenate([rep, cells]), 500, 1), make(pts, np.concatenate([cells, col]), 500, 2),
            make(pts, np.concatenate([cells[:17], col, rep, cells[17:]]), 500, 3),
            make(pts, np.concatenate([cells[:9], run, cells[9:]]), 500, 4), make(pts, np.concatenate([run, cells, run]), 500, 5)]


@pytest.mark.gpu
def test_triangles_without_area_are_never_drawn(pkg):
    items = degenerate_items()
    got, _ = check(pkg, items, "zero weights")
    for b, (g, it) in enumerate(zip(got, items)):
        area = LF.double_areas(it["points"], it["cells"])
        assert g["status"] == 0 and np.all(area[g["cells"]] > 0.0), b
        assert int(g["info"][0]) == 40 == int((area > 0.0).sum()), b


@pytest.mark.gpu
def test_size_ratio(pkg):
    """one triangle 2^33 times the others: they quantise to 0 and are never drawn; at 2^31 their weight is 2 of 2^32 + ..., and they
    are drawn exactly when x falls on them — which the long form decides"""
    def mesh(ratio, small=3000):
        j = np.arange(small, dtype=np.float64)
        pts = np.concatenate([[[0.0, 0.0, 0.0], [ratio, 0.0, 0.0], [0.0, 2.0, 0.0]], np.stack([j, 0 * j + 5.0, 0 * j], axis=1),
                              np.stack([j + 1.0, 0 * j + 5.0, 0 * j], axis=1), np.stack([j, 0 * j + 7.0, 0 * j], axis=1)])
        a = 3 + np.arange(small)
        return pts, np.concatenate([[[0, 1, 2]], np.stack([a, a + small, a + 2 * small], axis=1)])
    never, sometimes = make(*mesh(2.0 ** 33), 4000, 7), make(*mesh(2.0 ** 31), 60000, 8)
    got, lfs = check(pkg, [never, sometimes], "ratio")
    q = [LF.weights(it["points"], it["cells"])[0] for it in (never, sometimes)]
    assert q[0][0] == 2 ** 32 and np.all(q[0][1:] == 0) and np.all(got[0]["cells"] == 0) and got[0]["info"][0] == 1.0
    assert q[1][0] == 2 ** 32 and np.all(q[1][1:] == 2) and got[1]["info"][0] == 3001.0
    # 60,000 draws at probability 6000 / (2^32 + 6000) each: the long form says how many fall on the small ones
    assert int((got[1]["cells"] > 0).sum()) == int((lfs[1]["cells"] > 0).sum())


@pytest.mark.gpu
def test_an_item_without_area_fails_alone(pkg):
    pts, cells = LF.strip(30)
    flat = make(pts, [[0, 1, 2], [3, 3, 4], [5, 5, 5]], 300, 9)  # collinear, repeated, a point
    before, after = make(pts, cells, 300, 1), make(*ONE, 300, 2)
    rc, got = raw_call(pkg, [before, flat, after], expect=(LF.NO_AREA,))
    assert b"no area" in pkg._native.lib().icp_last_error()
    assert [g["status"] for g in got] == [0, LF.NO_AREA, 0]
    assert np.all(np.isnan(got[1]["points"])) and np.all(np.isnan(got[1]["bary"])) and np.all(got[1]["cells"] == -1)
    assert np.all(got[1]["vertex_ids"] == -1) and got[1]["info"].tolist() == [0.0, 0.0, 0.0, 0.0]
    for g, it in zip(got, (before, flat, after)):
        assert_item(g, long_form_of(it), "no area")
    _, alone = raw_call(pkg, [before])
    _, alone2 = raw_call(pkg, [after])
    assert all(same(got[0][k], alone[0][k]) and same(got[2][k], alone2[0][k]) for k in LF.OUTPUTS)
    # one item outside the limits among good ones: its status alone, nothing of it written
    bad = make(pts, cells, 300, 1)
    bad["cells"] = bad["cells"].copy()
    bad["cells"][7, 1] = pts.shape[0]
    rc, got = raw_call(pkg, [before, bad, after], expect=(-1,))
    assert [g["status"] for g in got] == [0, -1, 0] and LF.untouched(got[1])
    assert all(same(got[0][k], alone[0][k]) and same(got[2][k], alone2[0][k]) for k in LF.OUTPUTS)


@pytest.mark.gpu
def test_nearest_vertex(pkg):
    # a duplicated vertex: the triangle uses the higher id, the lower id at the same coordinates wins
    tri = ONE[0]
    dup = make(np.concatenate([tri, tri]), [[3, 4, 5]], 600, 1)
    # a needle beside a separate vertex.  With the separate vertex at (50, −0.01, 0) it mirrors the apex (50, 0.01, 0) in the line y = 0,
    # and every point of the triangle has y >= 0: the apex is never farther, so no sample can name vertex 3 (at y = 0 the two are equally
    # far and the lower id wins).  That mesh is compared with the long form; the assertion that some sample names a vertex that is no
    # corner of its triangle is made on the same needle with the separate vertex at (25, −0.01, 0), 25 away from the nearest corner.
    corners = [[0.0, 0.0, 0.0], [100.0, 0.0, 0.0], [50.0, 0.01, 0.0]]
    mirrored = make(corners + [[50.0, -0.01, 0.0]], [[0, 1, 2]], 600, 2)
    needle = make(corners + [[25.0, -0.01, 0.0]], [[0, 1, 2]], 600, 2)
    # M around the wave and around the LDS tile of the search: random vertices about one triangle (M = 1: a point, no area)
    rng = np.random.default_rng(4)
    sizes = (1, 63, 64, 65, VTILE - 1, VTILE, VTILE + 1, 2 * VTILE + 5)
    clouds = [make(np.concatenate([tri, rng.uniform(-0.5, 3.5, size=(M, 3)) * [1.0, 1.0, 0.1]])[:M], [[0, min(1, M - 1), min(2, M - 1)]], 400, M)
              for M in sizes]
    got, lfs = check(pkg, [dup, needle, mirrored] + clouds, "nearest")
    assert np.all(got[0]["vertex_ids"] < 3) and np.unique(got[0]["vertex_ids"]).size == 3
    assert (got[1]["vertex_ids"] == 3).sum() >= 1 and np.all(got[1]["cells"] == 0)
    assert np.all(got[2]["vertex_ids"] < 3)
    assert got[3]["status"] == LF.NO_AREA and all(g["status"] == 0 for g in got[4:])
    for g in got[5:]:  # many samples of a cloud name a vertex that is no corner of the one triangle
        assert (g["vertex_ids"] > 2).sum() > 100


# ---------------------------------------------------------------- NULL outputs, canaries

@pytest.mark.gpu
def test_null_outputs(pkg):
    items = degenerate_items()[:3] + [make(*ONE, 257, 5), make(*LF.strip(TILE + 1), 300, 6)]
    lfs = [long_form_of(it) for it in items]
    names = LF.OUTPUTS
    for whole in names:  # each output argument NULL in turn
        _, got = raw_call(pkg, items, whole_null=(whole,))
        for b, g in enumerate(got):
            assert g[whole] is None
            assert_item(g, lfs[b], ("whole", whole, b))
    for name in names:   # each entry NULL for one item
        nulls = [(name,) if b == 2 else () for b in range(len(items))]
        _, got = raw_call(pkg, items, nulls)
        for b, g in enumerate(got):
            assert_item(g, lfs[b], ("entry", name, b))
    nulls = [tuple(set(names) - {names[b % 5]}) for b in range(len(items))]  # one output each
    _, got = raw_call(pkg, items, nulls)
    for b, g in enumerate(got):
        assert g[names[b % 5]] is not None
        assert_item(g, lfs[b], ("one output", b))


# ---------------------------------------------------------------- determinism: alone, shuffled, small rounds, without ids

def mixed_items(pkg):
    """40 items of mixed (M, T, n), the item without area among them"""
    _, target = pkg.data.load_femur_model_and_target(50)
    rng = np.random.default_rng(12)
    pts30, cells30 = LF.strip(30)
    items = []
    for b in range(40):
        kind = b % 5
        if b == 13:
            items.append(make(pts30, [[0, 1, 2], [3, 3, 4]], 100, b))
        elif kind == 0:
            items.append(make(*LF.strip(int(rng.integers(1, 3 * TILE))), int(rng.integers(1, 900)), b))
        elif kind == 1:
            items.append(make(target.points, target.cells, int(rng.integers(1, 400)), b))
        elif kind == 2:
            M = int(rng.integers(3, 1500))
            items.append(make(rng.normal(size=(M, 3)), rng.integers(0, M, size=(int(rng.integers(1, 800)), 3)), int(rng.integers(1, 600)), b))
        elif kind == 3:
            items.append(make(*ONE, int(rng.integers(1, 700)), b))
        else:
            items.append(degenerate_items()[b % 4] | {"seed": b, "n": 150 + b})
    return items


def same_item(a, b):
    return a["status"] == b["status"] and all(a[k] is None or b[k] is None or same(a[k], b[k]) for k in LF.OUTPUTS)


def chunk_check():
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    hook = "ICP_TEST_SAMPLES_CHUNK_DOUBLES"
    os.environ.pop(hook, None)
    items = mixed_items(pkg)
    rc, whole = raw_call(pkg, items, expect=(LF.NO_AREA,))
    assert [g["status"] for g in whole] == [LF.NO_AREA if b == 13 else 0 for b in range(40)]
    for b, it in enumerate(items):
        assert_item(whole[b], long_form_of(it), ("mixed", b))
    # calls of 1 and 7 items in shuffled order
    order = np.random.default_rng(5).permutation(40)
    at = 0
    for size in [1, 7] * 5:
        sel = order[at:at + size]
        at += size
        _, part = raw_call(pkg, [items[b] for b in sel], expect=(0, LF.NO_AREA))
        assert all(same_item(p, whole[b]) for p, b in zip(part, sel)), ("shuffled", sel)
    assert at == 40
    # rounds of one item, and rounds that two small items share
    for words in ("1", "9000"):
        os.environ[hook] = words
        _, other = raw_call(pkg, items, expect=(LF.NO_AREA,))
        assert all(same_item(a, b) for a, b in zip(whole, other)), ("rounds", words)
        os.environ.pop(hook)
    # without vertex ids for some items (in rounds of one: some rounds skip the search altogether), and for all
    for nulls, env in (([("vertex_ids",) if b % 3 else () for b in range(40)], "1"), ([("vertex_ids",) if b % 2 else () for b in range(40)], None),
                       ([("vertex_ids",)] * 40, None)):
        if env:
            os.environ[hook] = env
        _, other = raw_call(pkg, items, nulls, expect=(LF.NO_AREA,))
        os.environ.pop(hook, None)
        assert all(same_item(a, b) for a, b in zip(whole, other)), "without ids"
    # the same seed twice: the same bits; another seed: other cells
    _, again = raw_call(pkg, items, expect=(LF.NO_AREA,))
    assert all(same_item(a, b) and all(same(a[k], b[k]) for k in LF.OUTPUTS) for a, b in zip(whole, again))
    _, reseeded = raw_call(pkg, [it | {"seed": it["seed"] + 1000} for it in items], expect=(LF.NO_AREA,))
    assert all(not same(a["cells"], b["cells"]) for q, (a, b) in enumerate(zip(whole, reseeded)) if q != 13 and items[q]["n"] >= 20 and items[q]["cells"].shape[0] > 1)
    print("chunk check ok")


@pytest.mark.gpu
def test_an_items_bits_do_not_depend_on_the_batch_the_rounds_or_the_outputs():
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=300,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "chunk check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


# ---------------------------------------------------------------- one large item

FULL_IDS = 2000  # vertex ids are compared with the long form for the first 2,000 samples: 1.2e8 distances in numpy.  A condition of the test.


@pytest.fixture(scope="module")
def big_target(pkg):
    _, big = pkg.data.synthetic_femur_target()
    assert big.n_points == 58322 and big.n_cells == 116640
    return big


@pytest.mark.gpu
def test_one_large_item(pkg, big_target):
    big, n = big_target, 50000
    got = pkg.surface_samples([big], [n], [1024])[0]
    lf = LF.long_form(big.points, big.cells, n, 1024, ids_for=FULL_IDS)
    assert got.status == 0
    assert same(got.points, lf["points"]) and same(got.cells, lf["cells"]) and same(got.bary, lf["bary"])
    assert [float(got.info["triangles"]), got.info["largest_area"], got.info["area"]] == lf["info"][:3].tolist()
    assert same(got.vertex_ids[:FULL_IDS], lf["vertex_ids"])
    # for all 50,000: the reported vertex is at most as far as the nearest corner of the sample's own triangle
    c = big.cells[got.cells]
    corner = np.min([LF.squared_distance(got.points, big.points[c[:, j]]) for j in range(3)], axis=0)
    assert got.vertex_ids.min() >= 0 and got.vertex_ids.max() < big.n_points
    assert np.all(LF.squared_distance(got.points, big.points[got.vertex_ids]) <= corner)
    area = 0.5 * LF.double_areas(big.points, big.cells)
    assert abs(got.info["area"] - area.sum()) <= 1e-6 * area.sum() and got.info["largest_area"] == area.max()


# ---------------------------------------------------------------- total variance

TV_COUNTS = (1, 255, 256, 257, 513, 50000)


@pytest.mark.gpu
def test_total_variance_bit_for_bit(pkg, big_target):
    """the femur kernel has no mirror and no weights, and exp(−0) = 1 on both sides: the trace is the same at every point, and the
    fixed tree gives the same bits on both sides"""
    femur, _, _ = pkg.data.load_femur_mesh("femur_reference")
    kernel = pkg.data.femur_kernel(femur)
    pts = pkg.surface_samples([big_target], [50000], [3], vertex_ids=False)[0].points
    got = pkg.total_variance([pts[:n] for n in TV_COUNTS], kernel)
    want = [LF.total_variance(pts[:n], kernel) for n in TV_COUNTS]
    assert got.tolist() == want
    trace = 10.0 * np.trace(kernel[0].A) + 24.0
    assert np.all(np.abs(got - trace) <= 1e-12 * trace)
    assert pkg.total_variance(pts[:300], kernel)[0] == LF.total_variance(pts[:300], kernel)  # one array: one item


@pytest.mark.gpu
def test_total_variance_of_a_face_kernel(pkg):
    """B-spline terms with region weights at the sample points and mirror gain 0.7.  The device's and numpy's exp and B-spline sums may
    differ in the last place, so the comparison has a tolerance, derived: every trace term is non-negative (A[c][c] >= 0, the mirrored
    base value b_m <= b by Cauchy-Schwarz on the spline sums, gain <= 1), so the relative errors of the terms carry over to their sum —
    a few 2^-53 per factor (some ten roundings in the spline sums and products, two in the weights: under 40·2^-53) —, and the tree adds
    (8 + the number of blocks)·2^-53 at most: with 196 blocks at n = 50,000 under 250·2^-53 < 3e-14.  rtol = 1e-12 holds that with
    room, and is what the issue sets."""
    g = 21
    mesh = pkg.data.TriangleMesh(FK.patch(g, 0.3), FK.grid_cells(g))
    mask = pkg.data.FaceMask(FK.masks(mesh.points)["part"])
    kernel = pkg.face_kernel(mesh, mask)
    assert all(k.weights is not None and k.mirror_gain == 0.7 for k in kernel)
    smp = pkg.surface_samples([mesh], [50000], [77], vertex_ids=False)[0].points
    pw = pkg.region_weights([smp] * len(kernel), [mask.region(mesh, k.level) for k in kernel], 40.0)
    got = pkg.total_variance([smp[:n] for n in TV_COUNTS], kernel, [[w[:n] for w in pw] for n in TV_COUNTS])
    for n, value in zip(TV_COUNTS, got):
        want = LF.total_variance(smp[:n], kernel, [w[:n] for w in pw])
        print("n", n, "device", value, "long form", want, "relative difference", abs(value - want) / want)
        assert want > 0.0 and abs(value - want) <= 1e-12 * want, n
    assert pkg.data.approx_total_variance(mesh, kernel, 50000, 77, mask=mask) == got[-1]


# ---------------------------------------------------------------- the Python glue

@pytest.mark.gpu
def test_fit_samples_feed_the_fits(pkg, femur50):
    model, target = femur50
    ids, tps = pkg.data.fit_samples(model, target, 300, seed=3)
    assert ids.shape == (300,) and ids.dtype == np.int32 and ids.min() >= 0 and ids.max() < model.n_points and tps.shape == (300, 3)
    ref = LF.long_form(model.ref_points, model.cells, 300, 3)
    tgt = LF.long_form(target.points, target.cells, 300, 3, vertex_ids=False)
    assert same(ids, ref["vertex_ids"]) and same(tps, tgt["points"])
    ctx = pkg.IcpContext(model, target, device=0)
    _, _, d2 = ctx.closestPointOnTarget(tps)
    assert np.sqrt(d2).max() <= 1e-9 * np.abs(target.points).max()  # the points lie on the target
    theta0 = pkg.initial_parameters(model)
    theta0[10:] = 0.3 * np.random.default_rng(17).normal(size=model.rank)
    th = np.stack([theta0, theta0])
    got, status = pkg.icp_fits(ctx, th, 2, (1.0, 0.1), pkg.ModelAndTargetSampling, ids, tps, seed=1)
    by_hand, status2 = pkg.icp_fits(ctx, th, 2, (1.0, 0.1), pkg.ModelAndTargetSampling, ref["vertex_ids"].copy(), tgt["points"].copy(), seed=1)
    assert np.all(status == 0) and np.all(status2 == 0) and same(got, by_hand) and not same(got[0], theta0)
    ctx.close()


@pytest.mark.gpu
def test_samples_feed_the_nystrom_models_and_the_variance_ratio(pkg):
    femur, _, _ = pkg.data.load_femur_mesh("femur_reference")
    kernel = pkg.data.femur_kernel(femur)
    smp = pkg.data.surface_samples(femur, 200, seed=1)
    assert smp.status == 0 and smp.vertex_ids.shape == (200,)
    model, info = pkg.nystrom_models([(femur, smp.points, kernel, 30)])[0]
    assert info["status"] == 0 and model is not None
    total = pkg.data.approx_total_variance(femur, kernel, 50000)
    trace = 10.0 * np.trace(kernel[0].A) + 24.0
    assert abs(total - trace) <= 1e-12 * trace
    ratio = info["variance"].sum() / total
    assert 0.0 < ratio < 1.0
    with pytest.raises(ValueError, match="no area"):
        pkg.data.surface_samples(pkg.data.TriangleMesh(femur.points, [[0, 0, 1]]), 5)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    chunk_check()
