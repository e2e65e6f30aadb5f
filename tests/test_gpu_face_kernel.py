"""GPU: general kernel terms of Gaussian-process shape models (icp_gp_models_general_many, icp_region_weights_many) through
the public interface — against the numpy long form (tests/face_kernel_long_form.py) run on the DEVICE's pivots, as
tests/test_gpu_gp_models.py does and with its bounds: the rows y and z of a vertex tie exactly under the face kernel, so the long
form's own choice of pivots is not the device's.

Every device result of the module's checks against the long form comes from ONE gp_models call (all meshes, kernels and configurations
side by side); the long forms are made once per item and shared."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import face_kernel_long_form as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
CONFIGS = [(1, 1), (2, 2), (5, 5), (64, 64), (65, 65), (200, 200), (256, 256)]
LAT_LEVELS = [F.FACE_LEVELS, ((-2, 4.0),), ((0, 1.0),)]  # the five levels together, level -2 alone, level 0 alone
NOT_FINITE = -3


@functools.lru_cache(maxsize=None)
def points_of(name):
    return {"sym11": lambda: F.patch(11, 0.0), "jit11": lambda: F.patch(11, 1.5), "jit6": lambda: F.patch(6, 1.5), "lat27": F.lat27,
            "one": lambda: F.ONE_POINT.copy()}[name]()


def mesh_of(pkg, name):
    pts = points_of(name)
    g = {"sym11": 11, "jit11": 11, "jit6": 6}.get(name)
    return pkg.data.TriangleMesh(pts, F.grid_cells(g) if g else np.zeros((0, 3), dtype=np.int32))


def kernel_of(pkg, name, kname, weights):
    """kname: 'face-all' / 'face-part' (the weights of 'part' and of jit11's 'all' come from the device, through face_kernel: `weights`
    is that cache), 'lat<i>' (LAT_LEVELS[i] at gain 0.7, no weights), 'gamma1', 'mixed', 'iso', 'e0'"""
    S, G = pkg.data.BSplineKernelTerm, pkg.data.GaussianKernelTerm
    pts = points_of(name)
    if kname.startswith("face-"):
        key = (name, kname)
        if key not in weights:
            mask = None if (kname == "face-all" and name != "jit11") else pkg.data.FaceMask(F.masks(pts)[kname[5:]])
            weights[key] = pkg.face_kernel(mesh_of(pkg, name), mask)
        return weights[key]
    if kname.startswith("lat"):
        return F.face_terms(S, pts, None, 0.7, LAT_LEVELS[int(kname[3:])])
    if kname == "gamma1":
        return F.face_terms(S, pts, None, 1.0)
    if kname == "mixed":  # a Gaussian term with weights, mirrored about y with gain 0.5, plus a plain B-spline term
        w = F.region_weights(pts, pts[pts[:, 1] > 0.0])
        return [G(3.0, 50.0, np.diag([1.0, 2.0, 1.0]), w, 0.5, 1), S(2.0, -5)]
    if kname == "iso":
        return [G(4.0, 60.0)]
    if kname == "e0":     # only the x row, which the mirror at gain 1 cancels on the plane x = 0: trace K = 0
        e0 = np.zeros((3, 3))
        e0[0, 0] = 1.0
        return [S(1.0, -2, e0, None, 1.0, 0)]
    raise KeyError(kname)


# (mesh, kernel, n_pivots, rank); the r < m cases: the gap behind the rank is asserted from the long form
FACE_ITEMS = [(a, "face-" + k, m, r) for a in ("sym11", "jit11") for k in ("all", "part") for m, r in CONFIGS]
FACE_ITEMS += [("jit6", "face-part", m, r) for m, r in ((5, 5), (64, 64), (108, 108))]
FACE_ITEMS += [("jit11", "face-part", 64, 20), ("jit11", "face-all", 200, 90)]
LAT_ITEMS = [("lat27", f"lat{i}", 81, 81) for i in range(len(LAT_LEVELS))]
OTHER_ITEMS = [("lat27", "gamma1", 81, 81), ("jit6", "mixed", 60, 60), ("jit6", "mixed", 40, 13), ("one", "e0", 1, 1), ("jit11", "face-part", 128, 51)]
ITEMS = FACE_ITEMS + LAT_ITEMS + OTHER_ITEMS
CHECKED = FACE_ITEMS + [("jit6", "mixed", 60, 60), ("jit6", "mixed", 40, 13)]


def run_items(pkg, items, weights, want=("variance", "basis", "pivots", "residual")):
    return pkg.gp_models([mesh_of(pkg, i[0]) for i in items], [kernel_of(pkg, i[0], i[1], weights) for i in items], [i[2] for i in items],
                         [i[3] for i in items], 0.0, device=0, want=want)


@pytest.fixture(scope="module")
def runs(pkg):
    weights = {}
    got = run_items(pkg, ITEMS, weights)

    @functools.lru_cache(maxsize=None)
    def long_form(q):
        name, kname, m, r = ITEMS[q]
        return F.long_form(points_of(name), kernel_of(pkg, name, kname, weights), m, r, 0.0, pivots=got[q][1]["pivots"])
    return got, weights, long_form


@pytest.mark.gpu
@pytest.mark.parametrize("item", CHECKED, ids=lambda i: "-".join(str(v) for v in i))
def test_model_against_the_long_form_on_the_devices_pivots(pkg, runs, item):
    got, weights, long_form = runs
    q = ITEMS.index(item)
    name, kname, m, r = item
    model, info = got[q]
    pts = points_of(name)
    terms = kernel_of(pkg, name, kname, weights)
    n, R = pts.shape[0], 3 * pts.shape[0]
    lf = long_form(q)
    piv = info["pivots"]
    dmax = F.kernel_diagonal(pts, terms).max()  # = max |K|: K is positive semi-definite
    print(f"{name}-{kname}-{m}-{r}: m_eff {info['n_pivots']} rank {info['rank']} status {info['status']}")
    # 1. pivot validity: the device's pivot is the largest residual, to 1e-10, at every step; none repeats
    assert info["status"] == 0 and info["n_pivots"] == m == lf["m_eff"] and info["rank"] == r and model.rank == r
    assert len(set(piv.tolist())) == m and piv.min() >= 0 and piv.max() < R
    print(f"  1. min residual(device pivot) / max residual = 1 - {1.0 - (lf['step_taken'] / lf['step_max']).min():.3e}")
    assert np.all(lf["step_taken"] >= (1.0 - 1e-10) * lf["step_max"])
    # 2. variances
    var = info["variance"]
    err = np.abs(var - lf["variance"]).max()
    print(f"  2. max |variance - long form| = {err:.3e} (bound {1e-10 * var[0]:.3e})")
    assert np.all(np.diff(var) <= 0) and var[-1] > 0 and err <= 1e-10 * var[0]
    # 3. orthogonality
    B = model.basis
    orth = np.abs(B.T @ B / n - np.eye(r)).max()
    print(f"  3. |BtB/N - I| = {orth:.3e} (bound {1e3 * EPS * var[0] / var[-1]:.3e}, ratio {var[0] / var[-1]:.3e})")
    assert orth <= 1e3 * EPS * var[0] / var[-1]
    # 4. covariance
    if r < m:
        gap = lf["theta"][r - 1] - lf["theta"][r]
        print(f"  4. gap behind the rank {gap:.3e} = {gap / lf['theta'][0]:.3e} theta_1")
        assert gap >= 1e-6 * lf["theta"][0]
    cov = (B * var) @ B.T
    want = (lf["basis"] * lf["variance"]) @ lf["basis"].T
    cerr = np.abs(cov - want).max()
    print(f"  4. covariance: max |device - long form| = {cerr:.3e} (bound {1e-9 * dmax:.3e})")
    assert cerr <= 1e-9 * dmax
    res = info["residual"]
    if r == m:
        K = F.dense(pts, terms)
        rc = np.maximum(res, 0.0)
        slack = np.abs(K - cov) - np.sqrt(rc[:, None] * rc[None, :])
        print(f"  4. Cauchy-Schwarz with the device's residual: max excess {slack.max():.3e} (bound {1e-9 * dmax:.3e})")
        assert slack.max() <= 1e-9 * dmax
    # 5. trace identity, residual
    assert abs(info["total_variance"] - lf["trace"] / n) <= 2e-14 * info["total_variance"]  # (two summation orders of 3N terms)
    assert abs(info["approximated_variance"] - var.sum()) <= 1e-13 * var.sum()
    rerr = np.abs(res - lf["residual"]).max()
    print(f"  5. residual: min {res.min():.3e} (bound {-m * EPS * dmax:.3e}), max |device - long form| {rerr:.3e}")
    assert res.min() >= -m * EPS * dmax and rerr <= 1e-10 * dmax
    if r == m:
        trace = n * info["total_variance"]
        tid = abs(trace - (n * info["approximated_variance"] + res.sum()))
        print(f"  5. trace identity: {tid / trace:.3e} relative")
        assert tid <= 1e-12 * trace


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(LAT_LEVELS)), ids=lambda i: "levels" + "_".join(str(lv) for lv, _ in LAT_LEVELS[i]))
def test_full_rank_model_is_the_kernel_matrix(pkg, runs, i):
    """lat27 at (81, 81): every coordinate on a lattice node, neighbours exactly two cells apart at level -2, negative coordinates"""
    got, weights, _ = runs
    model, info = got[ITEMS.index(("lat27", f"lat{i}", 81, 81))]
    pts = points_of("lat27")
    K = F.dense(pts, kernel_of(pkg, "lat27", f"lat{i}", weights))
    assert info["status"] == 0 and info["n_pivots"] == 81 and model.rank == 81
    err = np.abs((model.basis * model.variance) @ model.basis.T - K).max()
    print(f"levels {LAT_LEVELS[i]}: max |B diag(var) Bt - K| = {err:.3e} (bound {1e-9 * np.abs(K).max():.3e})")
    assert err <= 1e-9 * np.abs(K).max()


@pytest.mark.gpu
def test_mirror_gain_one_stops_at_the_numerical_rank(pkg, runs):
    got, weights, long_form = runs
    q = ITEMS.index(("lat27", "gamma1", 81, 81))
    model, info = got[q]
    lf = long_form(q)
    d = F.kernel_diagonal(points_of("lat27"), kernel_of(pkg, "lat27", "gamma1", weights))
    print(f"gain 1: m_eff {info['n_pivots']}, zero rows {int((d == 0).sum())}, residual max {info['residual'].max():.3e}")
    assert info["status"] == 0 and info["n_pivots"] == lf["m_eff"] == 45 == info["rank"] == model.rank
    assert np.all(d[info["pivots"]] > 0.0) and int((d == 0.0).sum()) == 9  # no pivot is a zero row
    for a in (info["variance"], info["residual"], model.basis):
        assert np.all(np.isfinite(a))
    assert np.all(info["variance"] > 0) and np.abs(info["variance"] - lf["variance"]).max() <= 1e-10 * info["variance"][0]
    assert np.all(model.basis.reshape(27, 3, 45)[d.reshape(27, 3)[:, 0] == 0.0, 0, :] == 0.0)  # a zero row of K is a zero row of the basis


@pytest.mark.gpu
def test_an_item_without_a_column_fails_alone(pkg, runs):
    got, weights, _ = runs
    model, info = got[ITEMS.index(("one", "e0", 1, 1))]
    assert model is None and info["status"] == NOT_FINITE
    assert (info["n_pivots"], info["rank"], info["total_variance"], info["approximated_variance"]) == (0, 0, 0.0, 0.0)
    assert info["variance"].size == 0 and info["pivots"].size == 0 and np.all(np.isnan(info["residual"]))
    # straight through the ABI: NaN in every output array, info zero, the good item beside it computed
    raw = native_general(pkg, [("one", "e0", 1, 1), ("jit6", "mixed", 40, 13)], weights)
    assert raw["rc"] == NOT_FINITE and raw["status"].tolist() == [NOT_FINITE, 0]
    assert np.all(np.isnan(raw["variance"][0])) and np.all(np.isnan(raw["basis"][0])) and np.all(np.isnan(raw["residual"][0]))
    assert np.array_equal(raw["info"][0], np.zeros(4)) and np.array_equal(raw["pivots"][0], [-1])
    # the good item equals, as bits, the same item alone and the same item in the module's call
    alone = run_items(pkg, [("jit6", "mixed", 40, 13)], weights)[0]
    beside = got[ITEMS.index(("jit6", "mixed", 40, 13))]
    assert same_bits(alone, beside)
    assert np.array_equal(raw["basis"][1], alone[0].basis) and np.array_equal(raw["variance"][1], alone[1]["variance"])
    assert np.array_equal(raw["residual"][1], alone[1]["residual"]) and np.array_equal(raw["pivots"][1], alone[1]["pivots"])


def native_general(pkg, items, weights, restate=None):
    """icp_gp_models_general_many straight through ctypes.  restate: lists of plain Gaussian terms to hand over as kind 0 instead
    of the items' kernels (the public interface would send those through icp_gp_models_many)."""
    nat, L = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    n = len(items)
    pts = [np.ascontiguousarray(m.points) for m in (restate[0] if restate else [mesh_of(pkg, i[0]) for i in items])]
    kernels = restate[1] if restate else [kernel_of(pkg, i[0], i[1], weights) for i in items]
    arrs, keep = [], []
    for kb in kernels:
        arr = (nat.KernelTermGeneral * len(kb))()
        for t, k in enumerate(kb):
            gauss = hasattr(k, "sigma")
            arr[t].struct_size, arr[t].kind = ctypes.sizeof(nat.KernelTermGeneral), 0 if gauss else 1
            arr[t].scale, arr[t].sigma, arr[t].level = k.scale, (k.sigma if gauss else 0.0), (0 if gauss else k.level)
            arr[t].mirror_axis, arr[t].mirror_gain = k.mirror_axis, k.mirror_gain
            arr[t].A[:] = k.A.reshape(-1).tolist()
            if k.weights is not None:
                keep.append(np.ascontiguousarray(k.weights, dtype=np.float64))
                arr[t].weights = keep[-1].ctypes.data_as(dp)
        arrs.append(arr)
    mp, rk = np.array([i[2] for i in items], dtype=np.int32), np.array([i[3] for i in items], dtype=np.int32)
    out = {"variance": [np.zeros(r) for r in rk], "basis": [np.zeros((3 * p.shape[0], r)) for p, r in zip(pts, rk)],
           "pivots": [np.zeros(m, dtype=np.int32) for m in mp], "residual": [np.zeros(3 * p.shape[0]) for p in pts],
           "info": [np.full(4, 7.0) for _ in items]}
    ptrs = lambda arrays, t=dp: (t * n)(*[a.ctypes.data_as(t) for a in arrays])  # noqa: E731
    status = np.full(n, 99, dtype=np.int32)
    n_pts, n_terms = np.array([p.shape[0] for p in pts], dtype=np.int32), np.array([len(a) for a in arrs], dtype=np.int32)
    c_terms = (ctypes.POINTER(nat.KernelTermGeneral) * n)(*[ctypes.cast(a, ctypes.POINTER(nat.KernelTermGeneral)) for a in arrs])
    out["rc"] = L.icp_gp_models_general_many(n, 0, n_pts.ctypes.data_as(ip), ptrs(pts), n_terms.ctypes.data_as(ip), c_terms, mp.ctypes.data_as(ip),
                                             rk.ctypes.data_as(ip), None, ptrs(out["variance"]), ptrs(out["basis"]), ptrs(out["pivots"], ip),
                                             ptrs(out["residual"]), ptrs(out["info"]), status.ctypes.data_as(ip))
    out["status"] = status
    return out


@pytest.mark.gpu
def test_plain_terms_restated_as_general_ones_have_the_old_entry_points_bits(pkg):
    """icp_gp_models_many on the femur reference at (64, 51) and on the seven-vertex mesh at (21, 21) == icp_gp_models_general_many with
    the same terms as kind 0"""
    from test_gpu_gp_models import meshes_of, kernels_of
    ms = meshes_of(pkg)
    meshes, kernels = [ms["femur"], ms["seven"]], [kernels_of(pkg, ms["femur"])["femur"], kernels_of(pkg, ms["seven"])["femur"]]
    items = [("femur", "femur", 64, 51), ("seven", "femur", 21, 21)]
    old = pkg.gp_models(meshes, kernels, [64, 21], [51, 21])
    new = native_general(pkg, items, None, restate=(meshes, kernels))
    assert new["rc"] == 0 and np.all(new["status"] == 0)
    for b, (model, info) in enumerate(old):
        assert "status" not in info  # (the public call went through icp_gp_models_many)
        assert np.array_equal(model.basis, new["basis"][b]) and np.array_equal(info["variance"], new["variance"][b])
        assert np.array_equal(info["pivots"], new["pivots"][b]) and np.array_equal(info["residual"], new["residual"][b])
        assert np.array_equal(new["info"][b], [info["n_pivots"], info["rank"], info["total_variance"], info["approximated_variance"]])


@pytest.mark.gpu
def test_region_weights(pkg):
    """|w_dev - w_numpy| <= 8 * 2^-52 * w: the exponent's argument has the same bits on both sides (the expression's order is
    prescribed, nothing is contracted), each exp is good to about an ulp; 1.0 exactly at region points; an item alone == in a batch"""
    jit11 = points_of("jit11")
    cloud = np.random.default_rng(5).normal(size=(300, 3)) * np.array([70.0, 90.0, 20.0])
    order = np.argsort(-jit11[:, 0], kind="stable")
    items = []
    for pts in (jit11, cloud):
        items += [(pts, jit11[order[:1]]), (pts, jit11[order[:77]]), (pts, cloud), (pts, pts[pts[:, 0] >= -20.0])]
    got = pkg.region_weights([p for p, _ in items], [r for _, r in items], [40.0] * 7 + [25.0])
    for b, (pts, reg) in enumerate(items):
        sd = 40.0 if b < 7 else 25.0
        want = F.region_weights(pts, reg, sd)
        err = np.abs(got[b] - want) / want
        print(f"item {b}: {len(pts)} points, region of {len(reg)}: max relative error {err.max() / EPS:.2f} eps, min w {want.min():.3e}")
        assert got[b].shape == (len(pts),) and np.all(want > 0.0) and err.max() <= 8 * EPS
        at_region = (pts[:, None, :] == reg[None, :, :]).all(axis=2).any(axis=1)
        assert np.all(got[b][at_region] == 1.0) and (b % 4 != 3 or at_region.sum() == len(reg))
        if b in (1, 6):
            assert np.array_equal(pkg.region_weights(pts, reg, sd), got[b])  # alone == in the batch
    mask = pkg.data.FaceMask(F.masks(jit11)["part"])
    assert np.array_equal(mask.smoothed_region_weights(mesh_of(pkg, "jit11"), -3), got[3])
    assert np.array_equal(pkg.face_kernel(mesh_of(pkg, "jit11"), mask)[4].weights, got[3])
    assert np.array_equal(pkg.face_kernel(mesh_of(pkg, "jit11"), mask)[0].weights, np.ones(121))


@pytest.mark.gpu
def test_the_model_registers(pkg, runs):
    """a face-kernel model of jit11 at (128, 51) is a model like the fixtures: a context takes it, projection inverts its instances (the
    bound of tests/test_gpu_model_projection.py against the regularised solve; against c itself the sigma^2 = 1e-5 shrink is allowed for)"""
    got, _, _ = runs
    model, info = got[ITEMS.index(("jit11", "face-part", 128, 51))]
    assert model.rank == 51 and info["n_pivots"] == 128 and np.array_equal(model.mean_def, np.zeros_like(model.ref_points))
    target = pkg.data.TriangleMesh(points_of("jit11") + np.array([1.0, -2.0, 0.5]), F.grid_cells(11))
    ctx = pkg.IcpContext(model, target, device=0)
    rng = np.random.default_rng(3)
    Q = model.basis * np.sqrt(model.variance)[None, :]
    A = Q.T @ Q + 1e-5 * np.eye(51)
    for s in range(3):
        c = np.clip(rng.normal(size=51), -2.5, 2.5)
        theta = pkg.initial_parameters(model)
        theta[10:] = c
        x = ctx.transformedMesh(theta)
        assert np.abs(x - model.instance(c)).max() <= 1e-9
        back = ctx.coefficients(x)
        want = np.linalg.solve(A, Q.T @ (x - model.ref_points).reshape(-1))
        bound = 1e-10 * max(1.0, float(np.abs(want).max()))
        shrink = 1e-5 / (model.n_points * model.variance[-1])
        print(f"round trip {s}: |c' - long form| {np.abs(back - want).max():.3e} (bound {bound:.3e}); |c' - c| {np.abs(back - c).max():.3e} "
              f"(shrink {shrink:.3e})")
        assert np.abs(back - want).max() <= bound
        assert np.abs(back - c).max() <= bound + shrink * np.abs(c).max()
    ctx.close()


# ---------------------------------------------------------------- batch independence, as bits (a process with the test-hooks library)

MIXED = [("jit11", "face-part", 128, 51), ("jit6", "iso", 21, 12), ("lat27", "gamma1", 81, 81), ("jit6", "mixed", 60, 60),
         ("jit11", "iso", 65, 65), ("sym11", "face-all", 64, 64), ("jit6", "face-part", 5, 5)]


def same_bits(a, b):
    (ma, ia), (mb, ib) = a, b
    return (all(np.array_equal(ia[k], ib[k]) for k in ("variance", "pivots", "residual")) and np.array_equal(ma.basis, mb.basis)
            and all(ia[k] == ib[k] for k in ("n_pivots", "rank", "total_variance", "approximated_variance")))


def chunk_check():
    """one item alone == the same item inside a call of 7 mixed plain and general items == that call reversed == with the chunk buffer
    forced to a ninth of the largest basis and to the smallest value the widest item allows: every output array equal as bits"""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    os.environ.pop("ICP_TEST_GP_MODELS_CHUNK_DOUBLES", None)
    weights = {}
    whole = run_items(pkg, MIXED, weights)
    assert not same_bits(whole[1], whole[3])
    for q in range(len(MIXED)):
        assert same_bits(run_items(pkg, [MIXED[q]], weights)[0], whole[q]), ("alone", q)
    rev = run_items(pkg, MIXED[::-1], weights)[::-1]
    assert all(same_bits(a, b) for a, b in zip(whole, rev)), "reversed"
    for doubles in (363 * 51 // 9, 48 * 81):
        os.environ["ICP_TEST_GP_MODELS_CHUNK_DOUBLES"] = str(doubles)
        small = run_items(pkg, MIXED, weights)
        assert all(same_bits(a, b) for a, b in zip(whole, small)), doubles
    os.environ.pop("ICP_TEST_GP_MODELS_CHUNK_DOUBLES", None)
    print("chunk check ok")


@pytest.mark.gpu
def test_an_items_bits_do_not_depend_on_the_batch_or_the_chunk():
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "chunk check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    chunk_check()
