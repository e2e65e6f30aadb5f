"""GPU: Gaussian-process shape models from analytic kernels (icp_gp_models_many) through the public interface — against the numpy
long form (tests/gp_model_long_form.py) run on the DEVICE's pivots.  The pivots themselves are not compared with the long form's own
choice: far-apart points leave exact and 1-ulp ties, and exp differs by an ulp between device and host; what is checked is that every
pivot the device took was, in the long form's arithmetic, the largest residual to 1e-10.

Every device result of the module comes from ONE gp_models call (all meshes, kernels and configurations side by side); the long forms
are made once per item and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gp_model_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
CONFIGS = [(1, 1), (2, 2), (5, 5), (64, 51), (65, 65), (200, 200), (256, 201), (256, 256)]  # every decomposition route, the edge at 200
# 3N = 21 binds.  Rank 12: on all 21 rows the femur kernel's eigenvalues come in exact pairs (its B has the eigenvalue 1 twice), the
# isotropic one's in threes; 12 | 13 is a gap of 5.6e-4 θ₁ and 0.16 θ₁
SMALL_CONFIGS = {"femur": [(1, 1), (2, 2), (5, 5), (21, 12), (21, 21)], "iso": [(1, 1), (2, 2), (5, 5), (21, 12), (21, 21)]}


def meshes_of(pkg):
    """femur reference (3N = 4,866: no multiple of 16 or 48); 7 vertices; 40 vertices that are 20 points twice"""
    femur, _, _ = pkg.data.load_femur_mesh("femur_reference")
    rng = np.random.default_rng(7)
    seven = pkg.data.TriangleMesh(rng.normal(size=(7, 3)) * np.array([80.0, 20.0, 15.0]), np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]]))
    twenty = femur.points[:: femur.n_points // 20][:20]
    dup = pkg.data.TriangleMesh(np.concatenate([twenty, twenty]), np.array([[0, 1, 2], [20, 21, 22]]))
    return {"femur": femur, "seven": seven, "dup": dup}


def kernels_of(pkg, mesh):
    return {"femur": pkg.data.femur_kernel(mesh), "iso": [pkg.data.GaussianKernelTerm(4.0, 60.0)]}


def plan(pkg):
    """the items of the module's one call: (mesh name, kernel name, n_pivots, rank, rel_tolerance)"""
    items = [("femur", k, m, r, 0.0) for k in ("femur", "iso") for m, r in CONFIGS]
    items += [("seven", k, m, r, 0.0) for k in ("femur", "iso") for m, r in SMALL_CONFIGS[k]]
    items += [("femur", "femur", 256, 5, 0.2), ("femur", "femur", 256, 5, 0.1), ("dup", "femur", 120, 120, 0.0), ("dup", "iso", 120, 120, 0.0),
              ("femur", "femur", 128, 51, 0.0)]
    return items


def run_items(pkg, items, want=("variance", "basis", "pivots", "residual")):
    ms = meshes_of(pkg)
    return pkg.gp_models([ms[i[0]] for i in items], [kernels_of(pkg, ms[i[0]])[i[1]] for i in items], [i[2] for i in items],
                         [i[3] for i in items], [i[4] for i in items], device=0, want=want)


@pytest.fixture(scope="module")
def runs(pkg):
    items = plan(pkg)
    got = run_items(pkg, items)
    ms = meshes_of(pkg)

    @functools.lru_cache(maxsize=None)
    def long_form(q):
        name, kname, m, r, tol = items[q]
        return LF.long_form(ms[name].points, kernels_of(pkg, ms[name])[kname], m, r, tol, pivots=got[q][1]["pivots"])
    return items, got, ms, long_form


def ids(pkg_items):
    return [f"{a}-{k}-{m}-{r}" + (f"-tol{t}" if t else "") for a, k, m, r, t in pkg_items]


N_PLAIN = 2 * len(CONFIGS) + sum(len(v) for v in SMALL_CONFIGS.values())  # the items without a tolerance, femur and seven


@pytest.mark.gpu
@pytest.mark.parametrize("q", range(N_PLAIN))
def test_model_against_the_long_form_on_the_devices_pivots(pkg, runs, q):
    items, got, ms, long_form = runs
    name, kname, m, r, _ = items[q]
    model, info = got[q]
    mesh = ms[name]
    terms = kernels_of(pkg, mesh)[kname]
    n, R = mesh.n_points, 3 * mesh.n_points
    lf = long_form(q)
    piv = info["pivots"]
    dmax = LF.kernel_diagonal(n, terms).max()  # = max |K|: K is positive semi-definite
    print(f"{ids([items[q]])[0]}: m_eff {info['n_pivots']} rank {info['rank']}")
    # 1. pivot validity: the device's pivot is the largest residual, to 1e-10, at every step; none repeats
    assert info["n_pivots"] == m == lf["m_eff"] and info["rank"] == r and model.rank == r
    assert len(set(piv.tolist())) == m and piv.min() >= 0 and piv.max() < R
    worst = (lf["step_taken"] / lf["step_max"]).min()
    print(f"  1. min residual(device pivot) / max residual = 1 - {1.0 - worst:.3e}; own choice differs at "
          f"{int((LF.long_form(mesh.points, terms, m)['pivots'] != piv).sum()) if m <= 65 else -1} steps")
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
    # 4. covariance rows
    rows = np.arange(0, R, 97) if name == "femur" else np.arange(R)
    if r < m:
        gap = lf["theta"][r - 1] - lf["theta"][r]
        print(f"  4. gap behind the rank {gap:.3e} = {gap / lf['theta'][0]:.3e} theta_1")
        assert gap >= 1e-6 * lf["theta"][0]
    cov = (B[rows] * var) @ B.T
    want = (lf["basis"][rows] * lf["variance"]) @ lf["basis"].T
    cerr = np.abs(cov - want).max()
    print(f"  4. covariance rows: max |device - long form| = {cerr:.3e} (bound {1e-9 * dmax:.3e})")
    assert cerr <= 1e-9 * dmax
    res = info["residual"]
    if r == m:
        Kr = LF.kernel_columns(mesh.points, terms, rows).T
        rc = np.maximum(res, 0.0)
        slack = np.abs(Kr - cov) - np.sqrt(rc[rows][:, None] * rc[None, :])
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
@pytest.mark.parametrize("tol", [0.2, 0.1])
def test_stopping_at_a_tolerance(pkg, runs, tol):
    """m_eff equals the long form's on the device's pivots: in the long form Σd misses tol·trace(K) by more than 1e-6 relative on both
    sides of the deciding step (asserted), so rounding cannot move the stop"""
    items, got, ms, long_form = runs
    q = items.index(("femur", "femur", 256, 5, tol))
    model, info = got[q]
    lf = long_form(q)
    me = info["n_pivots"]
    print(f"tol {tol}: m_eff {me}; sum d in front of the last step {lf['step_sum'][-1] / lf['trace']:.6f}, behind it {lf['sum_after'] / lf['trace']:.6f}")
    assert 1 <= me < 256 and len(info["pivots"]) == me and lf["m_eff"] == me
    assert np.all(lf["step_sum"] > tol * lf["trace"] * (1.0 + 1e-6)) and lf["sum_after"] < tol * lf["trace"] * (1.0 - 1e-6)
    assert np.all(lf["step_taken"] >= (1.0 - 1e-10) * lf["step_max"])
    assert info["rank"] == 5 and model.rank == 5 and np.abs(info["variance"] - lf["variance"]).max() <= 1e-10 * info["variance"][0]
    assert abs(info["residual"].sum() - lf["sum_after"]) <= 1e-10 * lf["trace"]


@pytest.mark.gpu
@pytest.mark.parametrize("kname", ["femur", "iso"])
def test_duplicated_vertices_stop_at_the_numerical_rank(pkg, runs, kname):
    items, got, ms, long_form = runs
    q = items.index(("dup", kname, 120, 120, 0.0))
    model, info = got[q]
    lf = long_form(q)
    me = info["n_pivots"]
    print(f"dup-{kname}: m_eff {me}, residual in [{info['residual'].min():.3e}, {info['residual'].max():.3e}]")
    assert 1 <= me <= 60 and info["rank"] == me == model.rank == lf["m_eff"]
    assert len(set((info["pivots"] % 60).tolist())) == me  # (rows 3v + c and 60 + 3v + c: never a vertex and its copy)
    for a in (info["variance"], info["residual"], model.basis):
        assert np.all(np.isfinite(a))
    assert np.all(info["variance"] > 0) and np.abs(info["variance"] - lf["variance"]).max() <= 1e-10 * info["variance"][0]
    # in the long form the loop, left to itself, would have stopped at the same step
    dmax = LF.kernel_diagonal(40, kernels_of(pkg, ms["dup"])[kname]).max()
    assert lf["residual"].max() <= 120 * EPS * dmax and np.all(lf["step_max"] > 120 * EPS * dmax)
    B, n = model.basis, 40
    assert np.abs(B.T @ B / n - np.eye(me)).max() <= 1e3 * EPS * info["variance"][0] / info["variance"][-1]


@pytest.mark.gpu
def test_the_model_registers(pkg, runs):
    """a model built at (128, 51) is a model like the fixtures: a context takes it, projection inverts its instances (the bound of
    tests/test_gpu_model_projection.py against the regularised solve; against c itself the σ² = 1e-5 shrink is allowed for), a fit runs"""
    items, got, ms, _ = runs
    model, info = got[items.index(("femur", "femur", 128, 51, 0.0))]
    assert model.rank == 51 and info["n_pivots"] == 128 and np.array_equal(model.mean_def, np.zeros_like(model.ref_points))
    _, target = pkg.data.load_femur_model_and_target(50)
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
    ids_ = rng.integers(0, model.n_points, 300).astype(np.int32)
    tps = target.points[rng.integers(0, target.n_points, 300)]
    th0 = pkg.initial_parameters(model)[None, :]
    fit, status = pkg.icp_fits(ctx, th0, 3, (1.0, 0.1, 0.01), pkg.ModelSampling, ids_, tps)
    assert np.all(status == 0) and np.all(np.isfinite(fit)) and np.abs(fit[0, 10:]).max() > 0
    ctx.close()


# ---------------------------------------------------------------- batch independence, as bits (a process with the test-hooks library)

MIXED = [("femur", "femur", 128, 51, 0.0), ("seven", "iso", 21, 12, 0.0), ("femur", "iso", 65, 65, 0.0), ("dup", "femur", 120, 120, 0.0),
         ("femur", "femur", 64, 51, 0.0), ("seven", "femur", 5, 5, 0.0)]


def same_bits(a, b):
    (ma, ia), (mb, ib) = a, b
    return (all(np.array_equal(ia[k], ib[k]) for k in ("variance", "pivots", "residual")) and np.array_equal(ma.basis, mb.basis)
            and all(ia[k] == ib[k] for k in ("n_pivots", "rank", "total_variance", "approximated_variance")))


def chunk_check():
    """one item alone == the same item inside a call of 6 mixed items == that call reversed == with the chunk buffer forced to about a
    ninth of the femur basis (several rounds per item, rounds that hold several items): every output array equal as bits"""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    os.environ.pop("ICP_TEST_GP_MODELS_CHUNK_DOUBLES", None)
    whole = run_items(pkg, MIXED)
    assert not same_bits(whole[0], whole[4])
    for q in range(len(MIXED)):
        assert same_bits(run_items(pkg, [MIXED[q]])[0], whole[q]), ("alone", q)
    rev = run_items(pkg, MIXED[::-1])[::-1]
    assert all(same_bits(a, b) for a, b in zip(whole, rev)), "reversed"
    for doubles in (4866 * 51 // 9, 48 * 120):  # a ninth of the femur basis; the smallest buffer the widest item allows
        os.environ["ICP_TEST_GP_MODELS_CHUNK_DOUBLES"] = str(doubles)
        small = run_items(pkg, MIXED)
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
