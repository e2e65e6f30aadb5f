"""GPU: Gaussian-process shape models by the Nyström approximation (icp_nystrom_models_many) through the public interface — against
the numpy long form (tests/nystrom_model_long_form.py): eigh's spectrum for the eigenvalues, the residuals and the covariance rows, and
the long form run on the DEVICE's own eigenvectors for the basis (inside a cluster of equal eigenvalues — the femur kernel has them in
pairs — every basis is as good as any other, so eigenvectors are never compared with eigh's).

The femur kernel on strided femur reference vertices unless stated.  Every device result of the shapes comes from ONE nystrom_models
call; the long forms are made once per item and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import face_kernel_long_form as FK
import nystrom_model_long_form as NLF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
# (n, k): R = 3n = 3 (one pair), 33 (no multiple of 32), 63 (the last single pair; once with every eigenpair), 66 (two padded blocks),
# 129 (five blocks: the padded bye), 300 (ten blocks, several sweeps).  k = n/2 + 1 as apps/femur/CreateGPModel.scala has it.
SHAPES = [(1, 1), (11, 6), (21, 11), (21, 63), (22, 12), (43, 22), (100, 51)]
GAPPED = [(11, 6), (21, 11), (100, 51)]  # shapes whose spectrum has a gap behind k (asserted where it is used)
BIG = (400, 201)                         # R = 1,200


def femur(pkg):
    return pkg.data.load_femur_mesh("femur_reference")[0]


def strided(pkg, n):
    mesh = femur(pkg)
    return mesh.points[:: mesh.n_points // n][:n]


def mesh_of(pkg, n):
    """the mesh of shape n: the femur reference for n >= 100, else 150 of its vertices (3N = 450: no multiple of 16 or 48)"""
    mesh = femur(pkg)
    return mesh if n >= 100 else pkg.data.TriangleMesh(strided(pkg, 150), np.array([[0, 1, 2]]))


def items_of(pkg, shapes):
    terms = pkg.data.femur_kernel(femur(pkg))
    return [(mesh_of(pkg, n), strided(pkg, n), terms, k) for n, k in shapes]


def make_runs(pkg, shapes):
    items = items_of(pkg, shapes)
    got = pkg.nystrom_models(items, device=0)

    @functools.lru_cache(maxsize=None)
    def long_form(q):
        mesh, smp, terms, k = items[q]
        return NLF.long_form(mesh.points, smp, terms, k)
    return items, got, long_form


@pytest.fixture(scope="module")
def runs(pkg):
    return make_runs(pkg, SHAPES)


@pytest.fixture(scope="module")
def residual_tol(pkg, runs):
    """100 × the worst residual of the long form's eigh vectors over the shapes, relative to λ₁, never looser than 1e-10: eigh is
    backward stable at about R·2⁻⁵², and a Jacobi result may carry a small multiple of that"""
    items, got, long_form = runs
    worst = 0.0
    for q, (n, k) in enumerate(SHAPES):
        lf = long_form(q)
        worst = max(worst, NLF.residual(lf["K"], lf["eigh_values"], lf["eigh_vectors"][:, :k]) / lf["eigh_values"][0])
    return min(100.0 * worst, 1e-10)


def check_spectrum(shape, item, result, lf, tol):
    """eigenvalues, orthogonality, residual and basis of one item; prints every figure in front of its assertion"""
    (n, k), (mesh, smp, terms, _), (model, info) = shape, item, result
    R = 3 * n
    lam, U, w = info["sample_eigenvalues"], info["sample_eigenvectors"], lf["eigh_values"]
    K = lf["K"]
    print(f"n {n} k {k} R {R}: sweeps {info['sweeps']} off-diagonal mass {info['off_diagonal_mass']:.3e} status {info['status']}")
    assert info["status"] == 0 and 1 <= info["sweeps"] <= 40
    assert abs(info["trace"] - np.trace(K)) <= 1e-13 * np.trace(K)
    # 1. eigenvalues: all R
    err = np.abs(lam - w).max()
    print(f"  1. max |lambda - eigh| = {err / w[0]:.3e} lambda_1 (bound 1e-10)")
    assert lam.shape == (R,) and np.all(np.diff(lam) <= 0) and err <= 1e-10 * w[0]
    assert np.array_equal(info["variance"], lam[:k] / n)
    # 2. orthogonality of the k vectors handed out
    orth = np.abs(U.T @ U - np.eye(k)).max()
    print(f"  2. |UtU - I| = {orth:.3e} (bound {1e3 * EPS * w[0] / w[k - 1]:.3e})")
    assert U.shape == (R, k) and orth <= 1e3 * EPS * w[0] / w[k - 1]
    # 3. residual
    res_dev = NLF.residual(K, lam, U) / w[0]
    res_eigh = NLF.residual(K, w, lf["eigh_vectors"][:, :k]) / w[0]
    print(f"  3. max |K u - lambda u| / lambda_1: device {res_dev:.3e}, eigh {res_eigh:.3e} (tol {tol:.3e})")
    assert res_dev <= tol
    # 4. basis, against the long form on the device's own decomposition
    own = NLF.long_form(mesh.points, smp, terms, k, eigenvalues=lam, eigenvectors=U)
    assert info["rank"] == own["k_eff"] == k == model.rank
    berr, bmax = np.abs(model.basis - own["basis"]).max(), np.abs(own["basis"]).max()
    print(f"  4. max |basis - long form on the device's vectors| = {berr / bmax:.3e} max|b| (bound 1e-9)")
    assert model.basis.shape == (3 * mesh.n_points, k) and berr <= 1e-9 * bmax
    assert np.array_equal(model.mean_def, np.zeros_like(model.ref_points)) and np.array_equal(model.variance, lam[:k] / n)


def check_covariance_rows(shape, item, result, lf):
    (n, k), (mesh, smp, terms, _), (model, info) = shape, item, result
    w = lf["eigh_values"]
    gap = (w[k - 1] - w[k]) / w[k - 1]
    print(f"n {n} k {k}: lambda_k {w[k - 1]:.6g} lambda_k+1 {w[k]:.6g} gap {gap:.3e}")
    assert gap >= 1e-3
    rows = np.arange(0, 3 * mesh.n_points, 97 if mesh.n_points > 1000 else 7)
    cov = (model.basis[rows] * model.variance) @ model.basis.T
    want = (lf["basis"][rows] * lf["variance"]) @ lf["basis"].T
    err = np.abs(cov - want).max()
    print(f"  covariance rows: max |device - eigh-based| = {err / np.abs(lf['K']).max():.3e} max|K| (bound 1e-9)")
    assert err <= 1e-9 * np.abs(lf["K"]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("q", range(len(SHAPES)), ids=[f"n{n}-k{k}" for n, k in SHAPES])
def test_model_against_the_long_form(pkg, runs, residual_tol, q):
    items, got, long_form = runs
    check_spectrum(SHAPES[q], items[q], got[q], long_form(q), residual_tol)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GAPPED, ids=[f"n{n}-k{k}" for n, k in GAPPED])
def test_covariance_rows_where_the_spectrum_has_a_gap(pkg, runs, shape):
    items, got, long_form = runs
    q = SHAPES.index(shape)
    check_covariance_rows(shape, items[q], got[q], long_form(q))


@pytest.mark.gpu
def test_twelve_hundred_rows(pkg, residual_tol):
    """R = 1,200, k = 201: 38 blocks"""
    items, got, long_form = make_runs(pkg, [BIG])
    check_spectrum(BIG, items[0], got[0], long_form(0), residual_tol)
    check_covariance_rows(BIG, items[0], got[0], long_form(0))


@pytest.mark.gpu
def test_duplicated_samples_and_the_effective_rank(pkg):
    """40 sample points and 7 of them again, k = R = 141: 21 eigenvalues at rounding level, some negative, do not count; with
    min_variance = 0 the count is that of λ_i/n >= 0 on the device's own eigenvalues"""
    mesh = mesh_of(pkg, 40)
    s = strided(pkg, 40)
    smp = np.concatenate([s, s[:7]])
    terms = pkg.data.femur_kernel(femur(pkg))
    (model, info), (model0, info0) = pkg.nystrom_models([(mesh, smp, terms, 141)] * 2, min_variance=[1e-8, 0.0], device=0)
    lf = NLF.long_form(mesh.points, smp, terms, 141)
    lam, w = info["sample_eigenvalues"], lf["eigh_values"]
    print(f"k_eff {info['rank']} (min_variance 0: {info0['rank']}); tail in [{lam[120:].min():.3e}, {lam[120:].max():.3e}]; sweeps {info['sweeps']}")
    assert info["status"] == 0 and info0["status"] == 0 and lf["k_eff"] == 120
    assert info["rank"] == 120 == model.rank and np.abs(lam - w).max() <= 1e-10 * w[0]
    assert np.abs(lam[120:]).max() <= 141 * EPS * w[0] * 10
    for a in (model.basis, model.variance, lam, info["sample_eigenvectors"], info["variance"]):
        assert np.all(np.isfinite(a))
    assert np.array_equal(info0["sample_eigenvalues"], lam)
    assert info0["rank"] == int(np.sum(lam[:141] / 47 >= 0.0)) == model0.rank and 120 <= info0["rank"] <= 141
    own = NLF.long_form(mesh.points, smp, terms, 141, eigenvalues=lam, eigenvectors=info["sample_eigenvectors"])
    assert np.abs(model.basis - own["basis"]).max() <= 1e-9 * np.abs(own["basis"]).max()


@pytest.mark.gpu
def test_general_terms(pkg):
    """the face kernel — B-spline terms, region weights, the mirror — on a 14 × 14 patch (N = 196) with 30 sample points on its surface;
    the weights of both sides are made in numpy from the same regions"""
    pts = FK.patch(14, 0.5)
    mesh = pkg.data.TriangleMesh(pts, FK.grid_cells(14))
    level_mask = FK.masks(pts)["part"]
    terms = FK.face_terms(pkg.data.BSplineKernelTerm, pts, level_mask)
    smp = pkg.data.uniform_mesh_samples(mesh, 30, seed=4)
    sw = [FK.region_weights(smp, pts[level_mask >= level]) for level, _ in FK.FACE_LEVELS]
    k = 20
    model, info = pkg.nystrom_model(mesh, smp, terms, k, sw, device=0)
    lf = NLF.long_form(pts, smp, terms, k, sample_weights=sw)
    lam, U, w = info["sample_eigenvalues"], info["sample_eigenvectors"], lf["eigh_values"]
    print(f"face kernel: sweeps {info['sweeps']} k_eff {info['rank']}; max |lambda - eigh| = {np.abs(lam - w).max() / w[0]:.3e} lambda_1")
    assert info["status"] == 0 and np.abs(lam - w).max() <= 1e-10 * w[0]
    assert np.abs(U.T @ U - np.eye(k)).max() <= 1e3 * EPS * w[0] / w[k - 1]
    own = NLF.long_form(pts, smp, terms, k, sample_weights=sw, eigenvalues=lam, eigenvectors=U)
    assert info["rank"] == own["k_eff"] == model.rank and own["k_eff"] >= 1
    berr = np.abs(model.basis - own["basis"]).max()
    print(f"  max |basis - long form on the device's vectors| = {berr / np.abs(own['basis']).max():.3e} max|b| (bound 1e-9)")
    assert berr <= 1e-9 * np.abs(own["basis"]).max()


@pytest.mark.gpu
def test_the_model_registers(pkg, runs):
    """a model built at (100, 51) is a model like the fixtures, whose bases are not orthonormal either: a context takes it, projection
    inverts its instances at tests/test_gpu_model_projection.py's bound against the regularised solve, a 3-iteration fit runs"""
    items, got, _ = runs
    model, info = got[SHAPES.index((100, 51))]
    assert model.rank == 51
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
        print(f"round trip {s}: |c' - long form| {np.abs(back - want).max():.3e} (bound {bound:.3e})")
        assert np.abs(back - want).max() <= bound
    ids_ = rng.integers(0, model.n_points, 300).astype(np.int32)
    tps = target.points[rng.integers(0, target.n_points, 300)]
    th0 = pkg.initial_parameters(model)[None, :]
    fit, status = pkg.icp_fits(ctx, th0, 3, (1.0, 0.1, 0.01), pkg.ModelSampling, ids_, tps)
    assert np.all(status == 0) and np.all(np.isfinite(fit)) and np.abs(fit[0, 10:]).max() > 0
    ctx.close()


@pytest.mark.gpu
def test_a_bad_item_fails_alone(pkg, runs):
    """R > 2,400, rank > 256, rank > R, a non-finite sample, a negative min_variance, past the Python-side checks (NLF.native_call):
    ICP_ERR_INVALID_ARG for that item, nothing of it written, and its neighbours in the call are built — to the bits of the shapes' call"""
    items, got, _ = runs
    q = SHAPES.index((22, 12))
    mesh, smp, terms, k = items[q]
    good = (mesh.points, smp, terms, k)
    nan = smp.copy()
    nan[3, 0] = np.nan
    bad = [(mesh.points, np.zeros((801, 3)), terms, 5), (mesh.points, strided(pkg, 100), terms, 257), (mesh.points, smp, terms, 67),
           (mesh.points, nan, terms, 5), good]
    call = [good]
    for b in bad:
        call += [b, good]
    mv = [1e-8] * len(call)
    mv[-2] = -1e-8
    rc, status, outs = NLF.native_call(pkg, call, min_variance=mv)
    assert rc == -1 and status.tolist() == [0, -1] * 5 + [0]
    for o in outs[::2]:
        assert np.array_equal(o["basis"], got[q][0].basis) and np.array_equal(o["sample_eigenvalues"], got[q][1]["sample_eigenvalues"])
        assert np.array_equal(o["sample_eigenvectors"], got[q][1]["sample_eigenvectors"]) and o["info"][0] == 12
    assert all(np.all(a == 7.0) for o in outs[1::2] for a in o.values())


# ---------------------------------------------------------------- batch independence, as bits (a process with the test-hooks library)

MIXED = [(100, 51), (1, 1), (43, 22), (21, 63), (22, 12), (11, 6)]


def same_bits(a, b):
    (ma, ia), (mb, ib) = a, b
    return (all(np.array_equal(ia[k], ib[k]) for k in ("variance", "sample_eigenvalues", "sample_eigenvectors"))
            and np.array_equal(ma.basis, mb.basis) and all(ia[k] == ib[k] for k in ("rank", "sweeps", "trace", "off_diagonal_mass", "status")))


def chunk_check():
    """one item alone == the same item inside a call of 6 mixed items (different R, k and N) == that call reversed == with the chunk
    buffer forced to about a ninth of the femur basis, and to the smallest one the widest item allows: every output array equal as bits"""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    os.environ.pop("ICP_TEST_NYSTROM_MODELS_CHUNK_DOUBLES", None)
    items = items_of(pkg, MIXED)
    whole = pkg.nystrom_models(items, device=0)
    assert not same_bits(whole[2], whole[4])
    for q in range(len(MIXED)):
        assert same_bits(pkg.nystrom_models([items[q]], device=0)[0], whole[q]), ("alone", q)
    rev = pkg.nystrom_models(items[::-1], device=0)[::-1]
    assert all(same_bits(a, b) for a, b in zip(whole, rev)), "reversed"
    for doubles in (4866 * 51 // 9, 48 * 63):
        os.environ["ICP_TEST_NYSTROM_MODELS_CHUNK_DOUBLES"] = str(doubles)
        small = pkg.nystrom_models(items, device=0)
        assert all(same_bits(a, b) for a, b in zip(whole, small)), doubles
    os.environ.pop("ICP_TEST_NYSTROM_MODELS_CHUNK_DOUBLES", None)
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
