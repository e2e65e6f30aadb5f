"""GPU: the two-sided block Jacobi iteration of icp_nystrom_models_many (kernels_nystrom_model.hip) on designed spectra and
at the edges of its block counts (tests/nystrom_designed_spectra.py; tests/test_nystrom_designed_spectra_cpu.py asserts that the cases
are what their table says).  Every designed case goes through ONE nystrom_models call, the count ladder through a second one; the long
forms (tests/nystrom_model_long_form.py) are made once per case and shared.

Tolerances.  Every figure is printed in front of its assertion.  The standing bounds of tests/test_gpu_nystrom_models.py are kept: 1e-10·λ₁
for eigenvalues, 1e-9·max|b| for the basis, 1e-13 for the trace.  Residual, orthogonality and reconstruction follow that file's residual_tol
rule PER CASE: 100 × the figure numpy's eigh gives for the same matrix, relative to λ₁, never looser than 1e-10 — measured against the
reference, never against the device (on `diagonal` eigh is exact, and so must the device be).  Eigenvectors are never compared with
eigh's: inside a cluster every basis is as good as any other.

The basis at min_variance = 0.  Column i is k(X, S)·u_i·√n/λ_i.  Where λ_i is at rounding level (graded_*, rank_one_A) the product
k(X, S)·u_i is all cancellation and the column is not determined to 1e-9·max|b| by ANY summation order — numpy's own in another order
differs by 0.3·max|b| (asserted in the CPU test).  So the standing bound holds the columns with λ_i >= 1e-9·λ₁, with max|b| over those — all the
columns of every case without such a tail, and all that the second items with min_variance = 1e-8 hand out (asserted; the figure is
2.7e-10 at the worst there, on graded_a_43) —, and the columns behind them are held entry by entry to the forward error of the two products being compared:
|Δ| <= 4·(R + 8)·2⁻⁵²·(|k(X, S)|·|u_i|)·√n/|λ_i| (two sums of R terms, γ_R each, and the evaluations of exp on both sides, doubled)."""
import functools
import time

import numpy as np
import pytest

import nystrom_designed_spectra as DS
import nystrom_model_long_form as NLF
import test_gpu_nystrom_models as TN

EPS = DS.EPS
NAMES = ["diagonal", "near_diagonal_a", "near_diagonal_b", "circulant", "graded_a", "graded_b", "twins_coupled", "twins_below_threshold",
         "twins_exact", "twins_blocked", "rank_one_A", "scaled_one", "scaled_down", "scaled_up", "permuted", "near_diagonal_b_43",
         "graded_a_43", "twins_coupled_43"]
FLOORED = [name + "+floor" for name in DS.VARIANCE_FLOOR_CASES]  # the same case again with min_variance = 1e-8
LADDER = DS.ladder()
AT_THE_ROW_LIMIT = (DS.MAX_ROWS // 3, DS.MAX_RANK)  # R = 2,400: 75 blocks, an odd count: padded to 76 by one whole block
PAST_TWELVE_HUNDRED = (401, 201)                    # R = 1,203: 38 blocks as 1,200 has, the last one with 19 rows instead of 16


LEAD = 1e-9  # the standing basis bound holds the columns with λ_i >= LEAD·λ₁ (the module's docstring)


def tol_of(figure):
    """the residual_tol rule: 100 × eigh's own figure (relative to λ₁), never looser than 1e-10"""
    return min(100.0 * figure, 1e-10)


@pytest.fixture(scope="module")
def designed(pkg):
    cases = DS.cases(pkg.data.GaussianKernelTerm)
    assert list(cases) == NAMES
    keys = NAMES + FLOORED
    items, mv = [], []
    for key in keys:
        pts, smp, terms, k, _ = cases[key.split("+")[0]]
        items.append((pkg.data.TriangleMesh(pts, np.array([[0, 1, 2]])), smp, terms, k))
        mv.append(1e-8 if key.endswith("+floor") else 0.0)
    t0 = time.perf_counter()
    got = pkg.nystrom_models(items, min_variance=mv, device=0)
    print(f"{len(items)} designed items in one call: {time.perf_counter() - t0:.3f} s")

    @functools.lru_cache(maxsize=None)
    def long_form(name):
        pts, smp, terms, k, _ = cases[name]
        return NLF.long_form(pts, smp, terms, k, min_variance=0.0)
    return cases, dict(zip(keys, zip(items, mv, got))), long_form


def check_decomposition(label, K, w, v, k, info, closed=None):
    """status, sweeps, trace, eigenvalues, residual of the k vectors handed out and, where k = R, orthogonality and reconstruction over
    all R vectors; w, v: eigh's"""
    lam, U = info["sample_eigenvalues"], info["sample_eigenvectors"]
    R = K.shape[0]
    print(f"{label}: R {R} k {k} sweeps {info['sweeps']} off-diagonal mass {info['off_diagonal_mass']:.3e} status {info['status']}")
    assert info["status"] == 0 and 1 <= info["sweeps"] <= DS.MAX_SWEEPS
    assert abs(info["trace"] - np.trace(K)) <= 1e-13 * np.trace(K)
    err = np.abs(lam - w).max() / w[0]
    print(f"  max |lambda - eigh| = {err:.3e} lambda_1 (bound 1e-10)")
    assert lam.shape == (R,) and U.shape == (R, k) and np.all(np.diff(lam) <= 0) and err <= 1e-10
    if closed is not None:
        cerr, eerr = np.abs(lam - closed).max() / w[0], np.abs(w - closed).max() / w[0]
        print(f"  max |lambda - closed form| = {cerr:.3e} lambda_1 (eigh {eerr:.3e}; bound 1e-10)")
        assert cerr <= 1e-10
    res, res_eigh = NLF.residual(K, lam, U) / w[0], NLF.residual(K, w, v[:, :k]) / w[0]
    print(f"  max |K u - lambda u| / lambda_1: device {res:.3e}, eigh {res_eigh:.3e} (tol {tol_of(res_eigh):.3e})")
    assert res <= tol_of(res_eigh)
    if k < R:
        return
    orth, orth_eigh = np.abs(U.T @ U - np.eye(R)).max(), np.abs(v.T @ v - np.eye(R)).max()
    print(f"  |UtU - I| over all {R}: device {orth:.3e}, eigh {orth_eigh:.3e} (tol {tol_of(orth_eigh):.3e})")
    assert orth <= tol_of(orth_eigh)
    rec, rec_eigh = np.abs((U * lam) @ U.T - K).max() / w[0], np.abs((v * w) @ v.T - K).max() / w[0]
    print(f"  max |U diag(lambda) Ut - K| / lambda_1: device {rec:.3e}, eigh {rec_eigh:.3e} (tol {tol_of(rec_eigh):.3e})")
    assert rec <= tol_of(rec_eigh)


def check_basis(item, mv, result, lf):
    """check_spectrum's step 4 against the long form on the device's own eigenpairs, k_eff counted on the device's own eigenvalues; the
    columns of rounding-level eigenvalues as the module's docstring says"""
    (mesh, smp, terms, k), (model, info) = item, result
    n, R = len(smp), 3 * len(smp)
    lam, U = info["sample_eigenvalues"], info["sample_eigenvectors"]
    own = NLF.long_form(mesh.points, smp, terms, k, min_variance=mv, eigenvalues=lam, eigenvectors=U)
    ke = own["k_eff"]
    kept = int(np.sum(lam[:ke] >= LEAD * lam[0]))
    print(f"  k_eff {info['rank']} (long form on the device's eigenvalues {ke}; {kept} with lambda >= {LEAD:g} lambda_1; min_variance {mv:g})")
    assert info["rank"] == ke == model.rank and 1 <= kept <= ke <= k
    assert kept == ke or (mv == 0.0 and lam[-1] < R * EPS * lam[0])  # every column handed out, but for rounding-level tails at no floor
    assert np.array_equal(info["variance"], lam[:k] / n) and np.array_equal(model.variance, lam[:ke] / n)
    assert model.basis.shape == (3 * mesh.n_points, ke) and np.array_equal(model.mean_def, np.zeros_like(model.ref_points))
    for a in (model.basis, model.variance, lam, U, info["variance"]):
        assert np.all(np.isfinite(a))
    err = np.abs(model.basis - own["basis"])
    bmax = np.abs(own["basis"][:, :kept]).max()
    print(f"  max |basis - long form on the device's vectors| = {err[:, :kept].max() / bmax:.3e} max|b| over {kept} columns (bound 1e-9)")
    assert err[:, :kept].max() <= 1e-9 * bmax
    if kept < ke:
        # (with A diagonal an eigenvector lives on one coordinate, and the rows of the others are exactly zero on both sides)
        fwd = 4 * (R + 8) * EPS * (np.abs(lf["Kxs"]) @ (np.abs(U[:, kept:ke]) * (np.sqrt(float(n)) / np.abs(lam[kept:ke]))[None, :]))
        tail = err[:, kept:ke]
        worst = (tail[fwd > 0.0] / fwd[fwd > 0.0]).max()
        print(f"  the {ke - kept} columns behind them: max |difference| / forward error bound = {worst:.3e} (bound 1); "
              f"their difference is {tail.max() / bmax:.3e} max|b|")
        assert np.all(tail <= fwd)


@pytest.mark.gpu
@pytest.mark.parametrize("key", NAMES + FLOORED)
def test_designed_case(designed, key):
    cases, runs, long_form = designed
    name = key.split("+")[0]
    item, mv, result = runs[key]
    lf, facts = long_form(name), cases[name][4]
    closed = DS.ring_spectrum(*facts["ring"]) if "ring" in facts else None
    check_decomposition(key, lf["K"], lf["eigh_values"], lf["eigh_vectors"], item[3], result[1], closed)
    check_basis(item, mv, result, lf)
    if mv > 0.0:
        # the floor changes what is handed out and nothing else
        base = runs[name][2][1]
        assert np.array_equal(result[1]["sample_eigenvalues"], base["sample_eigenvalues"]) and result[1]["sweeps"] == base["sweeps"]
        assert np.array_equal(result[1]["sample_eigenvectors"], base["sample_eigenvectors"]) and result[1]["rank"] < base["rank"]


@pytest.mark.gpu
def test_diagonal_is_left_alone(designed):
    """An exactly diagonal K: eigenvalues equal as bits to the sorted diagonal, the eigenvectors a signed permutation of exact zeros and
    ones in the sort's order (descending, ties to the lower index), no mass at all, and `sweeps` at the smallest value the host loop of
    abi_nystrom_models.inl can report: 1 — its first pass always runs the rounds and k_nys_sweep_end, which counts the sweep (state[1])
    before it tests the mass, and the loop leaves as soon as no item iterates."""
    cases, runs, long_form = designed
    info = runs["diagonal"][2][1]
    K = long_form("diagonal")["K"]
    lam, U = info["sample_eigenvalues"], info["sample_eigenvectors"]
    d = np.diag(K)
    order = np.argsort(-d, kind="stable")
    print(f"diagonal: sweeps {info['sweeps']} mass {info['off_diagonal_mass']} distinct entries of U {np.unique(U).tolist()}")
    assert np.array_equal(lam.view(np.uint64), d[order].view(np.uint64))
    assert np.array_equal(np.abs(U), (np.arange(96)[:, None] == order[None, :]).astype(np.float64))
    assert np.all((U != 0.0).sum(axis=0) == 1) and np.all((U != 0.0).sum(axis=1) == 1) and set(np.unique(np.abs(U)).tolist()) == {0.0, 1.0}
    assert info["off_diagonal_mass"] == 0.0 and info["sweeps"] == 1 and info["status"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["twins_exact", "twins_blocked", "twins_below_threshold"])
def test_twins_meet(designed, name):
    """two decoupled copies of one spectrum, in the same blocks or in different ones, and with a coupling below the rotation threshold,
    which must not show in any figure: with A = I every eigenvalue of the 16-point Gram matrix comes six times"""
    cases, runs, long_form = designed
    lam, other = runs[name][2][1]["sample_eigenvalues"], runs["twins_exact"][2][1]["sample_eigenvalues"]
    spread = (lam.reshape(16, 6).max(axis=1) - lam.reshape(16, 6).min(axis=1)).max() / lam[0]
    apart = np.abs(lam - other).max() / lam[0]
    print(f"{name}: an eigenvalue and its twins within {spread:.3e} lambda_1; against twins_exact {apart:.3e} lambda_1 (bounds 1e-10); "
          f"sweeps {runs[name][2][1]['sweeps']} (twins_exact {runs['twins_exact'][2][1]['sweeps']})")
    assert spread <= 1e-10 and apart <= 1e-10


@pytest.mark.gpu
def test_another_assignment_of_rows_to_blocks(designed):
    cases, runs, long_form = designed
    a, b = runs["permuted"][2][1]["sample_eigenvalues"], runs["circulant"][2][1]["sample_eigenvalues"]
    print(f"permuted against circulant: {np.abs(a - b).max() / b[0]:.3e} lambda_1 (bound 1e-10)")
    assert np.abs(a - b).max() <= 1e-10 * b[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name, e", [("scaled_down", -40), ("scaled_up", 40)])
def test_scaling_by_a_power_of_two_is_exact(designed, name, e):
    """Every entry of K, both thresholds (2⁻⁵⁴·‖K‖_F and (R·2⁻⁵²·‖K‖_F)²) and every product scale by an exact power of two: eigenvectors and
    basis equal as bits, eigenvalues and variances equal as bits after the scaling, the same sweeps.  A quantity that is absolute where it
    should be relative to ‖K‖_F shows here."""
    cases, runs, long_form = designed
    (m1, i1), (m2, i2) = runs["scaled_one"][2], runs[name][2]
    f = 2.0 ** e
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)  # noqa: E731
    print(f"{name}: sweeps {i2['sweeps']} (scale 1: {i1['sweeps']}); rank {i2['rank']} ({i1['rank']}); "
          f"max |lambda 2^{-e} - lambda at scale 1| = {np.abs(i2['sample_eigenvalues'] / f - i1['sample_eigenvalues']).max():.3e}; "
          f"max |U - U at scale 1| = {np.abs(i2['sample_eigenvectors'] - i1['sample_eigenvectors']).max():.3e}")
    assert i1["sweeps"] == i2["sweeps"] and i1["rank"] == i2["rank"] == 48 and i1["status"] == i2["status"] == 0
    assert np.array_equal(bits(i2["sample_eigenvectors"]), bits(i1["sample_eigenvectors"]))
    assert np.array_equal(bits(i2["sample_eigenvalues"]), bits(i1["sample_eigenvalues"] * f))
    assert np.array_equal(bits(i2["variance"]), bits(i1["variance"] * f)) and np.array_equal(bits(m2.variance), bits(m1.variance * f))
    assert np.array_equal(bits(m2.basis), bits(m1.basis))
    assert i2["trace"] == i1["trace"] * f and i2["off_diagonal_mass"] == i1["off_diagonal_mass"] * f * f


# ---------------------------------------------------------------- the count ladder: the femur kernel on strided femur vertices


@pytest.fixture(scope="module")
def ladder_runs(pkg):
    items, got, long_form = TN.make_runs(pkg, LADDER)
    worst = 0.0
    for q, (n, k) in enumerate(LADDER):
        lf = long_form(q)
        worst = max(worst, NLF.residual(lf["K"], lf["eigh_values"], lf["eigh_vectors"][:, :k]) / lf["eigh_values"][0])
    return items, got, long_form, tol_of(worst)


@pytest.mark.gpu
@pytest.mark.parametrize("q", range(len(LADDER)), ids=[f"n{n}-k{k}" for n, k in LADDER])
def test_ladder_shape(ladder_runs, q):
    """both sides of three, four and six blocks and of kNysMaxRank, and the exact multiples R = 96 (one whole padded block) and 192 (no
    padding at all): check_spectrum of tests/test_gpu_nystrom_models.py, and its covariance rows where the spectrum has a gap behind k"""
    items, got, long_form, tol = ladder_runs
    n, k = LADDER[q]
    blocks = -(-3 * n // DS.BLOCK)
    print(f"R {3 * n}: {blocks} blocks, padded to {blocks + blocks % 2}")
    TN.check_spectrum(LADDER[q], items[q], got[q], long_form(q), tol)
    w = long_form(q)["eigh_values"]
    if k < 3 * n and (w[k - 1] - w[k]) / w[k - 1] >= 1e-3:
        TN.check_covariance_rows(LADDER[q], items[q], got[q], long_form(q))
    else:
        print(f"n {n} k {k}: no gap behind k, the covariance rows are not compared")


# ---------------------------------------------------------------- the limits


def run_at_scale(pkg, shape):
    """eigenvalues, residual and status only: a small mesh, no basis asked for"""
    n, k = shape
    mesh, smp, terms = TN.mesh_of(pkg, 40), TN.strided(pkg, n), pkg.data.femur_kernel(TN.femur(pkg))
    assert smp.shape == (n, 3) and len(np.unique(smp, axis=0)) == n
    t0 = time.perf_counter()
    _, info = pkg.nystrom_model(mesh, smp, terms, k, device=0, want=("sample_eigenvalues", "sample_eigenvectors"))
    dt = time.perf_counter() - t0
    lf = NLF.long_form(mesh.points, smp, terms, k)
    blocks = -(-3 * n // DS.BLOCK)
    print(f"n {n} k {k}: {blocks} blocks, padded to {blocks + blocks % 2}; the call took {dt:.2f} s")
    check_decomposition(f"n {n}", lf["K"], lf["eigh_values"], lf["eigh_vectors"], k, info)


@pytest.mark.gpu
def test_the_row_limit_runs(pkg):
    """R = kNysMaxRows = 2,400 with k = kNysMaxRank = 256: the largest item the library takes (measured: DESIGN 5.17)"""
    assert 3 * AT_THE_ROW_LIMIT[0] == DS.MAX_ROWS
    run_at_scale(pkg, AT_THE_ROW_LIMIT)


@pytest.mark.gpu
def test_one_sample_past_twelve_hundred(pkg):
    """R = 1,203, one sample past the existing 1,200: 38 blocks as there, the last one with 19 rows and 13 of padding (the odd block count
    at scale is the row limit's: 75, padded to 76)"""
    run_at_scale(pkg, PAST_TWELVE_HUNDRED)
