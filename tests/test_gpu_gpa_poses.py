"""GPU: the alignment half of icp_pca_models_many (kernels_pca_model.hip, abi_pca_models.inl) on the designed cases of
tests/gpa_designed_poses.py, pinned without a GPU by tests/test_gpa_designed_poses_cpu.py: block counts on both sides of the strided
step of pca_reduce_partials (257 row blocks, 257 vertex blocks with an outlier alone in the last), vertex sets of 1 to 5 vertices under
the rank rule, poses at which Horn's matrix is special, the cap of 32 rounds, and twins scaled by 2^∓40.  DESIGN.md §9.6.

ONE pca_models call carries every case — the 65,537-vertex items beside the one-vertex items, so the grid is sized by one item and
most workgroups of the others return at once.  The long forms are made once (gpa_designed_poses.long_forms) and shared.  The bounds
are those of tests/test_gpu_pca_models.py, unchanged; every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

import gpa_designed_poses as GP
from test_gpu_pca_models import same_bits

pytestmark = pytest.mark.gpu

EPS = GP.EPS
CASES = GP.cases()
IDS = [c["name"] for c in CASES]
INDEX = {c["name"]: q for q, c in enumerate(CASES)}
WELL_POSED = [q for q, c in enumerate(CASES) if c["group"] != "twin" and c["rank"] > 0 and not GP.invariants_only(c)]
INVARIANTS = [q for q, c in enumerate(CASES) if c["group"] != "twin" and c["rank"] > 0 and GP.invariants_only(c)]
HEALTHY = [q for q, c in enumerate(CASES) if c["rank"] > 0]
FAILING = [q for q, c in enumerate(CASES) if c["rank"] == 0]
TWINS = [q for q, c in enumerate(CASES) if c["group"] == "twin"]


def ids(qs):
    return [IDS[q] for q in qs]


@functools.lru_cache(maxsize=None)
def device():
    from conftest import load_package
    return load_package().pca_models([c["meshes"] for c in CASES], gpa_iterations=[c["iterations"] for c in CASES],
                                     halt_distance=[c["halt"] for c in CASES])


def proper(info):
    """(max |det R − 1|, max |R·Rᵀ − I|) over the item's transforms"""
    Rs = [tf[:9].reshape(3, 3) for tf in info["transforms"]]
    return max(abs(np.linalg.det(R) - 1.0) for R in Rs), max(np.abs(R @ R.T - np.eye(3)).max() for R in Rs)


@pytest.mark.parametrize("q", WELL_POSED, ids=ids(WELL_POSED))
def test_alignment_against_the_long_form(q):
    """transforms, mean shape and RMS within the conditioning bound of the long form, the rounds equal (the halt probes stop on the
    long form's round), proper rotations, and the transforms reproduce the mean shape from the data"""
    c, lf, kabsch, (model, info) = CASES[q], GP.long_forms()[q], GP.kabsch_forms()[q], device()[q]
    meshes = c["meshes"]
    bound, data = GP.conditioning_bound(meshes, lf["gap"]), GP.data_bound(meshes)
    assert info["status"] == 0 and info["n_meshes"] == c["n"]
    err = max(np.abs(info["mean"] - lf["mean"]).max(), np.abs(info["transforms"] - lf["transforms"]).max())
    det, orth = proper(info)
    cons = GP.consistency(meshes, info)
    print(f"{c['name']}: gap {lf['gap']:.3e}, device - long form {err:.3e}, CPU spread of the two solvers {GP.solver_spread(lf, kabsch):.3e}, "
          f"bound {bound:.3e}; rms {info['rms']:.6e} (long form {lf['rms'][-1]:.6e}); rounds {info['rounds']} ({lf['rounds']}); "
          f"|det R - 1| {det:.1e}, |RRt - I| {orth:.1e}; consistency {cons:.3e}, bound {data:.3e}")
    assert info["rounds"] == lf["rounds"] == c.get("stops", c["iterations"])
    assert err <= bound
    assert abs(info["rms"] - lf["rms"][-1]) <= bound
    assert det <= 1e-13 and orth <= 1e-13
    assert cons <= data
    assert np.array_equal(model.ref_points, info["mean"]) and not model.mean_def.any()


def test_a_diagonal_horn_matrix_is_decided_by_the_scan_alone():
    """half turns about x, y, z of mirror-symmetric sets (gpa_designed_poses.mirror_symmetric): every partial sum that has to vanish
    cancels exactly inside the workgroup's fixed tree, so the centroids are exactly 0 and Horn's matrix is exactly diagonal from the
    start; no Jacobi rotation is made, the scan for the largest diagonal entry picks a unit quaternion and the rotation is the exact
    signed diagonal matrix.  Hence bits, not bounds: the transforms are the half turns themselves with zero translations, the mean
    shape is the in-order mean of the meshes turned back, rounds 2 and 3 move nothing and the last RMS is exactly 0"""
    import pca_model_long_form as LF
    q = INDEX["pose " + GP.EXACT]
    c, (model, info) = CASES[q], device()[q]
    turns = [np.eye(3)] * 3 + [GP.turn(a, 2) for a in range(3)]
    print("rotations\n", info["transforms"][:, :9], "\ntranslations\n", info["transforms"][:, 9:], "\nrms", info["rms"])
    assert info["status"] == 0 and info["rounds"] == 3
    assert np.array_equal(info["transforms"][:, :9], np.stack([T.reshape(-1) for T in turns]))
    assert not info["transforms"][:, 9:].any()
    assert np.array_equal(info["mean"], LF.mean_in_order([m @ T.T for m, T in zip(c["meshes"], turns)]))
    assert info["rms"] == 0.0


@pytest.mark.parametrize("q", INVARIANTS, ids=ids(INVARIANTS))
def test_invariants_where_the_rotation_is_not_unique(q):
    """N = 2: the turn about the line through the two vertices is free, so the transforms are not compared; the aligned positions are
    unique: proper rotations, consistency with the data, the mean shape without a gap in its bound (rank and variances: below)"""
    c, lf, (model, info) = CASES[q], GP.long_forms()[q], device()[q]
    data = GP.data_bound(c["meshes"])
    det, orth = proper(info)
    cons, err = GP.consistency(c["meshes"], info), np.abs(info["mean"] - lf["mean"]).max()
    print(f"{c['name']}: |det R - 1| {det:.1e}, |RRt - I| {orth:.1e}, consistency {cons:.3e}, mean shape - long form {err:.3e}, bound {data:.3e}")
    assert info["status"] == 0 and info["rounds"] == lf["rounds"] == c["iterations"]
    assert det <= 1e-13 and orth <= 1e-13
    assert cons <= data and err <= data
    assert abs(info["rms"] - lf["rms"][-1]) <= data


@pytest.mark.parametrize("q", HEALTHY, ids=ids(HEALTHY))
def test_model_against_the_long_form(q):
    """the bounds of test_gpu_pca_models.test_model_against_the_long_form, unchanged, with the predicted rank"""
    c, lf, (model, info) = CASES[q], GP.long_forms()[q], device()[q]
    n, N, r = c["n"], c["N"], c["rank"]
    lam, theta, tau = lf["variance"], lf["theta"], lf["tau"]
    if c["group"] == "tiny":
        got = info["variance"] * N  # the device's eigenvalues, as far as the call hands them out: those it kept
        behind = f"{tau / got[r]:.2e}" if got.shape[0] > r else "none handed out (rank as predicted)"
        print(f"{c['name']}: device rank {info['rank']} (predicted {r}), theta_rank/tau {got[min(r, got.shape[0]) - 1] / tau:.2e} "
              f"(long form {theta[r - 1] / tau:.2e}), tau/(largest device eigenvalue behind the rank) {behind}; "
              f"long form tau/max|theta behind| {tau / max(np.abs(theta[r:]).max(), 1e-300):.2e}")
    assert info["status"] == 0
    assert info["rank"] == lf["rank"] == r == model.rank and model.basis.shape == (3 * N, r)
    assert np.abs(info["variance"] - lam).max() <= 1e-10 * lam[0]
    assert np.all(np.diff(info["variance"]) <= 0.0) and np.array_equal(info["variance"], model.variance)
    B = model.basis
    orth = np.abs(B.T @ B / N - np.eye(r)).max()
    print(f"{c['name']}: |BtB/N - I| {orth:.3e}, bound {1e3 * EPS * lam[0] / lam[-1]:.3e}; lambda_1 {lam[0]:.4e}, lambda_r {lam[-1]:.4e}")
    assert orth <= 1e3 * EPS * lam[0] / lam[-1]
    rows = sorted({0, 1, 3 * N // 2, 3 * N - 1})
    L = lf["L"]
    want = L[rows] @ L.T
    got = (B[rows] * info["variance"]) @ B.T
    assert np.abs(got - want).max() <= 1e-9 * float(np.sum(L * L, axis=1).max())
    assert abs(info["total_variance"] - lf["trace"] / N) <= 1e-10 * lf["trace"] / N
    if r == n - 1:
        assert abs(info["total_variance"] - info["approximated_variance"]) <= 1e-12 * info["total_variance"]


@pytest.mark.parametrize("q", FAILING, ids=ids(FAILING))
def test_one_vertex_fails_alone(q):
    """aligned, n meshes of one vertex are one point: no component is left.  Status −3 and NaN arrays for that item; its neighbours in
    the call are the healthy items of every other test here"""
    c, (model, info) = CASES[q], device()[q]
    assert model is None and info["status"] == -3 and info["rank"] == 0 and info["rounds"] == 0
    assert all(np.all(np.isnan(info[k])) for k in ("variance", "mean", "transforms"))
    assert info["mean"].shape == (1, 3) and info["transforms"].shape == (c["n"], 12)
    assert all(device()[p][1]["status"] == 0 for p in (q - 1, q + 1) if 0 <= p < len(CASES) and CASES[p]["rank"] > 0)


@pytest.mark.parametrize("q", TWINS, ids=ids(TWINS))
def test_scaling_by_a_power_of_two_is_exact(q):
    """every alignment operation is +, −, ×, ÷, √ or a comparison with a threshold that scales with the data: the rotations keep their
    bits, translations, mean shape and RMS are the base's bits times the scale, the rounds are equal.  The model half is held to the
    bounds above against the scaled base (its bits are printed, not asserted)"""
    c, (model, info) = CASES[q], device()[q]
    (bmodel, base), s = device()[INDEX[c["of"]]], c["scale"]
    assert info["status"] == base["status"] == 0 and info["rounds"] == base["rounds"] == c.get("stops", c["iterations"])
    assert np.array_equal(info["transforms"][:, :9], base["transforms"][:, :9])
    assert np.array_equal(info["transforms"][:, 9:], base["transforms"][:, 9:] * s)
    assert np.array_equal(info["mean"], base["mean"] * s)
    assert info["rms"] == base["rms"] * s and info["rms"] > 0.0
    lam = base["variance"] * s * s
    exact = np.array_equal(info["variance"], lam) and np.array_equal(model.basis, bmodel.basis)
    print(f"{c['name']}: variance - scaled base {np.abs(info['variance'] - lam).max() / lam[0]:.2e} of lambda_1, "
          f"basis - base {np.abs(model.basis - bmodel.basis).max():.2e}; model half bit-exact: {exact}")
    assert info["rank"] == base["rank"] and np.abs(info["variance"] - lam).max() <= 1e-10 * lam[0]
    N, r = c["N"], c["rank"]
    rows = sorted({0, 1, 3 * N // 2, 3 * N - 1})
    want = (bmodel.basis[rows] * lam) @ bmodel.basis.T
    got = (model.basis[rows] * info["variance"]) @ model.basis.T
    assert np.abs(got - want).max() <= 1e-9 * float(np.abs(np.sum(bmodel.basis * bmodel.basis * lam[None, :], axis=1)).max())
    assert abs(info["total_variance"] - base["total_variance"] * s * s) <= 1e-10 * base["total_variance"] * s * s


def test_the_largest_items_bits_do_not_depend_on_the_call(pkg):
    """the N = kPcaBlock² + 1 item alone == the same item inside the call of every case, every array as bytes"""
    q = INDEX[f"edge N={GP.EDGE_N[3]} n=3 rounds=3"]
    c = CASES[q]
    alone = pkg.pca_model(c["meshes"], gpa_iterations=c["iterations"], halt_distance=c["halt"])
    assert alone[1]["status"] == 0 and same_bits(alone, device()[q])
