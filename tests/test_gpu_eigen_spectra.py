"""GPU: the tridiagonal eigen route (ranks 65..256, icp_tridiag.hpp) on spectra made for it — tests/designed_spectra.py: `wide` (every gap
above kTriRefineGap, the vectors handed on unrefined), `close` and `graded` (gaps between 1e-10 and 1e-6 of the norm: the Ogita-Aishima
step has vectors to correct), `multiple` (a pair 1e-13 apart: status 2, the Jacobi fall-back).  Over the rank ladder whose edges select
the reduction, solve and back-transformation templates, through icp_posterior_models_many (the capacity-32 sequence, the capacity-1
sequence, the rerun of an item on its own) and through the chain's own path (icp_proposal_posterior).  The same models of rank r, at
the edges of the Cholesky factor kernels' rank ladder (kernels_factor.hip): M and α against the numpy long form.

The reference is numpy's eigh of N' = D⁻¹MD⁻¹ from a float64 M (the long form's, or the one the call returns).  Every check is
invariant to the choice of basis inside a cluster of eigenvalues (a maximal run of reference gaps below 1e-5·μ_max).  Tolerances are
the project's own for the same quantities: S 1e-9 (check_against_long_form), VᵀV − I 1e-10 (test_gpu_rank201.py), the residual
1e-10·‖N'‖, V and projectors 1e-8 (test_gpu_face.py).  Each test asserts the band occupancy of its input (designed_spectra.regime)
before it looks at the device's output.  The measured figures are printed per rank and spectrum; the worst are in DESIGN.md §9.1."""
import numpy as np
import pytest

import designed_spectra as DS
import posterior_long_form as LF
from conftest import make_theta
from test_gpu_posterior_models import WANT, check_against_long_form, same_bits

pytestmark = pytest.mark.gpu

LADDER = (65, 128, 129, 192, 193, 200, 201, 208, 209, 256)  # both sides of every edge of tri_reduction_shape / tri_row_slots, kBigMaxRank
# `multiple` alone: both sides of launch_eigen_big's own edge as the status-2 fall-back — the full n × (n|1) image in one CU's LDS
# (k_eigen_big<true>, up to 140) | the packed triangle (k_eigen_big<false>); pinned by tests/test_designed_spectra_cpu.py
MULTIPLE_LADDER = (140, 141)
ORDER = ("wide", "close", "graded", "multiple")

# launch_posterior_factor's ladder (kernels_factor.hip), restated: rank -> the kernel that factors M.  A rank needs factor_tile_count(r)
# 2 × 4 register tiles over the r + 1 rows of [M; bᵀ]; the factor stays in LDS while (r + 1)·(r | 1) doubles fit beside the kernel's
# static arrays (w_fits), else it goes to global scratch.


def factor_kernel(r):
    tile_rows = (r + 2) >> 1
    tiles = sum((t >> 1) + 1 for t in range(tile_rows))
    w_fits = (r + 1) * (r | 1) <= 18432 - 2000
    if w_fits and tiles <= 256:
        return "k_posterior_factor_reg<1, 256>"
    if w_fits and tiles <= 1024:
        return "k_posterior_factor_reg<1, 1024>"
    if w_fits:
        return "k_posterior_factor_reg<2, 1024>"
    if tiles <= 3072:
        return "k_posterior_factor_tiles<3>"
    if tiles <= 4096:
        return "k_posterior_factor_tiles<4>"
    return "k_posterior_factor_generic"


# the last rank of every rung and the first of the next (from 128 on k_sum_partials runs ahead of the kernel: ranks 254..256 included)
FACTOR_LADDER = {
    61: "k_posterior_factor_reg<1, 256>", 62: "k_posterior_factor_reg<1, 1024>",
    125: "k_posterior_factor_reg<1, 1024>", 126: "k_posterior_factor_reg<2, 1024>",
    127: "k_posterior_factor_reg<2, 1024>", 128: "k_posterior_factor_tiles<3>",
    217: "k_posterior_factor_tiles<3>", 218: "k_posterior_factor_tiles<4>",
    253: "k_posterior_factor_tiles<4>", 254: "k_posterior_factor_generic",
}


def clusters(w):
    """maximal runs of eigenvalues (ascending) whose neighbouring gaps are below 1e-5 of the largest -> [(first, last + 1), ...]"""
    close = np.diff(w) < 1e-5 * w[-1]
    out, i, n = [], 0, w.shape[0]
    while i < n:
        j = i
        while j < n - 1 and close[j]:
            j += 1
        out.append((i, j + 1))
        i = j + 1
    return out


def check_decomposition(tag, Np, S, V):
    """S [r] descending and V [r, r] of the device against eigh of N' (S = 1/μ, column j belongs to the j-th smallest μ); every figure is
    printed before any is asserted -> the misses [(tag, figure, value), ...] for the caller to assert empty"""
    r = Np.shape[0]
    w, X = np.linalg.eigh(Np)
    proj, col = 0.0, 0.0
    for i, j in clusters(w):
        if j - i > 1:
            proj = max(proj, float(np.abs(V[:, i:j] @ V[:, i:j].T - X[:, i:j] @ X[:, i:j].T).max()))
        else:
            col = max(col, float(min(np.abs(V[:, i] - X[:, i]).max(), np.abs(V[:, i] + X[:, i]).max())))
    figures = {
        "S": (float(np.abs(S - 1.0 / w).max() / (1.0 / w).max()), 1e-9),
        "orthogonality": (float(np.abs(V.T @ V - np.eye(r)).max()), 1e-10),
        "residual": (float(np.abs(Np @ V - V / S[None, :]).max() / np.abs(Np).max()), 1e-10),
        "projectors": (proj, 1e-8),
        "columns": (col, 1e-8),
    }
    print(tag, {k: f"{v[0]:.2e}" for k, v in figures.items()}, f"clusters {sum(1 for i, j in clusters(w) if j - i > 1)}")
    misses = [(tag, k, err) for k, (err, tol) in figures.items() if not err <= tol]
    if not (np.all(np.isfinite(S)) and np.all(np.isfinite(V))):
        misses.append((tag, "not finite", float("nan")))
    if not np.all(np.diff(S) <= 0):
        misses.append((tag, "S ascends somewhere", float(np.diff(S).max())))
    return misses


class Item:
    def __init__(self, pkg, r, name, k):
        self.name = name
        self.model, self.ids, self.pts, self.U, self.sigma2 = DS.designed_model(pkg, r, DS.SPECTRA[name](r), 1000 * r + k)
        self.ctx = pkg.IcpContext(self.model, self.model.reference_mesh, device=0)
        lf = LF.long_form(self.model, self.ids, self.pts, sigma2=self.sigma2)
        self.Np = DS.n_prime(self.model, lf["M"])
        self.bands = DS.regime(self.Np)


def run(pkg, items):
    return pkg.posterior_models([it.ctx for it in items], [it.ids for it in items], [it.pts for it in items],
                                sigma2=[it.sigma2 for it in items], want=WANT)


@pytest.fixture(scope="module")
def designed(pkg):
    """rank -> (the four items by spectrum, the results of ONE call with the four of them in ORDER); made once per rank"""
    cache = {}

    def get(r):
        if r not in cache:
            items = {name: Item(pkg, r, name, k) for k, name in enumerate(DS.SPECTRA)}
            cache[r] = (items, dict(zip(ORDER, run(pkg, [items[n] for n in ORDER]))))
        return cache[r]

    yield get
    for items, _ in cache.values():
        for it in items.values():
            it.ctx.close()


def device_V(item, res):
    """V from basis_out = Φ·V (cond(Φ) is below 3, about 1.1e3 for `graded`)"""
    return np.linalg.lstsq(item.model.basis, res["basis"], rcond=None)[0]


@pytest.mark.parametrize("r", LADDER)
def test_every_rank_shape_on_every_spectrum(pkg, designed, r):
    """Four models of one rank, one per spectrum, each with its own context, in ONE call: the capacity-32 sequence with n = 4 and a
    status-2 item among them — `multiple`, which the call decomposes again on its own through launch_posterior_eigen's gated Jacobi
    fall-back: launch_eigen_big up to rank 200, the generic one-workgroup kernel above (rank 256: the whole case, rerun included,
    takes well under a second)."""
    items, res = designed(r)
    for name in ORDER:
        assert DS.in_regime(name, items[name].bands), (r, name, items[name].bands)
    assert [res[name]["status"] for name in ORDER] == [0, 0, 0, 0]
    misses = []
    for name in ORDER:
        misses += check_decomposition(f"rank {r} {name}", items[name].Np, res[name]["variance"], device_V(items[name], res[name]))
    assert not misses, misses
    for name in ORDER:
        it = items[name]
        check_against_long_form(it.model, res[name], it.ids, it.pts, it.sigma2, None, f"rank {r} {name}")
        assert all(v == 0 for v in pkg._native.runtime_stats(it.ctx.h).values()), name


@pytest.mark.parametrize("r", MULTIPLE_LADDER)
def test_multiple_spectrum_on_both_sides_of_the_square_edge(pkg, r):
    """The `multiple` model of rank 140 and of rank 141, each alone in a call: status 2 out of the multisection, then launch_eigen_big
    cold — with the square image in LDS at 140, on the packed triangle at 141 (LADDER runs the fall-back at 65, 128, 129, 192, 193 and
    200: neither side of this edge).  check_decomposition and the long form, as for the ladder's ranks."""
    it = Item(pkg, r, "multiple", list(DS.SPECTRA).index("multiple"))
    assert it.bands == (1, 0, 0, 0, r - 2) and DS.in_regime("multiple", it.bands), it.bands
    res = run(pkg, [it])[0]
    assert res["status"] == 0
    misses = check_decomposition(f"rank {r} multiple", it.Np, res["variance"], device_V(it, res))
    assert not misses, misses
    check_against_long_form(it.model, res, it.ids, it.pts, it.sigma2, None, f"rank {r} multiple")
    assert all(v == 0 for v in pkg._native.runtime_stats(it.ctx.h).values())
    it.ctx.close()


@pytest.mark.parametrize("r", [129, 209])
def test_one_item_takes_the_capacity_one_sequence(pkg, designed, r):
    """n == 1 selects kTriOne inside launch_posterior_eigen_tridiag_many: the `close` item alone gives the bits it gives among four"""
    items, res = designed(r)
    assert DS.in_regime("close", items["close"].bands)
    alone = run(pkg, [items["close"]])[0]
    assert alone["status"] == 0 and same_bits(alone, res["close"])


def test_a_multiple_neighbour_changes_nobody_elses_bits(pkg, designed):
    """abi_posterior_models.inl: an item's bits depend neither on the other items nor on their order — across the rerun of a neighbour
    whose spectrum the side-by-side decomposition could not separate."""
    items, res = designed(201)
    for name in ORDER:
        assert DS.in_regime(name, items[name].bands), (name, items[name].bands)
    between = ("wide", "close", "multiple", "graded")
    runs = [dict(zip(order, run(pkg, [items[n] for n in order]))) for order in (between, between[::-1], ("wide", "close", "graded"))]
    for name in ("wide", "close", "graded"):
        assert res[name]["status"] == 0
        for other in runs:
            assert same_bits(res[name], other[name]), name
    for other in runs[:2]:
        assert same_bits(res["multiple"], other["multiple"])


def single_path_variances(r, kind):
    """variances 1/μ, μ as the wide spectrum with one pair (30, 31) 1e-8·μ_max apart ("close") or equal ("equal")"""
    mu = DS.wide(r)
    mu[31] = mu[30] + (1e-8 * mu[-1] if kind == "close" else 0.0)
    return 1.0 / mu


@pytest.mark.parametrize("kind", ["close", "equal"])
@pytest.mark.parametrize("r", [129, 209])
def test_single_path_close_and_multiple_variances(pkg, r, kind):
    """The chain's own path (NonRigidIcpProposal.icpPosterior: capacity 1, the completion launch behind the gated fall-back) on models
    with an orthonormal basis and designed variances.  Without correspondences N' = D⁻² is diagonal with the designed pair in it —
    1e-8 apart: the refinement step; equal: status 2 and the fall-back, at rank 209 the generic kernel —; one correspondence is a
    rank-3 change of it, which moves the pair apart (its bands are printed, not asserted).  Reference: eigh of D⁻¹MD⁻¹ from the M the
    call returns.  propose(z) and propose(−z) average to propose(0)."""
    model = DS.orthonormal_model(pkg, r, single_path_variances(r, kind), 7 * r)
    ctx = pkg.IcpContext(model, model.reference_mesh, device=0)
    theta = make_theta(model, 5)
    misses = []
    for K in (0, 1):
        prop = pkg.NonRigidIcpProposal(ctx, 0.1, 6.0, 3.0, K, "ModelSampling", False)
        post = prop.icpPosterior(theta)
        assert int(post.keep.sum()) == K
        Np = DS.n_prime(model, post.M)
        bands = DS.regime(Np)
        tag = f"single path rank {r} {kind} K={K}"
        print(tag, "bands", bands)
        if K == 0:
            assert bands == ((0, 0, 1, 0, r - 2) if kind == "close" else (1, 0, 0, 0, r - 2)), bands
        misses += check_decomposition(tag, Np, post.S, post.V)
        z = np.random.default_rng(r + K).normal(size=r)
        got0, a, b = prop.propose(theta, np.zeros(r)), prop.propose(theta, z), prop.propose(theta, -z)
        assert np.all(np.isfinite(a)) and np.abs(a - got0).max() > 1e-3
        assert np.allclose(0.5 * (a + b), got0, rtol=1e-8, atol=1e-11), tag
        prop.close()
    assert not misses, misses
    assert all(v == 0 for v in pkg._native.runtime_stats(ctx.h).values())
    ctx.close()


def test_factor_ladder_edges_are_the_ones_listed():
    edges = [r for r in range(1, 256) if factor_kernel(r) != factor_kernel(r + 1)]
    assert sorted(FACTOR_LADDER) == sorted(edges + [r + 1 for r in edges])
    assert all(factor_kernel(r) == name for r, name in FACTOR_LADDER.items())


@pytest.mark.parametrize("r", sorted(FACTOR_LADDER))
def test_factor_ladder_edges_match_numpy(pkg, r):
    """Both sides of every edge of launch_posterior_factor's ladder (FACTOR_LADDER names the kernel of each rank): M and α of one
    posterior through icp_proposal_posterior — the `wide` model of rank r, identity pose, every vertex sampled, equal noise along and
    across the normal, so that Σ_i = σ²I — against the numpy long form over the correspondences the call reports, at the parity
    tests' 1e-9 of the largest entry (test_gpu_parity.py: REL).  icpPosterior raises unless the call's status is 0."""
    model = DS.designed_model(pkg, r, DS.wide(r), 1000 * r)[0]
    ctx = pkg.IcpContext(model, model.reference_mesh, device=0)
    prop = pkg.NonRigidIcpProposal(ctx, 0.1, 2.0, 2.0, model.n_points, "ModelSampling", False)
    post = prop.icpPosterior(make_theta(model, r, pose=False))
    keep = post.keep.astype(bool)
    assert keep.sum() >= model.n_points // 2
    lf = LF.long_form(model, post.corr_id[keep], post.corr_point[keep], sigma2=4.0)
    err_M = float(np.abs(post.M - lf["M"]).max() / np.abs(lf["M"]).max())
    err_alpha = float(np.abs(post.alpha - lf["alpha"]).max() / np.abs(lf["alpha"]).max())
    print(f"rank {r} {FACTOR_LADDER[r]}: M {err_M:.2e} alpha {err_alpha:.2e} kept {int(keep.sum())}")
    assert err_M < 1e-9 and err_alpha < 1e-9
    assert all(v == 0 for v in pkg._native.runtime_stats(ctx.h).values())
    prop.close()
    ctx.close()
