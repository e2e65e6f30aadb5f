"""CPU: the models of tests/designed_spectra.py give the posterior spectra they were designed for — what tests/test_gpu_eigen_spectra.py
feeds the rank 65..256 eigen route is pinned here, without a GPU.

Measured (float64, ranks 65 / 129 / 256): eigenvalues of the long form's N' = D⁻¹MD⁻¹ within 4e-15·μ_max of the design for every
spectrum; 1/S of the long form (which goes through M⁻¹) within 1.3e-15·μ_max for wide / close / multiple.  graded, six decades: the
entries of M carry eps·μ_max of rounding, which the smallest eigenvalues (2, a millionth of μ_max) see in full — they come out
2.9e-11 / 3.1e-11 / 2.2e-11 relative off the design from eigh of N' and 5.0e-11 / 2.8e-11 / 1.5e-11 from 1/S; the bound asserted
is 1e-10 relative per eigenvalue, under which the grading of 2e6 stays as it is."""
import numpy as np
import pytest

import designed_spectra as DS
import posterior_long_form as LF

RANKS = (65, 129, 256)
MULTIPLE_RANKS = (140, 141)   # tests/test_gpu_eigen_spectra.py: MULTIPLE_LADDER, the `multiple` spectrum alone


@pytest.fixture(scope="module")
def designed(pkg):
    out = {}
    for r in RANKS + MULTIPLE_RANKS:
        for k, name in enumerate(DS.SPECTRA):
            if r in MULTIPLE_RANKS and name != "multiple":
                continue
            mu = DS.SPECTRA[name](r)
            model, ids, pts, U, s2 = DS.designed_model(pkg, r, mu, 1000 * r + k)
            out[r, name] = (mu, model, U, LF.long_form(model, ids, pts, sigma2=s2))
    return out


@pytest.mark.parametrize("name", list(DS.SPECTRA))
@pytest.mark.parametrize("r", RANKS)
def test_long_form_reproduces_the_designed_spectrum(designed, r, name):
    mu, model, U, lf = designed[r, name]
    assert mu.shape == (r,) and mu[0] == 2.0 and np.all(np.diff(mu) > 0)
    w, X = np.linalg.eigh(DS.n_prime(model, lf["M"]))
    inv_s = 1.0 / lf["S"]
    err_w, err_s = np.abs(w - mu).max() / mu[-1], np.abs(inv_s - mu).max() / mu[-1]
    rel_w, rel_s = (np.abs(w - mu) / mu).max(), (np.abs(inv_s - mu) / mu).max()
    print(f"rank {r} {name}: eigvalsh(N') {err_w:.1e} of mu_max ({rel_w:.1e} relative), 1/S {err_s:.1e} of mu_max ({rel_s:.1e} relative)")
    assert np.all(np.diff(lf["S"]) <= 0)
    assert err_w <= 1e-13
    if name == "graded":
        assert rel_w <= 1e-10 and rel_s <= 1e-10
    else:
        assert err_s <= 1e-13
    # ... and the eigenvectors are U's, where an eigenvalue is on its own (gaps of 1e-5·mu_max or more on both sides: eps·mu_max / gap)
    gaps = np.diff(w) / w[-1]
    alone = np.concatenate([[True], gaps >= 1e-5]) & np.concatenate([gaps >= 1e-5, [True]])
    dots = np.abs(np.einsum("ij,ij->j", X, U))
    assert alone.sum() >= (r // 4 if name == "graded" else r - 8) and np.all(dots[alone] >= 1.0 - 1e-8)


@pytest.mark.parametrize("name", list(DS.SPECTRA))
@pytest.mark.parametrize("r", RANKS)
def test_regime_reports_the_intended_bands(designed, r, name):
    mu, model, U, lf = designed[r, name]
    bands = DS.regime(DS.n_prime(model, lf["M"]))
    assert sum(bands) == r - 1 and DS.in_regime(name, bands), bands
    want = {"wide": (0, 0, 0, 0, r - 1), "multiple": (1, 0, 0, 0, r - 2)}.get(name)
    if want:
        assert bands == want
    if name == "close":  # the four designed gaps (3e-8, 5e-8 | 1e-7 on the band's edge | 2.5e-7) and nothing else below 1e-5
        assert bands[2] + bands[3] == 4 and bands[2] in (2, 3) and bands[4] == r - 5


def test_regime_counts_by_band():
    w = np.array([1.0, 1.0 + 5e-12, 1.0 + 5e-10, 2.0, 2.0 + 5e-8, 3.0, 3.0 + 5e-6, 4.0, 10.0])
    assert DS.regime(np.diag(w)) == (1, 1, 1, 1, 4)
    for name, bands, ok in (("wide", (0, 0, 0, 1, 9), False), ("close", (0, 0, 0, 4, 9), False), ("close", (0, 1, 2, 0, 9), False),
                            ("graded", (0, 0, 1, 0, 9), True), ("multiple", (2, 0, 0, 0, 9), False), ("multiple", (1, 1, 0, 0, 9), False)):
        assert DS.in_regime(name, bands) is ok, (name, bands)


@pytest.mark.parametrize("name", list(DS.SPECTRA))
@pytest.mark.parametrize("r", RANKS)
def test_gram_matrix_is_well_conditioned(designed, r, name):
    """G = QᵀQ, which icp_ctx_create factors and inverts: positive definite, condition number below 1e8"""
    mu, model, U, lf = designed[r, name]
    w = np.linalg.eigvalsh(lf["Q"].T @ lf["Q"])
    print(f"rank {r} {name}: cond(G) {w[-1] / w[0]:.1e}, cond(basis) {np.linalg.cond(model.basis):.1f}")
    assert w[0] > 0 and w[-1] / w[0] < 1e8


@pytest.mark.parametrize("r", MULTIPLE_RANKS)
def test_multiple_spectrum_at_the_square_edge_of_the_fallback(designed, r):
    """the two inputs of test_multiple_spectrum_on_both_sides_of_the_square_edge: the designed pair and nothing else below 1e-5·μ_max,
    the eigenvalues within 1e-13·μ_max of the design, a well-conditioned Gram matrix — as at RANKS"""
    from test_gpu_eigen_spectra import MULTIPLE_LADDER
    assert MULTIPLE_LADDER == MULTIPLE_RANKS
    test_long_form_reproduces_the_designed_spectrum(designed, r, "multiple")
    test_regime_reports_the_intended_bands(designed, r, "multiple")
    test_gram_matrix_is_well_conditioned(designed, r, "multiple")
