"""CPU: the designed spectra of tests/nystrom_designed_spectra.py are what their table says — asserted on the numpy long form
(tests/nystrom_model_long_form.py), so that a case can never quietly stop being hard: the exact zeros, the counts of small gaps and of
eigenvalues below the iteration's stop level, the coupling of the twin copies, eigh against the closed form of the ring cases, and
eigh's own residuals, which the GPU test's tolerances are multiples of.  The derived count ladder holds both sides of every boundary."""
import numpy as np
import pytest

import nystrom_designed_spectra as DS
import nystrom_model_long_form as NLF

EPS = DS.EPS


@pytest.fixture(scope="module")
def table(pkg):
    cases = DS.cases(pkg.data.GaussianKernelTerm)
    return cases, {name: NLF.long_form(pts, smp, terms, k, min_variance=0.0) for name, (pts, smp, terms, k, _) in cases.items()}


NAMES = ["diagonal", "near_diagonal_a", "near_diagonal_b", "circulant", "graded_a", "graded_b", "twins_coupled", "twins_below_threshold",
         "twins_exact", "twins_blocked", "rank_one_A", "scaled_one", "scaled_down", "scaled_up", "permuted", "near_diagonal_b_43",
         "graded_a_43", "twins_coupled_43"]


def test_the_table_is_complete(table):
    cases, _ = table
    assert list(cases) == NAMES and set(DS.VARIANCE_FLOOR_CASES) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_the_case_is_what_the_table_says(table, name):
    cases, lfs = table
    pts, smp, terms, k, facts = cases[name]
    lf = lfs[name]
    K, w, v = lf["K"], lf["eigh_values"], lf["eigh_vectors"]
    R, N = 3 * len(smp), len(pts)
    assert k == R == len(w) and np.array_equal(pts[:len(smp)], smp) and N == len(smp) + DS.EXTRA
    assert (3 * N) % 16 != 0 and (3 * N) % 48 != 0
    assert R == {16: 48, 32: 96, 43: 129}[len(smp)] and all(t.plain for t in terms) and len(terms) == 1
    off = K - np.diag(np.diag(K))
    ratio = np.linalg.norm(off) / np.linalg.norm(K)
    gaps = int(np.sum(-np.diff(w) < 1e-12 * w[0]))
    below, negative = int(np.sum(w < R * EPS * w[0])), int(np.sum(w < 0.0))
    res = NLF.residual(K, w, v) / w[0]
    print(f"{name}: R {R} |off|/|K| {ratio:.3e}; {gaps} of {R - 1} gaps < 1e-12 l1; {below} eigenvalues < R eps l1, {negative} negative; "
          f"l1 {w[0]:.4g} lR {w[-1]:.3e}; eigh residual {res:.2e} l1")
    # the GPU tolerances are multiples of eigh's figures: they are small
    assert res <= 1e-12
    assert np.abs(v.T @ v - np.eye(R)).max() <= 1e-12 and np.abs((v * w) @ v.T - K).max() <= 1e-12 * w[0]
    if "offdiag" in facts:
        lo, hi = facts["offdiag"]
        assert lo <= ratio <= hi
        if hi == 0.0:
            assert np.all(off == 0.0)
    if facts.get("small_gaps") is not None:
        assert gaps == facts["small_gaps"]
    if "below_level" in facts:
        assert below == facts["below_level"] and negative >= 1
    else:
        assert below == 0 and negative == 0
    if "lambda_" in facts:
        assert abs(w[0] - facts["lambda_"][0]) <= 2e-3 * w[0] and abs(w[-1] - facts["lambda_"][1]) <= 2e-2 * w[-1]
    if "ring" in facts:
        closed = DS.ring_spectrum(*facts["ring"])
        err = np.abs(closed - w).max() / w[0]
        print(f"  eigh against the closed form: {err:.2e} l1 (bound 1e-13)")
        assert closed.shape == (R,) and err <= 1e-13
    if "copies" in facts:
        a, b = facts["copies"]
        coupling = float(np.abs(K[np.ix_(a, b)]).max())
        tau = 2.0 ** -54 * np.linalg.norm(K)
        print(f"  coupling of the copies {coupling:.3e} (rotation threshold {tau:.3e})")
        lo, hi = facts["coupling"]
        assert lo <= coupling <= hi and sorted(np.concatenate([a, b]).tolist()) == list(range(len(a) + len(b)))
        assert coupling > 1e6 * tau or coupling < 1e-30 * tau  # rotated for certain, or never
    if "same_as" in facts:
        other = lfs[facts["same_as"]]["eigh_values"]
        assert np.abs(other - w).max() <= 1e-13 * w[0]


def test_diagonal_is_exactly_diagonal(table):
    cases, lfs = table
    K = lfs["diagonal"]["K"]
    assert np.array_equal(np.diag(K), np.tile([12.0, 6.0, 3.0], 32)) and np.array_equal(K, np.diag(np.diag(K)))
    assert np.array_equal(lfs["diagonal"]["eigh_values"], np.repeat([12.0, 6.0, 3.0], 32))


def test_the_scaled_cases_are_exact_powers_of_two(table):
    """every entry of K and of k(X, S) scales by exactly 2^∓40: what the GPU test's bit equalities rest on"""
    cases, lfs = table
    one = lfs["scaled_one"]
    for name, f in (("scaled_down", 2.0 ** -40), ("scaled_up", 2.0 ** 40)):
        assert np.array_equal(cases[name][0], cases["scaled_one"][0]) and np.array_equal(cases[name][1], cases["scaled_one"][1])
        assert np.array_equal(lfs[name]["K"], one["K"] * f) and np.array_equal(lfs[name]["Kxs"], one["Kxs"] * f)
        assert np.all(np.abs(lfs[name]["K"][lfs[name]["K"] != 0.0]) > 1e-200)  # (no underflow anywhere near)


def test_rank_one_factor(table):
    cases, lfs = table
    A = cases["rank_one_A"][2][0].A
    assert np.array_equal(A, A.T) and np.linalg.matrix_rank(A) == 1 and abs(np.trace(A) - 1.0) <= 4 * EPS
    w = lfs["rank_one_A"]["eigh_values"]
    assert np.abs(w[16:]).max() <= 48 * EPS * w[0] and w[15] > 1e-6 * w[0]


def test_the_basis_of_rounding_level_eigenvalues_is_not_determined(table):
    """Why the GPU test cannot hold the columns of λ at rounding level (min_variance = 0 on graded_* and rank_one_A) to 1e-9·max|b|:
    numpy's own product k(X, S)·u·√n/λ, summed over the samples in another order, differs by a tenth of max|b| and more there — and by
    3e-10 at the most on the columns a default call hands out (λ/n >= 1e-8)."""
    cases, lfs = table
    for name in DS.VARIANCE_FLOOR_CASES:
        lf, n = lfs[name], len(cases[name][1])
        ke = lf["k_eff"]
        w, v = lf["eigh_values"], lf["eigh_vectors"]
        p = np.random.default_rng(0).permutation(len(w))
        again = lf["Kxs"][:, p] @ (v[p][:, :ke] * (np.sqrt(float(n)) / w[:ke])[None, :])
        kept = int(np.sum(w / n >= 1e-8))
        tail = np.abs(again - lf["basis"]).max() / np.abs(lf["basis"]).max()
        lead = np.abs(again[:, :kept] - lf["basis"][:, :kept]).max() / np.abs(lf["basis"][:, :kept]).max()
        print(f"{name}: k_eff {ke} at min_variance 0, {kept} at 1e-8; another summation order moves the basis by {tail:.2e} max|b|, "
              f"the kept columns by {lead:.2e}")
        assert kept < ke and tail >= 1e-2 and lead <= 1e-6


def test_the_ladder_holds_both_sides_of_every_boundary():
    lad = DS.ladder()
    rs = [3 * n for n, _ in lad]
    print("ladder (n, k):", lad)
    assert 96 in rs and 192 in rs and rs == sorted(set(rs)) and not set(rs) & set(DS.EXISTING_R)
    for b, (lo, hi) in DS.boundary_sides().items():
        assert lo <= b < hi == lo + 3 and all(r in rs or r in DS.EXISTING_R for r in (lo, hi))
    ks = dict((3 * n, k) for n, k in lad)
    lo, hi = DS.boundary_sides()[DS.MAX_RANK]
    assert ks[lo] == lo and ks[hi] == DS.MAX_RANK and all(k == n // 2 + 1 for n, k in lad if 3 * n < lo)
    assert all(1 <= k <= min(3 * n, DS.MAX_RANK) and 3 * n <= DS.MAX_ROWS for n, k in lad)


def test_closed_form_against_forty_digits():
    """the circulant Gram matrix's closed form against mpmath's eigsy at 40 digits, for every σ of the ring cases; the graded spectra run
    down to 1e-41 and below (eigsy's own rounding level at 40 digits), thirty orders below anything a double decomposition can see"""
    mp = pytest.importorskip("mpmath")
    n, r = 32, 1000.0
    with mp.workdps(40):
        for sigma, floor in ((5.0, None), (60.0, None), (100.0, None), (400.0, None), (1e4, 1e-30), (1e6, 1e-30)):
            g = [mp.exp(-((2 * mp.mpf(r) * mp.sin(mp.pi * j / n)) ** 2) / mp.mpf(sigma) ** 2) for j in range(n)]
            G = mp.matrix(n, n)
            for i in range(n):
                for j in range(n):
                    G[i, j] = g[(j - i) % n]
            true = sorted((mp.eigsy(G, eigvals_only=True)), reverse=True)
            closed = np.sort(DS.ring_gram_spectrum(n, r, sigma))[::-1]
            err = max(abs(mp.mpf(float(c)) - t) for c, t in zip(closed, true)) / true[0]
            print(f"sigma {sigma:g}: closed form against 40 digits {float(err):.2e} l1; smallest true eigenvalue {float(true[-1]):.3e}")
            assert err <= 1e-13
            if floor is not None:
                assert abs(true[-1]) < floor * true[0]  # (what is left at 40 digits is eigsy's own rounding)
