"""Shape models whose posterior has a spectrum chosen by the test: the inputs of tests/test_gpu_eigen_spectra.py, pinned without a GPU
by tests/test_designed_spectra_cpu.py.

A context takes any basis Φ with positive variances λ (D = diag(√λ)); with every vertex observed once at isotropic noise σ² the matrix the
rank 65..256 eigen route decomposes is N' = D⁻¹ M D⁻¹ = D⁻² + ΦᵀΦ/σ² (M of tests/posterior_long_form.py).  For a spectrum μ (μ_min >= 2 >
1/λ_min), a random orthogonal U [r, r] and a random P [3N, r] with orthonormal columns, C = chol(σ²(U diag(μ) Uᵀ − D⁻²))ᵀ and Φ = P·C give
ΦᵀΦ = CᵀC and so N' = U diag(μ) Uᵀ up to rounding: dense, with prescribed eigenvalues.

Gaps are counted relative to the largest eigenvalue; the route judges them relative to a norm of the tridiagonal matrix, which is that
or a small multiple of it (icp_tridiag.hpp: kTriRefineGap = 1e-6 — below it the refinement step runs —, 1e-10 — below it status 2 hands
over to the Jacobi iteration)."""
import numpy as np

BANDS = (1e-11, 1e-9, 1e-7, 1e-5)  # regime(): gaps below the first, between neighbours, at or above the last


def wide(r):
    """the control: every gap about 3/(4(r − 1)) of μ_max, the vectors are handed on unrefined"""
    return np.linspace(2.0, 8.0, r)


def close(r):
    """as wide, with a pair 3e-8·μ_max apart at (10, 11), a triple 1e-7 and 2.5e-7 apart at (40, 41, 42) and a pair 5e-8 apart at the top"""
    mu = wide(r)
    top = mu[-1]
    mu[11] = mu[10] + 3e-8 * top
    mu[41] = mu[40] + 1e-7 * top
    mu[42] = mu[41] + 2.5e-7 * top
    mu[r - 2] = mu[r - 1] - 5e-8 * top
    assert np.all(np.diff(mu) > 0)
    return mu


def graded(r):
    """geometric from 2 to 2e6: six decades, as M grows under σ² = 0.01 over many observations.  Every eigenvalue is separated from its
    neighbours by a fixed fraction of itself, and the small ones — the posterior's largest variances — lie a few 1e-8 of μ_max apart.
    The lowest 32 take the ratio of rank 256 (1e6^(1/255): smallest gap 5.6e-8·μ_max) at every rank, the others one ratio from there
    up to 2e6 — at rank 256 the same ratio, below it a larger one.  (One ratio from 2 to 2e6 over r values would leave the smallest
    gap at 2.4e-7·μ_max at rank 65 and 1.1e-7 at 129: inside the refinement regime, but above the 1e-7 the regime check of these
    inputs asks for.)"""
    head = 2.0 * (1e6 ** (1.0 / 255.0)) ** np.arange(32)
    return np.concatenate([head[:-1], np.geomspace(head[-1], 2e6, r - 31)])


def multiple(r):
    """as wide, with one pair 1e-13·μ_max apart at (30, 31): below the 1e-10 the multisection tells apart"""
    mu = wide(r)
    mu[31] = mu[30] + 1e-13 * mu[-1]
    return mu


SPECTRA = {"wide": wide, "close": close, "graded": graded, "multiple": multiple}


def grid_mesh(n_grid):
    """an n_grid[0] × n_grid[1] patch, 10 mm between neighbours, gently curved"""
    a, b = n_grid
    i, j = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    ref = np.stack([10.0 * i, 10.0 * j, 4.0 * np.sin(0.5 * i) * np.cos(0.4 * j)], axis=-1).reshape(-1, 3).astype(np.float64)
    idx = np.arange(a * b).reshape(a, b)
    p, q, s, t = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    cells = np.concatenate([np.stack([p, q, s], axis=1), np.stack([q, t, s], axis=1)], axis=0).astype(np.int32)
    return ref, cells


def random_orthonormal(rng, rows, cols):
    q, rr = np.linalg.qr(rng.normal(size=(rows, cols)))
    return q * np.sign(np.diag(rr))[None, :]


def designed_model(pkg, r, mu, seed, n_grid=(8, 12), sigma2=0.25):
    """-> (model, vertex_ids, points, U, sigma2): a StatisticalMeshModel of rank r on the grid whose posterior under the observations
    (every vertex once, at a random instance of the model) at isotropic noise sigma2 has N' = U diag(mu) Uᵀ."""
    mu = np.asarray(mu, dtype=np.float64)
    assert mu.shape == (r,) and mu.min() >= 2.0
    ref, cells = grid_mesh(n_grid)
    n = ref.shape[0]
    assert 3 * n >= r
    rng = np.random.default_rng(seed)
    lam = rng.uniform(1.0, 4.0, size=r)
    U = random_orthonormal(rng, r, r)
    P = random_orthonormal(rng, 3 * n, r)
    A = sigma2 * ((U * mu[None, :]) @ U.T - np.diag(1.0 / lam))
    C = np.linalg.cholesky(0.5 * (A + A.T)).T
    model = pkg.data.StatisticalMeshModel(ref, cells, 0.05 * rng.normal(size=(n, 3)), P @ C, lam)
    ids = np.arange(n, dtype=np.int32)
    points = model.instance(0.7 * rng.normal(size=r))
    return model, ids, points, U, sigma2


def orthonormal_model(pkg, r, variance, seed, n_grid=(8, 12)):
    """a model of rank r on the grid with an orthonormal basis (P alone) and the given variances"""
    ref, cells = grid_mesh(n_grid)
    n = ref.shape[0]
    rng = np.random.default_rng(seed)
    return pkg.data.StatisticalMeshModel(ref, cells, np.zeros_like(ref), random_orthonormal(rng, 3 * n, r), np.asarray(variance, dtype=np.float64))


def n_prime(model, M):
    """D⁻¹ M D⁻¹, symmetrised, of the long form's M"""
    d = np.sqrt(model.variance)
    M = 0.5 * (M + M.T)
    return M / d[:, None] / d[None, :]


def regime(N_prime):
    """counts of the gaps between neighbouring eigenvalues of N', relative to the largest one, in the bands
    (< 1e-11), [1e-11, 1e-9), [1e-9, 1e-7), [1e-7, 1e-5), (>= 1e-5)"""
    w = np.linalg.eigvalsh(0.5 * (N_prime + N_prime.T))
    gaps = np.diff(w) / w[-1]
    return tuple(int(c) for c in np.bincount(np.searchsorted(BANDS, gaps, side="right"), minlength=5))


def in_regime(name, bands):
    """the band occupancy a spectrum of this kind must have for its test to mean anything"""
    if name == "wide":
        return sum(bands[:4]) == 0
    if name in ("close", "graded"):
        return bands[2] >= 1 and bands[0] == 0 and bands[1] == 0
    if name == "multiple":
        return bands[0] == 1 and bands[1] == 0
    raise KeyError(name)
