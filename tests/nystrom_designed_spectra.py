"""Designed spectra and block-count edges for the two-sided block Jacobi iteration of icp_nystrom_models_many, shared by
tests/test_nystrom_designed_spectra_cpu.py and tests/test_gpu_nystrom_spectra.py.  numpy and the standard library only.

No matrix can be handed to the library, but sample points and plain Gaussian terms design one: for ONE term, K = scale·G(S, S) ⊗ A with
G_ij = exp(−|s_i − s_j|²/σ²), so the eigenvalues of K are the products of those of G (n × n) and of A (3 × 3).  Samples on a regular
polygon make G circulant: λ(G)_m = Σ_j g_j·cos(2πjm/n) with g_j = exp(−(2r·sin(πj/n))²/σ²), a closed form that does not go through eigh.

cases(T) -> {name: (mesh points, samples, terms, k, facts)}, T = data.GaussianKernelTerm.  `facts` is what the CPU test asserts of the
case's matrix (so that a case can never quietly stop being hard) and what the GPU test needs to know of it:
    ring          (n, r, sigma, scale, eig(A)) of a ring case: ring_spectrum(*ring) is its analytic spectrum
    offdiag       ‖off‖_F/‖K‖_F, as (low, high); (0, 0): every off-diagonal entry is exactly 0.0
    small_gaps    how many of the R − 1 neighbouring gaps of the sorted spectrum are below 1e-12·λ₁
    below_level   how many eigenvalues (eigh's) are below R·2⁻⁵²·λ₁, the iteration's own stop level per row
    copies        (rows of copy 1, rows of copy 2) of a twin case, and `coupling`: (low, high) of max |K[copy 1, copy 2]| — with the
                  seeded points here 3.6e-8 at d = 400 (far above the rotation threshold 2⁻⁵⁴·‖K‖_F), 4.1e-69 at d = 900 (far below it,
                  never rotated) and exactly 0 at d = 3000
    lambda_       (λ₁, λ_R) to three digits
    same_as       a case with the same spectrum
ladder() -> the (n, k) pairs of the count ladder, derived from kNysBlock, kNysMaxRank and kNysMaxRows of icp_kernels.hpp."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "icp-proposal_amd", "csrc")
EPS = 2.0 ** -52
EXTRA = 118  # mesh points besides the samples


def source_constant(name, file="icp_kernels.hpp"):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, file)).read())
    assert m, (name, file)
    return int(m.group(1))


BLOCK, MAX_RANK, MAX_ROWS, MAX_SWEEPS = (source_constant(c) for c in ("kNysBlock", "kNysMaxRank", "kNysMaxRows", "kNysMaxSweeps"))
EXISTING_R = (63, 66, 129)  # shapes tests/test_gpu_nystrom_models.py has already


def ring(n, r):
    a = 2.0 * np.pi * np.arange(n) / n
    return np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], axis=1)


def ring_gram_spectrum(n, r, sigma):
    """the n eigenvalues of the circulant Gram matrix of Ring(n, r), in the order m = 0 .. n − 1; every sum by math.fsum"""
    g = [math.exp(-((2.0 * r * math.sin(math.pi * j / n)) ** 2) / (sigma * sigma)) for j in range(n)]
    return np.array([math.fsum(g[j] * math.cos(2.0 * math.pi * ((j * m) % n) / n) for j in range(n)) for m in range(n)])


def ring_spectrum(n, r, sigma, scale, eig_a):
    """the 3n eigenvalues of scale·G ⊗ A on Ring(n, r), descending"""
    lam = np.multiply.outer(ring_gram_spectrum(n, r, sigma), scale * np.asarray(eig_a, dtype=np.float64)).reshape(-1)
    return np.sort(lam)[::-1]


def cloud(m):
    """m points c ~ 30·N(0, I), seed 1 (the first 16 of 21 are the 16)"""
    return 30.0 * np.random.default_rng(1).normal(size=(m, 3))


def mesh_points(samples, seed):
    """the samples and EXTRA further points near them: 3N is no multiple of 16 or 48 for n = 16, 32, 43"""
    rng = np.random.default_rng(seed)
    near = samples[rng.integers(0, len(samples), EXTRA)] + 40.0 * rng.normal(size=(EXTRA, 3))
    return np.concatenate([samples, near])


def cases(T):
    diag421 = np.diag([4.0, 2.0, 1.0])
    out = {}

    def add(name, samples, terms, facts):
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        out[name] = (mesh_points(samples, 7), samples, terms, 3 * len(samples), facts)

    def add_ring(name, n, sigma, facts, order=None):
        s = ring(n, 1000.0)
        if order is not None:
            s = s[order]
        add(name, s, [T(3.0, sigma, diag421)], dict(facts, ring=(n, 1000.0, sigma, 3.0, (4.0, 2.0, 1.0))))

    pairs32, pairs43 = 3 * 15, 3 * 21  # the ring's double eigenvalues (m and n − m), times the three values of A
    add_ring("diagonal", 32, 5.0, dict(offdiag=(0.0, 0.0), small_gaps=93, lambda_=(12.0, 3.0)))
    add_ring("near_diagonal_a", 32, 60.0, dict(offdiag=(3.2e-5, 3.4e-5), small_gaps=pairs32))
    add_ring("near_diagonal_b", 32, 100.0, dict(offdiag=(2.9e-2, 3.1e-2), small_gaps=pairs32))
    add_ring("circulant", 32, 400.0, dict(small_gaps=pairs32, lambda_=(43.8, 1.6e-3)))
    add_ring("graded_a", 32, 1e4, dict(below_level=63))
    add_ring("graded_b", 32, 1e6, dict(below_level=81))
    c16 = cloud(16)
    for name, d, coupling, gaps in (("twins_coupled", 400.0, (1e-9, 1.5e-6), None), ("twins_below_threshold", 900.0, (1e-70, 1e-60), 80),
                                    ("twins_exact", 3000.0, (0.0, 0.0), 80)):
        s = np.empty((32, 3))
        s[0::2], s[1::2] = c16, c16 + np.array([d, 0.0, 0.0])
        rows = np.arange(96).reshape(32, 3)
        add(name, s, [T(3.0, 60.0, np.eye(3))], dict(copies=(rows[0::2].reshape(-1), rows[1::2].reshape(-1)), coupling=coupling, small_gaps=gaps))
    add("twins_blocked", np.concatenate([c16, c16 + np.array([3000.0, 0.0, 0.0])]), [T(3.0, 60.0, np.eye(3))],
        dict(copies=(np.arange(48), np.arange(48, 96)), coupling=(0.0, 0.0), small_gaps=80, same_as="twins_exact"))
    v = np.array([1.0, 2.0, 2.0]) / 3.0
    add("rank_one_A", c16, [T(1.0, 60.0, np.outer(v, v))], dict(below_level=32))
    for name, e in (("scaled_one", 0), ("scaled_down", -40), ("scaled_up", 40)):
        add(name, c16, [T(2.0 ** e, 60.0, diag421)], dict(small_gaps=0))
    add_ring("permuted", 32, 400.0, dict(small_gaps=pairs32, same_as="circulant"), order=np.random.default_rng(5).permutation(32))
    # R = 129: five blocks and a bye
    add_ring("near_diagonal_b_43", 43, 100.0, dict(small_gaps=pairs43))
    add_ring("graded_a_43", 43, 1e4, dict(below_level=96))
    c21 = cloud(21)
    s = np.empty((43, 3))
    s[0:42:2], s[1:42:2], s[42] = c21, c21 + np.array([400.0, 0.0, 0.0]), np.array([200.0, 5000.0, 0.0])
    rows = np.arange(126).reshape(42, 3)
    add("twins_coupled_43", s, [T(3.0, 60.0, np.eye(3))], dict(copies=(rows[0::2].reshape(-1), rows[1::2].reshape(-1)), coupling=(1e-9, 1.5e-6)))
    return out


VARIANCE_FLOOR_CASES = ("graded_a", "graded_b", "graded_a_43", "rank_one_A")  # run a second time with min_variance = 1e-8


def boundary_sides():
    """{boundary: (largest 3n <= boundary, smallest 3n > boundary)} for three, four and six blocks and kNysMaxRank"""
    return {b: (b // 3 * 3, b // 3 * 3 + 3) for b in (3 * BLOCK, 4 * BLOCK, 6 * BLOCK, MAX_RANK)}


def ladder():
    """(n, k): both sides of every boundary and the exact multiples 3n = 96 and 192, without the shapes the existing file has; k = n/2 + 1
    as apps/femur/CreateGPModel.scala has it, and k = min(3n, kNysMaxRank) at the two sides of kNysMaxRank"""
    sides = boundary_sides()
    rs = sorted(({r for pair in sides.values() for r in pair} | {3 * BLOCK, 6 * BLOCK}) - set(EXISTING_R))
    at_rank = set(sides[MAX_RANK])
    return [(r // 3, min(r, MAX_RANK) if r in at_rank else r // 3 // 2 + 1) for r in rs]
