"""The long form of icp_gp_models_many in numpy (include/icp_proposal.h), for tests/test_gp_models_cpu.py and
tests/test_gpu_gp_models.py: the pivoted Cholesky factorisation of the kernel matrix on a mesh's own points, with the pivots chosen
here or handed in, and the model from the eigen-decomposition of the m x m Gram matrix.

    k(x, y) = sum_t scale_t exp(-|x - y|^2 / sigma_t^2) A_t,   K: row 3 vertex + coordinate
    d = diag K;  step j: p = argmax d (ties: lowest row); stop BEFORE the step when max d <= n_pivots 2^-52 max(d at start) or
    sum d <= rel_tolerance trace(K);  col = K[:, p] - L[:, :j] L[p, :j]^T;  L[:, j] = col / sqrt(d[p]);  d -= L[:, j]^2 (not clamped)
    G = L^T L = W Theta W^T;  variance = Theta / N descending;  basis = sqrt(N) L W Theta^-1/2
"""
import numpy as np


def kernel_columns(points, terms, rows):
    """K[:, rows] -> [3N, len(rows)], the terms summed in order"""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
    n = pts.shape[0]
    out = np.zeros((3 * n, rows.size))
    for k, p in enumerate(rows):
        vp, cp = divmod(int(p), 3)
        d = pts - pts[vp]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        col = np.zeros((n, 3))
        for t in terms:
            col = col + (t.scale * np.exp(-(d2 / (t.sigma * t.sigma))))[:, None] * np.asarray(t.A, dtype=np.float64)[None, :, cp]
        out[:, k] = col.reshape(-1)
    return out


def kernel_diagonal(n_points, terms):
    d3 = np.zeros(3)
    for t in terms:
        d3 = d3 + t.scale * np.diag(np.asarray(t.A, dtype=np.float64))
    return np.tile(d3, n_points)


def long_form(points, terms, n_pivots, rank=None, rel_tolerance=0.0, pivots=None):
    """-> dict: L [3N, m_eff], pivots [m_eff], residual [3N], m_eff, trace, variance [rank_eff] (descending), basis [3N, rank_eff],
    theta [m_eff] (all eigenvalues of L L^T, descending), and per step made: step_max (the largest residual in front of the step),
    step_gap (largest minus runner-up), step_taken (the residual of the row that WAS taken: the handed-in pivot's, else the largest),
    step_sum (sum d in front of the step).  With `pivots` handed in, step j takes pivots[j] (a negative entry or the end of the list
    ends the loop like n_pivots does); the stopping rules are evaluated all the same."""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    d = kernel_diagonal(n, terms)
    d0max, trace = d.max(), d.sum()
    L = np.zeros((3 * n, n_pivots))
    taken, smax, sgap, stake, ssum = [], [], [], [], []
    for j in range(n_pivots):
        if pivots is not None and (j >= len(pivots) or pivots[j] < 0):
            break
        order = np.argmax(d)  # (the first of equal maxima: the lowest row)
        dmax, dsum = d[order], d.sum()
        if dmax <= n_pivots * 2.0 ** -52 * d0max or dsum <= rel_tolerance * trace:
            break
        p = int(order) if pivots is None else int(pivots[j])
        second = np.partition(d, -2)[-2] if d.size > 1 else -np.inf
        smax.append(dmax); sgap.append(dmax - second); stake.append(d[p]); ssum.append(dsum)
        col = kernel_columns(pts, terms, [p])[:, 0] - L[:, :j] @ L[p, :j]
        L[:, j] = col / np.sqrt(d[p])
        d = d - L[:, j] ** 2
        taken.append(p)
    m = len(taken)
    L = L[:, :m]
    theta, W = np.linalg.eigh(L.T @ L)
    theta, W = theta[::-1], W[:, ::-1]
    re = min(m if rank is None else rank, m)
    basis = np.sqrt(n) * (L @ W[:, :re]) / np.sqrt(theta[:re])[None, :]
    return dict(L=L, pivots=np.array(taken, dtype=np.int64), residual=d, m_eff=m, trace=trace, theta=theta, variance=theta[:re] / n, basis=basis,
                step_max=np.array(smax), step_gap=np.array(sgap), step_taken=np.array(stake), step_sum=np.array(ssum), sum_after=d.sum())
