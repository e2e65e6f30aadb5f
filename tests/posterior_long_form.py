"""The numpy long form of a posterior shape model from correspondences, the yardstick of
tests/test_gpu_posterior_models.py; tests/test_posterior_models_cpu.py checks it against the textbook Gaussian-process posterior."""
import numpy as np


def precisions(n_obs, sigma2=None, covariances=None):
    """[n, 3, 3] Σ_i⁻¹ of either noise form"""
    if sigma2 is not None:
        return np.broadcast_to(np.eye(3) / float(sigma2), (n_obs, 3, 3)).copy()
    c = np.asarray(covariances, dtype=np.float64).reshape(n_obs, 3, 3)
    return np.linalg.inv(0.5 * (c + c.transpose(0, 2, 1)))


def long_form(model, vertex_ids, points, sigma2=None, covariances=None):
    """M = I + Σ Q_iᵀ Σ_i⁻¹ Q_i, b = Σ Q_iᵀ Σ_i⁻¹ (y_i − x̄_i − μ_i), α = M⁻¹ b, D M⁻¹ D = V S Vᵀ (S descending)."""
    ids = np.asarray(vertex_ids, dtype=np.int64).reshape(-1)
    y = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    r, N = model.rank, model.n_points
    D = np.sqrt(model.variance)
    Q = model.basis * D[None, :]
    Qo = Q.reshape(N, 3, r)[ids]
    W = precisions(ids.shape[0], sigma2, covariances)
    WQ = np.einsum("kab,kbr->kar", W, Qo)
    M = np.eye(r) + np.einsum("kar,kas->rs", Qo, WQ)
    M = 0.5 * (M + M.T)
    e = (y - model.ref_points[ids]) - model.mean_def[ids]
    b = np.einsum("kar,ka->r", WQ, e)
    alpha = np.linalg.solve(M, b)
    Minv = np.linalg.inv(M)
    Minv = 0.5 * (Minv + Minv.T)
    C = D[:, None] * Minv * D[None, :]
    S, V = np.linalg.eigh(0.5 * (C + C.T))
    S, V = S[::-1].copy(), V[:, ::-1].copy()
    mean = model.mean_def + (Q @ alpha).reshape(N, 3)
    return dict(M=M, b=b, alpha=alpha, Minv=Minv, S=S, V=V, Q=Q, mean=mean)


def covariance_blocks(Q, Minv, rows_a, rows_b):
    """3 × 3 blocks of Q M⁻¹ Qᵀ between the vertices rows_a[k] and rows_b[k] -> [n, 3, 3]"""
    r = Q.shape[1]
    Qa = Q.reshape(-1, 3, r)[np.asarray(rows_a)]
    Qb = Q.reshape(-1, 3, r)[np.asarray(rows_b)]
    return np.einsum("kar,rs,kbs->kab", Qa, Minv, Qb)


def model_blocks(basis, variance, rows_a, rows_b):
    """the same blocks of Φ'·diag(S)·Φ'ᵀ of a model (basis [3N, r], variance [r])"""
    r = basis.shape[1]
    Ba = basis.reshape(-1, 3, r)[np.asarray(rows_a)]
    Bb = basis.reshape(-1, 3, r)[np.asarray(rows_b)]
    return np.einsum("kar,r,kbr->kab", Ba, variance, Bb)


def point_variances(Q, Minv):
    """trace of every vertex's 3 × 3 block of Q M⁻¹ Qᵀ -> [N]"""
    return np.einsum("ir,rs,is->i", Q, Minv, Q).reshape(-1, 3).sum(axis=1)
