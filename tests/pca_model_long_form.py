"""The rules of icp_pca_models_many (include/icp_proposal.h) once more, in numpy: generalised Procrustes alignment
with two mathematically equal rigid solvers, the centring, the Gram route to the PCA and the rank rule.  The alignment rules restate
Scalismo's DataCollection.gpa from memory [SCALISMO-UNVERIFIED]; the halt rule is this project's (RMS displacement of the mean shape).
Shared by tests/test_pca_models_cpu.py and tests/test_gpu_pca_models.py; also the inputs both use."""
import numpy as np

EPS = 2.0 ** -52
DATA_FLOOR = 2.0 ** -80  # tau_0's factor: (2^-40)^2


def quaternion_rotation(q):
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def cross_covariance(x, y):
    """two passes: the centroids, then S = Σ (x − c_x)(y − c_y)ᵀ of the centred points -> (S, c_x, c_y)"""
    cx, cy = x.sum(axis=0) / x.shape[0], y.sum(axis=0) / y.shape[0]
    return (x - cx).T @ (y - cy), cx, cy


def rotation_kabsch(S):
    """argmin_R Σ |R x − y|² over proper rotations, by the SVD of Sᵀ = Σ y xᵀ with the determinant correction"""
    U, _, Vt = np.linalg.svd(S.T)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    return U @ D @ Vt


def horn_matrix(S):
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = S
    return np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                     [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                     [zx - xz, xy + yx, yy - xx - zz, yz + zy],
                     [xy - yx, zx + xz, yz + zy, zz - xx - yy]])


def rotation_horn(S):
    """Horn's unit quaternion: the eigenvector of the largest eigenvalue of the symmetric 4 × 4 matrix of S (numpy.linalg.eigh)
    -> (R, the relative gap between the two largest eigenvalues: the conditioning of the rotation)"""
    w, V = np.linalg.eigh(horn_matrix(S))
    gap = (w[3] - w[2]) / max(abs(w[3]), abs(w[0]))
    return quaternion_rotation(V[:, 3]), gap


def rigid(x, y, solver="horn"):
    """the least-squares rigid transform x -> y over all vertex pairs -> (R, t, c_x, c_y, gap); aligned = (x − c_x)·Rᵀ + c_y"""
    S, cx, cy = cross_covariance(x, y)
    R, gap = rotation_horn(S)
    if solver == "kabsch":
        R = rotation_kabsch(S)
    return R, cy - R @ cx, cx, cy, gap


def mean_in_order(meshes):
    s = np.zeros_like(meshes[0])
    for m in meshes:
        s = s + m
    return s / len(meshes)


def gpa(meshes, iterations, halt_distance, solver="horn"):
    """-> dict: aligned [n, N, 3], mean [N, 3], transforms [n, 12], rounds, rms (one per round run), gap (the smallest met)"""
    x = [np.array(m, dtype=np.float64) for m in meshes]
    n = len(x)
    mean = mean_in_order(x)
    Rt, tt = [np.eye(3) for _ in range(n)], [np.zeros(3) for _ in range(n)]
    rms, gap = [], np.inf
    for _ in range(iterations):
        for j in range(n):  # every mesh of a round against the same mean shape
            R, t, cx, cy, g = rigid(x[j], mean, solver)
            x[j] = (x[j] - cx) @ R.T + cy
            Rt[j], tt[j] = R @ Rt[j], R @ tt[j] + t
            gap = min(gap, g)
        new = mean_in_order(x)
        rms.append(float(np.sqrt(np.mean(np.sum((new - mean) ** 2, axis=1)))))
        mean = new
        if rms[-1] < halt_distance:
            break
    tf = np.array([np.concatenate([Rt[j].reshape(-1), tt[j]]) for j in range(n)])
    return {"aligned": np.stack(x), "mean": mean, "transforms": tf, "rounds": len(rms), "rms": rms, "gap": gap}


def centred(aligned, mean):
    """the data matrix L [3N, n]: column j = (x_j − mean) / √(n−1)"""
    n = aligned.shape[0]
    return ((aligned - mean[None]) / np.sqrt(float(n - 1))).reshape(n, -1).T


def thresholds(aligned, L):
    """(tau, tau_0, trace G)"""
    n, N = aligned.shape[0], aligned.shape[1]
    trace = float(np.sum(L * L))
    tau0 = DATA_FLOOR * float(np.sum(aligned * aligned)) / (n - 1)
    return max(tau0, 3 * N * n * EPS * trace), tau0, trace


def pca_gram(aligned, mean, rank=None):
    """the Gram route: G = LᵀL = W Θ Wᵀ, variance Θ/N, basis √N·L·W·Θ^-1/2, the effective rank min(rank, #{θ > τ})
    -> dict: L, theta (all n, descending), tau, trace, rank, variance [rank], basis [3N, rank]"""
    n, N = aligned.shape[0], aligned.shape[1]
    L = centred(aligned, mean)
    theta, W = np.linalg.eigh(L.T @ L)
    theta, W = theta[::-1], W[:, ::-1]
    tau, tau0, trace = thresholds(aligned, L)
    re = min(n - 1 if rank is None else rank, int(np.sum(theta > tau)))
    basis = np.sqrt(float(N)) * (L @ W[:, :re]) / np.sqrt(theta[:re])[None, :]
    return {"L": L, "theta": theta, "tau": tau, "tau0": tau0, "trace": trace, "rank": re, "variance": theta[:re] / N, "basis": basis}


def pca_svd(aligned, mean):
    """the same eigenvalues by numpy.linalg.svd of the centred matrix -> (θ descending [n], left vectors [3N, n])"""
    U, s, _ = np.linalg.svd(centred(aligned, mean), full_matrices=False)
    return s * s, U


def long_form(meshes, rank=None, iterations=3, halt_distance=1e-5, solver="horn"):
    g = gpa(meshes, iterations, halt_distance, solver)
    g.update(pca_gram(g["aligned"], g["mean"], rank))
    return g


# ---- inputs

def random_rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = angle * rng.normal()
    return quaternion_rotation(np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * axis]))


def posed_instances(model, n, n_vertices=None, seed=0, angle=0.3, shift=20.0, noise=0.0):
    """n instances of `model` (c ~ N(0, I)) restricted to its first n_vertices vertices, each under a seeded random rigid motion
    (rotation ~angle rad about the centroid, translation ~shift mm), with `noise` mm of vertex noise -> list of [N, 3]"""
    rng = np.random.default_rng(seed)
    N = model.n_points if n_vertices is None else n_vertices
    out = []
    for _ in range(n):
        x = model.instance(rng.normal(size=model.rank))[:N]
        if noise > 0.0:
            x = x + noise * rng.normal(size=x.shape)
        R, c = random_rotation(rng, angle), x.mean(axis=0)
        out.append(np.ascontiguousarray((x - c) @ R.T + c + shift * rng.normal(size=3)))
    return out
