"""The long form of icp_nystrom_models_many in numpy (include/icp_proposal.h), for tests/test_nystrom_models_cpu.py and
tests/test_gpu_nystrom_models.py: the dense kernel matrices from the terms, numpy's eigh, and the formulas

    K = k(S, S) = U diag(lambda) U^T, lambda descending;   k_eff = #{i < k : lambda_i / n >= min_variance};
    variance_i = lambda_i / n;   basis column i = k(X, S) u_i sqrt(n) / lambda_i  (i < k_eff).

Plain terms (data.GaussianKernelTerm without weights and mirror) are evaluated through the terms' own callables, as
tests/test_gp_models_cpu.py's _dense does; general terms through tests/face_kernel_long_form.py's base kernels, with the weights of
the left argument handed in (the term's own at mesh points, the sample weights at sample points)."""
import ctypes

import numpy as np

import face_kernel_long_form as FK


def cross(x, s, terms, x_weights=None, s_weights=None):
    """k(x, s) -> [3 len(x), 3 len(s)], the terms summed in order; x_weights / s_weights: per term None or the weights at x / at s
    (None for the list: the terms' own weights / none)"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1, 3)
    K = np.zeros((3 * len(x), 3 * len(s)))
    if all(getattr(t, "plain", False) for t in terms):
        for t in terms:
            K += t(x[:, None, :], s[None, :, :]).transpose(0, 2, 1, 3).reshape(K.shape)
        return K
    xw = [t.weights for t in terms] if x_weights is None else list(x_weights)
    sw = [None] * len(terms) if s_weights is None else list(s_weights)
    K4 = K.reshape(len(x), 3, len(s), 3)
    for t, wx, ws in zip(terms, xw, sw):
        A = np.asarray(t.A, dtype=np.float64)
        sgn = np.ones(3)
        sgn[t.mirror_axis] = -1.0
        for j in range(len(s)):
            val = np.repeat(FK.base_kernel(t, x, s[j])[:, None], 3, axis=1)
            if t.mirror_gain > 0.0:
                sm = s[j].copy()
                sm[t.mirror_axis] = -sm[t.mirror_axis]
                val = val + (t.mirror_gain * sgn)[None, :] * FK.base_kernel(t, x, sm)[:, None]
            ww = np.ones(len(x)) if wx is None else np.asarray(wx, dtype=np.float64) * float(ws[j])
            K4[:, :, j, :] += (((t.scale * ww)[:, None] * val)[:, :, None]) * A[None, :, :]
    return K


def residual(K, lam, U):
    """max |K u_i - lambda_i u_i| over the columns of U"""
    return float(np.abs(K @ U - U * lam[None, :U.shape[1]]).max())


def long_form(points, samples, terms, rank, min_variance=1e-8, sample_weights=None, eigenvalues=None, eigenvectors=None):
    """The model of `terms` on `points`, approximated on `samples`.  eigenvalues [R] / eigenvectors [R, rank]: the decomposition to form
    the model from (the device's own), instead of eigh's."""
    x = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    s = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 3)
    n = len(s)
    K = cross(s, s, terms, sample_weights if sample_weights is not None else [None] * len(terms), sample_weights)
    K = np.triu(K) + np.triu(K, 1).T  # (both triangles from one evaluation)
    Kxs = cross(x, s, terms, None, sample_weights)
    w, v = np.linalg.eigh(K)
    w, v = w[::-1].copy(), v[:, ::-1].copy()
    lam = w if eigenvalues is None else np.asarray(eigenvalues, dtype=np.float64)
    U = v[:, :rank] if eigenvectors is None else np.asarray(eigenvectors, dtype=np.float64)
    k_eff = int(np.sum(lam[:rank] / n >= min_variance))
    basis = Kxs @ (U[:, :k_eff] * (np.sqrt(float(n)) / lam[:k_eff])[None, :])
    return {"K": K, "Kxs": Kxs, "eigh_values": w, "eigh_vectors": v, "eigenvalues": lam, "eigenvectors": U, "k_eff": k_eff,
            "variance": lam[:rank] / n, "basis": basis}


def native_call(pkg, items, min_variance=None):
    """items (points [N, 3], samples [n, 3], plain Gaussian terms, rank) straight through ctypes, past the Python-side checks ->
    (rc, status [n_items], one dict of output arrays per item); the arrays are filled with 7.0 in front of the call"""
    nat, L = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    n = len(items)
    pts = [np.ascontiguousarray(i[0], dtype=np.float64) for i in items]
    smp = [np.ascontiguousarray(i[1], dtype=np.float64) for i in items]
    terms = []
    for _, _, kb, _ in items:
        arr = (nat.KernelTermGeneral * max(len(kb), 1))()
        for t, k in enumerate(kb):
            arr[t].struct_size, arr[t].kind = ctypes.sizeof(nat.KernelTermGeneral), nat.KERNEL_GAUSSIAN
            arr[t].scale, arr[t].sigma = k.scale, k.sigma
            arr[t].A[:] = np.asarray(k.A, dtype=np.float64).reshape(-1).tolist()
        terms.append(arr)
    i32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    n_pts, n_smp, n_terms, rank = i32([len(p) for p in pts]), i32([len(s) for s in smp]), i32([len(i[2]) for i in items]), i32([i[3] for i in items])
    outs = []
    for p, s, r in zip(pts, smp, rank):
        c = max(int(r), 1)
        outs.append({"variance": np.full(c, 7.0), "basis": np.full((3 * len(p), c), 7.0), "sample_eigenvalues": np.full(3 * len(s), 7.0),
                     "sample_eigenvectors": np.full((3 * len(s), c), 7.0), "info": np.full(4, 7.0)})
    ptrs = lambda arrays: (dp * n)(*[a.ctypes.data_as(dp) for a in arrays])  # noqa: E731
    c_terms = (ctypes.POINTER(nat.KernelTermGeneral) * n)(*[ctypes.cast(a, ctypes.POINTER(nat.KernelTermGeneral)) for a in terms])
    mv = None if min_variance is None else np.ascontiguousarray(min_variance, dtype=np.float64)
    status = np.full(n, 99, dtype=np.int32)
    rc = L.icp_nystrom_models_many(n, 0, n_pts.ctypes.data_as(ip), ptrs(pts), n_smp.ctypes.data_as(ip), ptrs(smp), n_terms.ctypes.data_as(ip),
                                   c_terms, None, rank.ctypes.data_as(ip), None if mv is None else mv.ctypes.data_as(dp),
                                   *[ptrs([o[k] for o in outs]) for k in ("variance", "basis", "sample_eigenvalues", "sample_eigenvectors", "info")],
                                   status.ctypes.data_as(ip))
    return rc, status, outs
