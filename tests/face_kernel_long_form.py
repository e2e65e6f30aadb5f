"""The long form of icp_gp_models_general_many and icp_region_weights_many in numpy (include/icp_proposal.h), for
tests/test_face_kernel_cpu.py and tests/test_gpu_face_kernel.py: kernel columns and the diagonal for general terms — Gaussian or cubic
B-spline base kernel, per-vertex weights on both arguments, the mirror symmetrisation — and the pivot loop of
tests/gp_model_long_form.py over them.

    k_t(x, y)[c][c'] = scale_t w_t(v(x)) w_t(v(y)) A_t[c][c'] (b_t(x, y) + gain_t s_c b_t(x, ym)),   ym = y mirrored, s_c = -1 on the axis
    value of a term = ((scale (w(v(x)) w(v(y)))) (b(x, y) + (gain s_c) b(x, ym))) A[c][c'], the terms summed in order
    B-spline, c = 2^level:  b(x, y) = S(x0 c, y0 c) S(x1 c, y1 c) S(x2 c, y2 c),  S(u, v) = sum_k beta(u - k) beta(v - k),
    k = ceil(max(u, v) - 2) .. floor(min(u, v) + 2) ascending

A term is anything with scale, A, weights, mirror_gain, mirror_axis and either sigma (Gaussian) or level (B-spline):
data.GaussianKernelTerm, data.BSplineKernelTerm.  The meshes and masks of the tests are made here as well."""
import contextlib

import numpy as np

import gp_model_long_form as LF


def beta3(t):
    a = np.abs(np.asarray(t, dtype=np.float64))
    inner = (2.0 / 3.0 - a * a) + ((0.5 * a) * a) * a
    outer = (((1.0 / 6.0) * (2.0 - a)) * (2.0 - a)) * (2.0 - a)
    return np.where(a < 1.0, inner, np.where(a < 2.0, outer, 0.0))


def spline_sum(u, v):
    """S(u, v), elementwise; at most five k, ascending (adding 0.0 for a k outside the range changes no bit of a sum >= 0)"""
    u, v = np.broadcast_arrays(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
    k0, k1 = np.ceil(np.maximum(u, v) - 2.0), np.floor(np.minimum(u, v) + 2.0)
    s = np.zeros(u.shape)
    for i in range(5):
        k = k0 + float(i)
        s = s + np.where(k <= k1, beta3(u - k) * beta3(v - k), 0.0)
    return s


def is_gaussian(term):
    return hasattr(term, "sigma")


def base_kernel(term, x, p):
    """b(x_i, p) for points x [n, 3] against one point p [3] -> [n]"""
    if is_gaussian(term):
        d = x - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return np.exp(-(d2 / (term.sigma * term.sigma)))
    c = 2.0 ** term.level
    return (spline_sum(x[:, 0] * c, p[0] * c) * spline_sum(x[:, 1] * c, p[1] * c)) * spline_sum(x[:, 2] * c, p[2] * c)


def _term_block(term, pts, vp):
    """the [n, 3] values val[i][c] = b(x_i, p) + (gain s_c) b(x_i, pm) and the weights' products [n] of one term against vertex vp"""
    n = pts.shape[0]
    p = pts[vp]
    val = np.repeat(base_kernel(term, pts, p)[:, None], 3, axis=1)
    if term.mirror_gain > 0.0:
        pm = p.copy()
        pm[term.mirror_axis] = -pm[term.mirror_axis]
        sgn = np.ones(3)
        sgn[term.mirror_axis] = -1.0
        val = val + (term.mirror_gain * sgn)[None, :] * base_kernel(term, pts, pm)[:, None]
    ww = np.ones(n) if term.weights is None else np.asarray(term.weights, dtype=np.float64) * float(term.weights[vp])
    return val, ww


def kernel_columns(points, terms, rows):
    """K[:, rows] -> [3N, len(rows)], the terms summed in order"""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
    out = np.zeros((3 * pts.shape[0], rows.size))
    for k, p in enumerate(rows):
        vp, cp = divmod(int(p), 3)
        col = np.zeros((pts.shape[0], 3))
        for t in terms:
            val, ww = _term_block(t, pts, vp)
            col = col + ((t.scale * ww)[:, None] * val) * np.asarray(t.A, dtype=np.float64)[None, :, cp]
        out[:, k] = col.reshape(-1)
    return out


def kernel_diagonal(points, terms):
    """diag K [3N]: every row against itself"""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    d = np.zeros((pts.shape[0], 3))
    for t in terms:
        val = np.repeat(np.array([base_kernel(t, pts[i:i + 1], pts[i])[0] for i in range(pts.shape[0])])[:, None], 3, axis=1)
        if t.mirror_gain > 0.0:
            sgn = np.ones(3)
            sgn[t.mirror_axis] = -1.0
            pm = pts.copy()
            pm[:, t.mirror_axis] = -pm[:, t.mirror_axis]
            bm = np.array([base_kernel(t, pts[i:i + 1], pm[i])[0] for i in range(pts.shape[0])])
            val = val + (t.mirror_gain * sgn)[None, :] * bm[:, None]
        ww = np.ones(pts.shape[0]) if t.weights is None else np.asarray(t.weights, dtype=np.float64) ** 2
        d = d + ((t.scale * ww)[:, None] * val) * np.diag(np.asarray(t.A, dtype=np.float64))[None, :]
    return d.reshape(-1)


def dense(points, terms):
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    return kernel_columns(pts, terms, np.arange(3 * pts.shape[0]))


def region_weights(points, region_points, stddev=40.0):
    """exp(-(d2 / (stddev stddev))), d2 the smallest (dx dx + dy dy) + dz dz to the region's points"""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    reg = np.ascontiguousarray(region_points, dtype=np.float64).reshape(-1, 3)
    d = pts[:, None, :] - reg[None, :, :]
    d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1)
    return np.exp(-(d2 / (stddev * stddev)))


@contextlib.contextmanager
def _general_kernel(pts):
    """gp_model_long_form's loop over the general kernel: its two kernel functions stand in for that module's while the loop runs"""
    saved = LF.kernel_columns, LF.kernel_diagonal
    LF.kernel_columns, LF.kernel_diagonal = kernel_columns, (lambda n, terms: kernel_diagonal(pts, terms))
    try:
        yield
    finally:
        LF.kernel_columns, LF.kernel_diagonal = saved


def long_form(points, terms, n_pivots, rank=None, rel_tolerance=0.0, pivots=None):
    """gp_model_long_form.long_form (same arguments, same result) with the general kernel"""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    with _general_kernel(pts):
        return LF.long_form(pts, terms, n_pivots, rank, rel_tolerance, pivots)


# ---------------------------------------------------------------- the tests' meshes, masks and kernels

def patch(g, jitter):
    """a g x g grid, x in [-70, 70], y in [-90, 90], z = 40 - 0.004 (x^2 + y^2), plus N(0, jitter^2) noise (seed 11)"""
    x, y = np.meshgrid(np.linspace(-70.0, 70.0, g), np.linspace(-90.0, 90.0, g), indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), 40.0 - 0.004 * (x.ravel() ** 2 + y.ravel() ** 2)], axis=1)
    if jitter:
        pts = pts + np.random.default_rng(11).normal(size=pts.shape) * jitter
    return pts


def grid_cells(g):
    i, j = np.meshgrid(np.arange(g - 1), np.arange(g - 1), indexing="ij")
    a = (i * g + j).ravel()
    return np.concatenate([np.stack([a, a + 1, a + g], axis=1), np.stack([a + 1, a + g + 1, a + g], axis=1)]).astype(np.int32)


def lat27():
    """{-8, 0, 8}^3: on lattice nodes at levels -2 and 0, neighbours two cells apart at level -2 (beta(+-2) = 0)"""
    v = np.array([-8.0, 0.0, 8.0])
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)


ONE_POINT = np.array([[0.0, 5.0, 5.0]])


def masks(points):
    """'all': 3 everywhere; 'part': -4 where x < -20, else 3 (levels -3 and -2 get a region that excludes a strip)"""
    n = points.shape[0]
    return {"all": np.full(n, 3, dtype=np.int32), "part": np.where(points[:, 0] < -20.0, -4, 3).astype(np.int32)}


FACE_LEVELS = ((-6, 128.0), (-5, 64.0), (-4, 32.0), (-3, 10.0), (-2, 4.0))


def face_terms(term_class, points, level_mask=None, gain=0.7, levels=FACE_LEVELS, stddev=40.0):
    """the face kernel's terms with the weights made HERE (numpy); level_mask None: weights None"""
    out = []
    for level, scale in levels:
        w = None if level_mask is None else region_weights(points, points[level_mask >= level], stddev)
        out.append(term_class(scale, level, np.eye(3), w, gain, 0))
    return out
