"""CPU: the definition of the static target's patch balls (TargetTables::balls, k_patch_balls) and of "which patches survive", in long
form numpy, against brute force — independent of any kernel.

The sphere list is cut into patches of 128 consecutive positions.  A patch's ball is taken from the FINITE spheres among them, in f32,
by the operations of the surface filter's wave: lane l holds positions 2l and 2l + 1, adds its two centres, the 64 lane sums go through
an xor butterfly (32, 16, … 1), the centre is the sum times 1 / count, the radius the largest |c_i - C| + R_i, inflated by
1.00002 and 2e-5 of the magnitudes.  A query with bound `thr` keeps a patch if |q - C|² <= (thr + Rw + 2e-5 (|qx| + |qy| + |qz|))², and a
position of a kept patch if its sphere passes |q - c|² <= (thr + R)².

What the tables must guarantee, checked here by brute force on the small meshes of tests/test_gpu_step_search.py:
every triangle within the query's bound (the exact f64 distance to the hinted triangle) has a sphere that passes, every position whose
sphere passes lies in a patch whose ball passes (so the two levels keep exactly the set of the sphere test alone), a non-finite sphere
neither passes nor spoils its neighbours' ball, and a patch without a finite sphere passes nothing, not even an infinite bound."""
import numpy as np
import pytest

import count_ladder as CL
import test_gpu_step_search as S

f32 = np.float32
ABS_SLACK = 3.0 / 8388608.0


def round_up_f32(v):
    return np.nextafter(np.asarray(v, dtype=np.float64).astype(f32), f32(np.inf))


def tri_spheres_np(pts, cells):
    """tri_sphere: centre = centroid rounded to f32, radius = largest corner distance (f64), inflated, rounded up"""
    a, b, c = pts[cells[:, 0]], pts[cells[:, 1]], pts[cells[:, 2]]
    with np.errstate(all="ignore"):
        m = ((a + b) + c) / 3.0
        r2 = np.maximum.reduce([dot3(x - m, x - m) for x in (a, b, c)])
        R = np.sqrt(r2) * (1.0 + 2e-6) + ABS_SLACK * np.abs(m).sum(axis=1)
    return np.concatenate([m.astype(f32), round_up_f32(R)[:, None]], axis=1)


def dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def butterfly(v, op):
    """the xor butterfly of a 64-lane wave, every lane ending with the same value"""
    v = v.copy()
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[lanes ^ o])
    assert (v == v[0]).all() or np.isnan(v).all()
    return v[0]


def patch_balls_np(spheres):
    """-> [ceil(T / 128), 4] f32 (Cx, Cy, Cz, Rw); NaN centre for a patch without a finite sphere"""
    T = spheres.shape[0]
    out = np.zeros(((T + 127) // 128, 4), dtype=f32)
    add = lambda x, y: (x + y).astype(f32)
    for p in range(out.shape[0]):
        s = np.full((128, 4), np.nan, dtype=f32)
        n = min(128, T - 128 * p)
        s[:n] = spheres[128 * p:128 * p + n]
        with np.errstate(all="ignore"):
            fin = np.abs(s).sum(axis=1, dtype=f32) <= f32(3.0e38)  # (|x| + |y| + |z| + |R|, left to right)
            fin &= np.arange(128) < n
            z = np.where(fin[:, None], s, f32(0.0))
            lane = add(z[0::2], z[1::2])  # lane l: position 2l plus position 2l + 1
            cnt = add(fin[0::2].astype(f32), fin[1::2].astype(f32))
            sx, sy, sz = (butterfly(lane[:, k], add) for k in range(3))
            sn = butterfly(cnt, add)
            if not sn > 0:
                out[p] = (np.nan, np.nan, np.nan, 0.0)
                continue
            inv = f32(1.0) / sn
            C = np.array([sx * inv, sy * inv, sz * inv], dtype=f32)
            d = (s[:, :3] - C).astype(f32)
            dist = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(f32) + d[:, 2] * d[:, 2]).astype(f32)).astype(f32)
            rad = np.where(fin, (dist + s[:, 3]).astype(f32), f32(0.0)).max()
            rad = max(rad, f32(0.0))
            Rw = f32(rad * f32(1.00002)) + f32(f32(2e-5) * f32(f32(f32(abs(C[0]) + abs(C[1])) + abs(C[2])) + rad))
        out[p] = (C[0], C[1], C[2], f32(Rw))
    return out


def ball_pass(q32, thr, balls):
    """[K, P]: query k keeps patch p"""
    with np.errstate(all="ignore"):
        d = (q32[:, None, :] - balls[None, :, :3]).astype(f32)
        d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(f32) + d[..., 2] * d[..., 2]).astype(f32)
        slack = (f32(2e-5) * ((np.abs(q32[:, 0]) + np.abs(q32[:, 1])).astype(f32) + np.abs(q32[:, 2])).astype(f32)).astype(f32)
        lim = ((thr[:, None] + balls[None, :, 3]).astype(f32) + slack[:, None]).astype(f32)
        return d2 <= (lim * lim).astype(f32)


def sphere_pass(q32, thr, spheres):
    """[K, T]: the packed-f32 test (its two fused multiply-adds taken in f64 and rounded once: the products of f32 are exact there)"""
    with np.errstate(all="ignore"):
        d = (q32[:, None, :] - spheres[None, :, :3]).astype(f32).astype(np.float64)
        xx = (d[..., 0] * d[..., 0]).astype(f32).astype(np.float64)
        yy = (d[..., 1] * d[..., 1] + xx).astype(f32).astype(np.float64)
        d2 = (d[..., 2] * d[..., 2] + yy).astype(f32)
        tt = (thr[:, None] + spheres[None, :, 3]).astype(f32)
        return d2 <= (tt * tt).astype(f32)


def queries_and_bounds(pts, cells, K, rng):
    """queries a few mm off finite triangles, each with a hinted triangle nearby -> (q, q32, thr as surface_bound makes it, exact d² to
    every triangle)"""
    ok = np.nonzero(np.isfinite(pts[cells]).all(axis=(1, 2)))[0]
    t = rng.choice(ok, K)
    q = pts[cells[t]].mean(axis=1) + rng.normal(size=(K, 3)) * 2.0
    hint = ok[np.minimum(np.searchsorted(ok, t) + rng.integers(0, 5, K), len(ok) - 1)]
    with np.errstate(all="ignore"):
        o = CL.closest_point_triangle_np(q[:, None, :], pts[cells[:, 0]][None], pts[cells[:, 1]][None], pts[cells[:, 2]][None])
        d2 = dot3(q[:, None, :] - o, q[:, None, :] - o)
    dh = d2[np.arange(K), hint]
    dh = np.where(np.isnan(dh), np.inf, dh)
    thr = round_up_f32(np.sqrt(dh) * (1.0 + 2e-6) + ABS_SLACK * np.abs(q).sum(axis=1))
    return q, q.astype(f32), thr, d2, dh


@pytest.mark.parametrize("name", ["t1", "t127", "t128", "t129", "ties", "degenerate", "t8200-shuffled"])
@pytest.mark.parametrize("order", ["file", "scattered"])
def test_patch_balls_keep_what_the_spheres_keep(pkg, name, order):
    _, target, _, _ = S.build_case(pkg, name)
    pts, cells = target.points, target.cells
    rng = np.random.default_rng(3)
    if order == "scattered":  # (a sphere list whose patches are not compact: the guarantees do not depend on the order)
        cells = cells[rng.permutation(len(cells))]
    spheres = tri_spheres_np(pts, cells)
    balls = patch_balls_np(spheres)
    assert balls.shape[0] == (len(cells) + 127) // 128
    K = 48
    q, q32, thr, d2, dh = queries_and_bounds(pts, cells, K, rng)
    sp, bp = sphere_pass(q32, thr, spheres), ball_pass(q32, thr, balls)
    # 1: every triangle within the bound (exactly: at most as far as the hinted one) has a sphere that passes
    within = d2 <= dh[:, None]
    assert within.any(axis=1).all()
    assert (sp | ~within).all(), "a triangle within the bound was filtered out by its sphere"
    # 2: every position whose sphere passes lies in a surviving patch
    patch_of = np.arange(len(cells)) // 128
    assert (bp[:, patch_of] | ~sp).all(), "a patch ball dropped a position its own sphere keeps"
    # 3: non-finite spheres pass nothing under a finite bound and leave no trace in the balls
    bad = ~np.isfinite(spheres).all(axis=1)
    assert not sp[:, bad][np.isfinite(thr)].any()
    if bad.any():
        keep = np.nonzero(~bad)[0]
        for p in np.unique(patch_of[bad]):
            members = keep[patch_of[keep] == p]
            if len(members):
                assert np.isfinite(balls[p]).all()
                c, R = spheres[members, :3].astype(np.float64), spheres[members, 3].astype(np.float64)
                assert (np.linalg.norm(c - balls[p, :3].astype(np.float64), axis=1) + R <= float(balls[p, 3])).all()
    # the selectivity the search lives on, in file order on the larger meshes (not a guarantee: printed)
    print(name, order, "patches", balls.shape[0], "kept per query %.1f" % bp.sum(axis=1).mean(), "spheres kept %.1f" % sp.sum(axis=1).mean())


def test_a_patch_without_a_finite_sphere_passes_nothing():
    """128 NaN spheres, then 5 finite ones: patch 0 has a NaN centre and passes no bound, an infinite one included; patch 1 is the ball
    of its five; an infinite bound keeps every live patch and every finite sphere"""
    rng = np.random.default_rng(1)
    spheres = np.full((133, 4), np.nan, dtype=f32)
    spheres[128:, :3] = rng.normal(size=(5, 3)) * 10.0
    spheres[128:, 3] = 1.5
    balls = patch_balls_np(spheres)
    assert np.isnan(balls[0, :3]).all() and np.isfinite(balls[1]).all()
    q32 = rng.normal(size=(4, 3)).astype(f32) * 50.0
    for thr in (np.full(4, np.inf, dtype=f32), np.full(4, 1e30, dtype=f32), np.zeros(4, dtype=f32)):
        bp, sp = ball_pass(q32, thr, balls), sphere_pass(q32, thr, spheres)
        assert not bp[:, 0].any() and not sp[:, :128].any()
    assert ball_pass(q32, np.full(4, np.inf, dtype=f32), balls)[:, 1].all()
    assert sphere_pass(q32, np.full(4, np.inf, dtype=f32), spheres)[:, 128:].all()
