"""The rules of icp_scans_prepare_many (include/icp_proposal.h) in numpy: the long form the GPU tests compare with,
bit for bit, and the geometry they share.

transform   A(x): q = s·x, u = q − c, y_i = ((R_i0·u_0 + R_i1·u_1) + R_i2·u_2) + o_i, o = c + t rounded once — elementwise numpy, so
            every operation is rounded separately and in this order.
cut j       z = A(Λ[cut_landmark[j]]), d² = ((dx·dx + dy·dy) + dz·dz); the min(cut_count[j], M) vertices smallest in (d², id):
            np.lexsort((ids, d²)).
flags       bit j: in cut set j; bit 7: in the mask list (ids >= M match nothing).
compaction  boolean masks: a triangle is kept iff none of its vertices is dropped, a vertex iff a kept triangle uses it."""
import numpy as np


def transform(points, s=1.0, R=None, c=None, t=None):
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    c = np.zeros(3) if c is None else np.asarray(c, dtype=np.float64).reshape(3)
    t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).reshape(3)
    o = c + t
    u0, u1, u2 = s * p[:, 0] - c[0], s * p[:, 1] - c[1], s * p[:, 2] - c[2]
    return np.stack([((R[i, 0] * u0 + R[i, 1] * u1) + R[i, 2] * u2) + o[i] for i in range(3)], axis=1)


def squared_distances(aligned, z):
    dx, dy, dz = aligned[:, 0] - z[0], aligned[:, 1] - z[1], aligned[:, 2] - z[2]
    return (dx * dx + dy * dy) + dz * dz


def cut_set(aligned, z, count):
    """ids of the min(count, M) vertices smallest in (d², id)"""
    d2 = squared_distances(aligned, z)
    ids = np.arange(aligned.shape[0])
    return np.sort(np.lexsort((ids, d2))[:min(int(count), aligned.shape[0])])


def long_form(points, cells, s=1.0, R=None, c=None, t=None, landmarks=None, cuts=(), mask_ids=()):
    """-> dict: aligned [M,3], landmarks [L,3], cut_flags [M] uint8, partial_points, partial_cells (int32), kept_ids (int32), counts"""
    aligned = transform(points, s, R, c, t)
    M = aligned.shape[0]
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    lm_in = np.zeros((0, 3)) if landmarks is None else np.asarray(landmarks, dtype=np.float64).reshape(-1, 3)
    lm = transform(lm_in, s, R, c, t)
    flags = np.zeros(M, dtype=np.uint8)
    for j, (l, count) in enumerate(cuts):
        flags[cut_set(aligned, lm[l], count)] |= np.uint8(1 << j)
    mask = np.asarray(mask_ids, dtype=np.int64).reshape(-1)
    flags[mask[mask < M]] |= np.uint8(0x80)
    drop = flags != 0
    keep = ~drop[cells].any(axis=1) if cells.shape[0] else np.zeros(0, dtype=bool)
    used = np.zeros(M, dtype=bool)
    used[cells[keep].ravel()] = True
    new_id = -np.ones(M, dtype=np.int64)
    new_id[used] = np.arange(int(used.sum()))
    return {"aligned": aligned, "landmarks": lm, "cut_flags": flags, "partial_points": aligned[used],
            "partial_cells": new_id[cells[keep]].astype(np.int32).reshape(-1, 3), "kept_ids": np.flatnonzero(used).astype(np.int32),
            "counts": (int(used.sum()), int(keep.sum()))}


# ---------------------------------------------------------------- geometry the tests share

def lattice(M, spacing=1.0):
    """an integer lattice of ⌈√M⌉ columns truncated to M vertices (exact ties at every count), with the lattice triangles that fit:
    two per cell, (p, q, s) and (q, t, s)"""
    cols = int(np.ceil(np.sqrt(M)))
    rows = -(-M // cols)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    pts = (np.stack([i, j, 0 * i], axis=-1).reshape(-1, 3).astype(np.float64) * spacing)[:M]
    idx = np.arange(rows * cols).reshape(rows, cols)
    if rows < 2 or cols < 2:
        return pts, np.zeros((0, 3), dtype=np.int32)
    p, q, s_, t = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    cells = np.stack([np.stack([p, q, s_], axis=1), np.stack([q, t, s_], axis=1)], axis=1).reshape(-1, 3)
    return pts, cells[(cells < M).all(axis=1)].astype(np.int32)


def kabsch_rotation(seed=5):
    """a proper rotation that is no permutation of axes, through the library's own Kabsch on seeded point pairs"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(6, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return a, a @ q.T + np.array([3.0, -2.0, 0.5])
