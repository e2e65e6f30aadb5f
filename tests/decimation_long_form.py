"""The rules of icp_decimate_many (include/icp_proposal.h) in numpy: the long form the GPU tests compare with, bit
for bit, and the geometry they share.

selection   d² = ((dx·dx + dy·dy) + dz·dz) elementwise, D = np.minimum(D, d²), np.argmax: the first of equal maxima is the lowest id.
labels      half-edges = the six ordered corner pairs of every triangle (u != v), len = np.float32(np.sqrt(d²)); a sweep is ONE
            np.minimum.at on a copy of the uint64 keys with every right-hand side made from the keys before the sweep; f32 sums
            through np.float32 arrays.
triangles   np.unique(..., return_index=True) on the canonical triple keys: the first index of every key."""
import numpy as np

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def squared_distances(points, z):
    dx, dy, dz = points[:, 0] - z[0], points[:, 1] - z[1], points[:, 2] - z[2]
    return (dx * dx + dy * dy) + dz * dz


def select(points, k, start=0):
    """-> ids [k_eff] int32, cover2 [k_eff] f64"""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    kk = min(int(k), p.shape[0])
    ids, cover2 = [int(start)], []
    D = squared_distances(p, p[start])
    for _ in range(1, kk):
        v = int(np.argmax(D))
        cover2.append(D[v])
        if D[v] == 0.0:
            break
        ids.append(v)
        D = np.minimum(D, squared_distances(p, p[v]))
    else:
        cover2.append(D.max())
    return np.array(ids, dtype=np.int32), np.array(cover2, dtype=np.float64)


def half_edges(points, cells):
    """-> (u, v, len f32) of every ordered pair of distinct corners of every triangle"""
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    u = np.concatenate([c[:, 0], c[:, 1], c[:, 1], c[:, 2], c[:, 2], c[:, 0]])
    v = np.concatenate([c[:, 1], c[:, 0], c[:, 2], c[:, 1], c[:, 0], c[:, 2]])
    ok = u != v
    u, v = u[ok], v[ok]
    d = points[u] - points[v]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return u, v, np.sqrt(d2).astype(np.float32)


def label(points, cells, ids):
    """-> labels [M] int32 (−1: no sample reaches the vertex), the number of sweeps that changed a key"""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    u, v, length = half_edges(p, cells)
    key = np.full(p.shape[0], NONE, dtype=np.uint64)
    key[np.asarray(ids, dtype=np.int64)] = np.arange(len(ids), dtype=np.uint64)
    sweeps = 0
    while True:
        ku = key[u]
        live = ku != NONE
        dist = (ku[live] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        with np.errstate(over="ignore"):
            new = (dist + length[live]).astype(np.float32)
        cand = (new.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ku[live] & np.uint64(0xFFFFFFFF))
        nxt = key.copy()
        np.minimum.at(nxt, v[live], cand)
        if np.array_equal(nxt, key):
            break
        key = nxt
        sweeps += 1
    labels = np.where(key == NONE, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    return labels, sweeps


def dual_triangles(labels, cells):
    """-> [T_out, 3] int32: the candidates' canonical triples, first of every triple, in the order of their original index"""
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    l = labels.astype(np.int64)[c] if c.shape[0] else np.zeros((0, 3), dtype=np.int64)
    cand = (l >= 0).all(axis=1) & (l[:, 0] != l[:, 1]) & (l[:, 1] != l[:, 2]) & (l[:, 0] != l[:, 2])
    l = l[cand]
    first = np.argmin(l, axis=1)  # (the labels of a candidate are distinct: one smallest)
    rows = np.arange(l.shape[0])
    canon = np.stack([l[rows, first], l[rows, (first + 1) % 3], l[rows, (first + 2) % 3]], axis=1)
    keys = (canon[:, 0] << 32) | (canon[:, 1] << 16) | canon[:, 2]
    _, index = np.unique(keys, return_index=True)
    return canon[np.sort(index)].astype(np.int32).reshape(-1, 3)


def long_form(points, cells, k, start=0):
    """-> dict: ids [k_eff] int32, points [k_eff, 3], cover2 [k_eff], labels [M] int32, cells [T_out, 3] int32, counts (k_eff, T_out,
    sweeps)"""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    ids, cover2 = select(p, k, start)
    labels, sweeps = label(p, cells, ids)
    tri = dual_triangles(labels, cells)
    return {"ids": ids, "points": p[ids], "cover2": cover2, "labels": labels, "cells": tri, "counts": (len(ids), tri.shape[0], sweeps)}


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


def edge_census(cells, n_points):
    """-> (edges in 1, 2 and >= 3 triangles, Euler characteristic V − E + F with V = n_points): the plain form of data.mesh_edge_census"""
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([c[:, [0, 1]], c[:, [1, 2]], c[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(e[:, 0] * int(n_points) + e[:, 1], return_counts=True)
    return int((cnt == 1).sum()), int((cnt == 2).sum()), int((cnt >= 3).sum()), int(n_points) - cnt.shape[0] + c.shape[0]
