"""Input data for the closest-point-proposal path: statistical mesh model, target meshes, synthetic targets.

Everything here is host-side preparation that the reference delegates to Scalismo IO
(`StatisticalModelIO.readStatisticalMeshModel`, `MeshIO.readMesh`, `LandmarkIO.readLandmarksJson`,
reference `apps/femur/LoadTestData.scala:32-50`).  The model arrays come from the build-owned fixtures in
`tests/golden/femur/` (bit-exact float32 copies of the reference's bundled data).

Conventions:
  ref_points  x̄  [N,3] f64     reference mesh vertices
  mean_def    μ   [N,3] f64     mean deformation (Statismo stores the mean *shape*; μ = mean − x̄)
  basis       Φ   [3N,r] f64    unscaled eigenfunctions (Statismo v0.9 layout), row 3i+d = vertex i, axis d
  variance    λ   [r]   f64     eigenvalues;  Q = Φ·diag(√λ)
  cells           [T,3] i32     triangles
"""
from __future__ import annotations

import dataclasses
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE_DIR = os.path.join(os.path.dirname(_HERE), "tests", "golden", "femur")


@dataclasses.dataclass
class TriangleMesh:
    """Counterpart of Scalismo's TriangleMesh3D as far as this path needs it: points + triangulation."""
    points: np.ndarray  # [V,3] f64
    cells: np.ndarray   # [T,3] i32

    def __post_init__(self):
        self.points = np.ascontiguousarray(self.points, dtype=np.float64)
        self.cells = np.ascontiguousarray(self.cells, dtype=np.int32)

    @property
    def n_points(self):
        return self.points.shape[0]

    @property
    def n_cells(self):
        return self.cells.shape[0]

    def transform(self, fn):
        return TriangleMesh(fn(self.points), self.cells)


@dataclasses.dataclass
class StatisticalMeshModel:
    """Counterpart of Scalismo's StatisticalMeshModel restricted to what crosses the C-ABI boundary."""
    ref_points: np.ndarray
    cells: np.ndarray
    mean_def: np.ndarray
    basis: np.ndarray
    variance: np.ndarray

    def __post_init__(self):
        self.ref_points = np.ascontiguousarray(self.ref_points, dtype=np.float64)
        self.cells = np.ascontiguousarray(self.cells, dtype=np.int32)
        self.mean_def = np.ascontiguousarray(self.mean_def, dtype=np.float64)
        self.basis = np.ascontiguousarray(self.basis, dtype=np.float64)
        self.variance = np.ascontiguousarray(self.variance, dtype=np.float64)
        assert self.basis.shape == (3 * self.ref_points.shape[0], self.variance.shape[0])

    @property
    def rank(self):
        return self.variance.shape[0]

    @property
    def n_points(self):
        return self.ref_points.shape[0]

    @property
    def n_cells(self):
        return self.cells.shape[0]

    @property
    def reference_mesh(self):
        return TriangleMesh(self.ref_points, self.cells)

    def instance(self, coeffs):
        """x̄ + μ + Q c (SURVEY App. A.1 without pose); numpy convenience, not used by the device path."""
        q = self.basis * np.sqrt(self.variance)[None, :]
        return self.ref_points + self.mean_def + (q @ np.asarray(coeffs, dtype=np.float64)).reshape(-1, 3)

    def decimate(self, k: int, start: int = 0, device: int = 0) -> "StatisticalMeshModel":
        """The model on its reference mesh decimated to min(k, N) vertices (`decimate` below): the new points are reference vertices, so
        rows 3·id … 3·id + 2 of the mean deformation and of the basis are gathered as they are and the variances stay — what
        Scalismo's model.decimate(n) yields when the new points are reference vertices, without its interpolation."""
        from . import api
        got = api.decimated_mesh(self.reference_mesh, k, start, device, want=("ids", "points", "cells"))
        ids = got["ids"].astype(np.int64)
        rows = (3 * ids[:, None] + np.arange(3)[None, :]).reshape(-1)
        return StatisticalMeshModel(got["points"], got["cells"], self.mean_def[ids], self.basis[rows], self.variance.copy())


def _general_fields(term):
    """A, weights, mirror_gain and mirror_axis of a kernel term, as arrays and numbers"""
    term.A = np.eye(3) if term.A is None else np.ascontiguousarray(term.A, dtype=np.float64)
    if term.A.shape != (3, 3):
        raise ValueError("A is a 3 x 3 matrix")
    if term.weights is not None:
        term.weights = np.ascontiguousarray(term.weights, dtype=np.float64)
        if term.weights.ndim != 1:
            raise ValueError("weights are one number per vertex")
    term.mirror_gain = float(term.mirror_gain)
    term.mirror_axis = int(term.mirror_axis)


@dataclasses.dataclass
class GaussianKernelTerm:
    """One term scale · exp(−‖x−y‖² / sigma²) · A of a matrix-valued kernel (gp_models): Scalismo's GaussianKernel(sigma) — no factor
    ½ — times a symmetric positive semi-definite 3 × 3 matrix A (DiagonalKernel: the identity).  Optionally a general term
    (icp_gp_models_general_many): per-vertex `weights` [N] on both arguments, and the mirror symmetrisation
    k(x, y) + mirror_gain · Ī · k(x, ȳ) about the plane coordinate `mirror_axis` = 0.  Without them the term is a plain one."""
    scale: float
    sigma: float
    A: np.ndarray = None
    weights: np.ndarray = None
    mirror_gain: float = 0.0
    mirror_axis: int = 0

    def __post_init__(self):
        self.scale = float(self.scale)
        self.sigma = float(self.sigma)
        _general_fields(self)

    @property
    def plain(self):
        return self.weights is None and self.mirror_gain == 0.0

    def __call__(self, x, y):
        """scale · exp(−‖x−y‖²/σ²) · A for points x [..., 3], y [..., 3] -> [..., 3, 3]: the plain term, without weights and mirror
        (numpy; the long forms of the tests use it)"""
        d = np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        return (self.scale * np.exp(-(d2 / (self.sigma * self.sigma))))[..., None, None] * self.A


@dataclasses.dataclass
class BSplineKernelTerm:
    """One term scale · w(x) · w(y) · A · (b(x, y) + mirror_gain · s · b(x, ȳ)) with b the cubic B-spline kernel on cells of 2^−level
    (Scalismo's BSplineKernel(order 3, scale level); include/icp_proposal.h states the arithmetic): what apps/bfm/FaceKernel.scala is
    made of.  `weights` [N] per vertex or None (1); ȳ is y with coordinate `mirror_axis` negated, s = −1 on that coordinate's row."""
    scale: float
    level: int
    A: np.ndarray = None
    weights: np.ndarray = None
    mirror_gain: float = 0.0
    mirror_axis: int = 0

    def __post_init__(self):
        self.scale = float(self.scale)
        if int(self.level) != self.level:
            raise ValueError("level is a whole number")
        self.level = int(self.level)
        _general_fields(self)

    plain = False


FACE_KERNEL_LEVELS = ((-6, 128.0), (-5, 64.0), (-4, 32.0), (-3, 10.0), (-2, 4.0))  # apps/bfm/FaceKernel.scala: (level, scale)
FACE_KERNEL_MIRROR_GAIN = 0.7  # 0.7·symmetrize(k) + 0.3·k = k(x, y) + 0.7·Ī·k(x, ȳ)


@dataclasses.dataclass
class FaceMask:
    """apps/bfm/FaceMask.scala as far as the face kernel needs it: one level per vertex; the region of a level is the vertices whose
    value is >= that level (bfm/CreateGPModel.scala: 3 everywhere)."""
    level_mask: np.ndarray

    def __post_init__(self):
        self.level_mask = np.ascontiguousarray(self.level_mask, dtype=np.int32)
        if self.level_mask.ndim != 1:
            raise ValueError("level_mask is one level per vertex")

    def region(self, mesh, level):
        """the points of the vertices whose level is >= `level`"""
        pts = mesh.points if hasattr(mesh, "points") else np.asarray(mesh, dtype=np.float64)
        if pts.shape[0] != self.level_mask.shape[0]:
            raise ValueError("the mask has one level per vertex of the mesh")
        reg = pts[self.level_mask >= level]
        if reg.shape[0] == 0:
            raise ValueError(f"no vertex of the mask reaches level {level}")
        return reg

    def smoothed_region_weights(self, mesh, level, stddev=40.0, device=0):
        """FaceMask.computeSmoothedRegions: exp(−d²/stddev²) per vertex, d the distance to the nearest point of the level's region
        (icp_region_weights_many)"""
        from . import api
        pts = mesh.points if hasattr(mesh, "points") else np.asarray(mesh, dtype=np.float64)
        return api.region_weights(pts, self.region(mesh, level), stddev, device)


def axis_of_main_variance(points) -> np.ndarray:
    """apps/femur/CreateGPModel.scala:48-54: the left singular vectors of the points' covariance about their centre of mass."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = 1.0 / p.shape[0]
    c = p.sum(axis=0) * n
    cov = ((p - c).T @ (p - c)) * n
    u, _, _ = np.linalg.svd(cov)
    return u


def femur_kernel(reference_mesh) -> list:
    """The kernel of apps/femur/CreateGPModel.scala:68-78 on `reference_mesh` (a TriangleMesh or points [N, 3]):
    10·B·G(90) + 5·I·G(40) + 3·I·G(10) with B = U·diag(10, 1, 1)·Uᵀ, U the axes of main variance (more variance along the bone).
    B does not depend on the signs the SVD gives its vectors; it is symmetrised exactly."""
    pts = reference_mesh.points if hasattr(reference_mesh, "points") else reference_mesh
    u = axis_of_main_variance(pts)
    b = u @ np.diag([10.0, 1.0, 1.0]) @ u.T
    b = 0.5 * (b + b.T)
    return [GaussianKernelTerm(10.0, 90.0, b), GaussianKernelTerm(5.0, 40.0, np.eye(3)), GaussianKernelTerm(3.0, 10.0, np.eye(3))]


def uniform_mesh_samples(mesh: TriangleMesh, n: int, seed: int = 0, return_cells: bool = False):
    """n random points on the surface of `mesh`, uniform by area: the stand-in for Scalismo's UniformMeshSampler3D, whose points
    api.nystrom_models takes as its sample points.  A triangle is drawn with probability proportional to its area, a point in it from
    uniform barycentric coordinates (the square-root map).  numpy on the host; the same seed gives the same points.
    -> points [n, 3], and with return_cells the triangle of every point [n] as well."""
    if int(n) != n or n < 1:
        raise ValueError("n is a whole number >= 1")
    p, cells = mesh.points, mesh.cells
    if cells.shape[0] < 1:
        raise ValueError("the mesh has no triangle")
    a, b, c = p[cells[:, 0]], p[cells[:, 1]], p[cells[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    if not (np.all(np.isfinite(area)) and area.sum() > 0.0):
        raise ValueError("the mesh has no area")
    rng = np.random.default_rng(seed)
    tri = rng.choice(cells.shape[0], size=int(n), p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(int(n))), rng.random(int(n))
    w = np.stack([1.0 - r1, r1 * (1.0 - r2), r1 * r2], axis=1)
    pts = w[:, 0:1] * a[tri] + w[:, 1:2] * b[tri] + w[:, 2:3] * c[tri]
    return (pts, tri.astype(np.int32)) if return_cells else pts


def surface_samples(mesh: TriangleMesh, n: int, seed: int = 0, device: int = 0):
    """n uniform random points on the surface of `mesh` on the device, with the triangle, the barycentric weights and the nearest
    vertex of every point (api.surface_samples, icp_surface_samples_many): Scalismo's UniformMeshSampler3D,
    deterministic to the bit under `seed`.  -> an api.SurfaceSamples; a mesh without area raises."""
    from . import api
    got = api.surface_samples([mesh], [n], [seed], device)[0]
    if got.status != 0:
        raise ValueError("the mesh has no area")
    return got


def approx_total_variance(mesh: TriangleMesh, kernel, n: int = 50000, seed: int = 1024, device: int = 0, mask=None) -> float:
    """apps/femur/CreateGPModel.scala:38-46, approxTotalVariance: the mean of trace k(x, x) over n uniform surface samples of `mesh`
    (surface_samples), for `kernel`, a list of kernel terms as api.gp_models takes it.  The reference's "ratio of approximated
    variance" of a model built from that kernel (:96) is

        variance.sum() / approx_total_variance(mesh, kernel)

    with `variance` the model's eigenvalues (api.nystrom_models, api.gp_models).  A term with weights — api.face_kernel(mesh, mask) —
    needs the `mask` (a FaceMask) it was made from: the smoothed region weights of the term's level are computed AT THE SAMPLES
    (api.region_weights, stddev 40), all levels in one call."""
    from . import api
    smp = api.surface_samples([mesh], [n], [seed], device, vertex_ids=False)[0]
    if smp.status != 0:
        raise ValueError("the mesh has no area")
    terms = list(kernel)
    weighted = [t for t, k in enumerate(terms) if getattr(k, "weights", None) is not None]
    pw = None
    if weighted:
        if mask is None or not all(isinstance(terms[t], BSplineKernelTerm) for t in weighted):
            raise ValueError("a kernel with weighted terms needs the FaceMask its B-spline terms' weights were made from")
        ws = api.region_weights([smp.points] * len(weighted), [mask.region(mesh, terms[t].level) for t in weighted], 40.0, device)
        pw = [None] * len(terms)
        for t, w in zip(weighted, ws):
            pw[t] = w
        pw = [pw]
    return float(api.total_variance([smp.points], [terms], pw, device)[0])


def fit_samples(model: StatisticalMeshModel, target: TriangleMesh, n: int, seed: int = 0, device: int = 0):
    """IcpBasedSurfaceFitting.scala:51-53: n uniform samples of the model's reference mesh, reduced to their nearest vertex ids, and n
    uniform samples of the target's surface — the `modelPointIds` / `targetPointSamples` of api.icp_fits and
    api.IcpBasedSurfaceFitting.  ONE device call with two items (api.surface_samples).  -> (ids [n] int32, points [n, 3])."""
    from . import api
    ref, tgt = api.surface_samples([model.reference_mesh, target], [n, n], [seed, seed], device, vertex_ids=[True, False])
    if ref.status != 0 or tgt.status != 0:
        raise ValueError("the model's reference mesh or the target has no area")
    return ref.vertex_ids, tgt.points


def load_femur_model(n_components: int = 50, fixture_dir: str = FIXTURE_DIR) -> StatisticalMeshModel:
    """femur GPMM with `n_components`+1 basis functions (reference: data/femur/femur_gp_model_*-components.h5)."""
    z = np.load(os.path.join(fixture_dir, f"femur_gp_model_{n_components}.npz"))
    pts = z["points"].astype(np.float64)
    mean = z["mean"].astype(np.float64)
    return StatisticalMeshModel(pts, z["cells"], mean - pts, z["pcaBasis"].astype(np.float64),
                                z["pcaVariance"].astype(np.float64))


def load_femur_mesh(name: str, fixture_dir: str = FIXTURE_DIR):
    """name in {"femur_reference","femur_target"} -> (TriangleMesh, landmark ids, landmarks [L,3])."""
    z = np.load(os.path.join(fixture_dir, name + ".npz"))
    return TriangleMesh(z["points"].astype(np.float64), z["cells"]), [str(s) for s in z["landmark_ids"]], z["landmarks"]


def rigid_landmark_transform(src: np.ndarray, dst: np.ndarray):
    """Least-squares rigid (R, t) with dst ≈ R·src + t (Kabsch).

    Stands in for Scalismo `LandmarkRegistration.rigid3DLandmarkRegistration` as called from the reference's
    `apps/util/AlignmentTransforms.scala:25-30` [SCALISMO-UNVERIFIED]; the optimum is unique, so only
    rounding differs.
    """
    src = np.asarray(src, dtype=np.float64)
    dst = np.asarray(dst, dtype=np.float64)
    cs, cd = src.mean(0), dst.mean(0)
    h = (src - cs).T @ (dst - cd)
    u, _, vt = np.linalg.svd(h)
    d = np.sign(np.linalg.det(vt.T @ u.T))
    rot = vt.T @ np.diag([1.0, 1.0, d]) @ u.T
    return rot, cd - rot @ cs


def landmark_correspondences(model: "StatisticalMeshModel", model_landmarks, target_landmarks):
    """Landmark pairs as correspondences of the model (IcpContext.posterior / posterior_models): every model landmark [L, 3] is
    matched to the nearest reference vertex (the lowest index where several are equally near: a fixed rule on
    the reference mesh) and observed at its target landmark.  -> (vertex_ids [L] int32, points [L, 3])."""
    ml = np.ascontiguousarray(model_landmarks, dtype=np.float64).reshape(-1, 3)
    tl = np.ascontiguousarray(target_landmarks, dtype=np.float64).reshape(-1, 3)
    if ml.shape != tl.shape or ml.shape[0] < 1:
        raise ValueError("one target landmark per model landmark, at least one pair")
    if not (np.all(np.isfinite(ml)) and np.all(np.isfinite(tl))):
        raise ValueError("landmarks contain a non-finite value")
    ref = model.ref_points
    ids = np.empty(ml.shape[0], dtype=np.int32)
    for k in range(ml.shape[0]):
        d = ref - ml[k]
        ids[k] = int(np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))  # (argmin: the first of equal minima)
    return ids, tl.copy()


def load_femur_model_and_target(n_components: int = 50):
    """Counterpart of reference `apps/femur/LoadTestData.scala:32-50`: model + landmark-aligned target mesh."""
    model = load_femur_model(n_components)
    _, ref_ids, ref_lms = load_femur_mesh("femur_reference")
    target, tgt_ids, tgt_lms = load_femur_mesh("femur_target")
    common = [i for i in tgt_ids if i in ref_ids]
    a = np.asarray([tgt_lms[tgt_ids.index(i)] for i in common])
    b = np.asarray([ref_lms[ref_ids.index(i)] for i in common])
    rot, t = rigid_landmark_transform(a, b)
    return model, target.transform(lambda p: p @ rot.T + t)


def subdivide(mesh: TriangleMesh, n: int) -> TriangleMesh:
    """n-way edge subdivision: every triangle -> n² triangles; shared edge/corner vertices are merged.

    V' = V + (n-1)·E + (n-1)(n-2)/2·F.  Used to synthesise the "~50k-vertex target" of BASELINE.json
    (n=6 on the femur target gives 58,322 vertices / 116,640 triangles).
    """
    pts, cells = mesh.points, mesh.cells
    V = pts.shape[0]
    new_pts = [pts]
    count = V
    edge_ids = {}

    def edge_points(a, b):
        nonlocal count
        key = (a, b) if a < b else (b, a)
        ids = edge_ids.get(key)
        if ids is None:
            lo, hi = key
            w = (np.arange(1, n, dtype=np.float64) / n)[:, None]
            new_pts.append(pts[lo] * (1.0 - w) + pts[hi] * w)
            ids = np.arange(count, count + n - 1, dtype=np.int64)
            count += n - 1
            edge_ids[key] = ids
        return ids if a < b else ids[::-1]

    out_cells = []
    for a, b, c in cells.tolist():
        # barycentric lattice: node (i,j) = a + (b-a)·i/n + (c-a)·j/n, i+j<=n
        idx = -np.ones((n + 1, n + 1), dtype=np.int64)
        idx[0, 0], idx[n, 0], idx[0, n] = a, b, c
        eab, eac, ebc = edge_points(a, b), edge_points(a, c), edge_points(b, c)
        for i in range(1, n):
            idx[i, 0] = eab[i - 1]
            idx[0, i] = eac[i - 1]
            idx[n - i, i] = ebc[i - 1]
        inner = [(i, j) for i in range(1, n) for j in range(1, n - i)]
        if inner:
            ij = np.asarray(inner, dtype=np.float64)
            p = pts[a] + (pts[b] - pts[a]) * (ij[:, :1] / n) + (pts[c] - pts[a]) * (ij[:, 1:] / n)
            new_pts.append(p)
            for k, (i, j) in enumerate(inner):
                idx[i, j] = count + k
            count += len(inner)
        for i in range(n):
            for j in range(n - i):
                out_cells.append((idx[i, j], idx[i + 1, j], idx[i, j + 1]))
                if i + j < n - 1:
                    out_cells.append((idx[i + 1, j], idx[i + 1, j + 1], idx[i, j + 1]))
    return TriangleMesh(np.concatenate(new_pts, axis=0), np.asarray(out_cells, dtype=np.int32))


def synthetic_femur_target(n_subdiv: int = 6, jitter_mm: float = 0.05, seed: int = 1024,
                           n_components: int = 50):
    """BASELINE.json metric config (`configs[1]`): femur model + the aligned bundled target subdivided
    `n_subdiv`-way with seeded N(0, jitter) vertex noise (removes coplanar ties).  SURVEY.md §8d."""
    model, target = load_femur_model_and_target(n_components)
    big = subdivide(target, n_subdiv) if n_subdiv > 1 else target
    if jitter_mm > 0:
        rng = np.random.Generator(np.random.PCG64(seed))
        big = TriangleMesh(big.points + rng.normal(0.0, jitter_mm, size=big.points.shape), big.cells)
    return model, big


def decimated_point_subset(mesh: TriangleMesh, k: int) -> np.ndarray:
    """Stand-in for Scalismo `mesh.operations.decimate(k).pointSet.points` (VTK quadric decimation; not
    reproducible here).  Only the resulting point list crosses the C-ABI, so any host-side
    choice is valid input; we take k vertices by a deterministic stride over the vertex list."""
    k = min(k, mesh.n_points)
    idx = (np.arange(k, dtype=np.int64) * mesh.n_points) // k
    return mesh.points[idx].copy()


def decimate(mesh: TriangleMesh, k: int, start: int = 0, device: int = 0) -> TriangleMesh:
    """`mesh` decimated to min(k, M) of its own vertices on the device (api.decimated_meshes, icp_decimate_many):
    farthest-point samples from vertex `start`, triangles from their graph-distance cells.  Not VTK's quadric decimation (which the
    reference's mesh.operations.decimate(k) calls and which cannot be reproduced), deterministic to the bit.  Its `.points` are the
    opt-in alternative to decimated_point_subset for the `decimatedTargetPoints=` arguments; mesh_edge_census says whether the
    triangles form a manifold."""
    from . import api
    got = api.decimated_mesh(mesh, k, start, device, want=("points", "cells"))
    return TriangleMesh(got["points"], got["cells"])


def mesh_edge_census(mesh: TriangleMesh) -> dict:
    """How many undirected edges of `mesh` lie in exactly one triangle ("boundary"), in two ("interior") and in three or more
    ("non_manifold"), and the Euler characteristic V − E + F over all its vertices ("euler").  A closed manifold has no boundary and
    no non-manifold edge; a sphere's Euler characteristic is 2."""
    c = mesh.cells.astype(np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([c[:, [0, 1]], c[:, [1, 2]], c[:, [2, 0]]], axis=0), axis=1)
    _, cnt = np.unique(e[:, 0] * mesh.n_points + e[:, 1], return_counts=True)
    return {"boundary": int((cnt == 1).sum()), "interior": int((cnt == 2).sum()), "non_manifold": int((cnt >= 3).sum()),
            "euler": int(mesh.n_points - cnt.shape[0] + c.shape[0])}


def boundary_vertex_flags(mesh: TriangleMesh) -> np.ndarray:
    """vertex lies on an edge owned by exactly one triangle (Scalismo `pointIsOnBoundary`)."""
    c = mesh.cells.astype(np.int64)
    e = np.concatenate([c[:, [0, 1]], c[:, [1, 2]], c[:, [2, 0]]], axis=0)
    e.sort(axis=1)
    key = e[:, 0] * mesh.n_points + e[:, 1]
    uniq, cnt = np.unique(key, return_counts=True)
    b = uniq[cnt == 1]
    flags = np.zeros(mesh.n_points, dtype=np.uint8)
    flags[b // mesh.n_points] = 1
    flags[b % mesh.n_points] = 1
    return flags


# ---------------------------------------------------------------------------------------------------------------
# Synthetic stand-in for the Basel Face Model configurations (BASELINE.json configs[3], configs[4]).
# The BFM-2017 files are not redistributable and absent from the reference tree (README.md:60-70, .gitignore:26-29);
# SURVEY.md §8d prescribes a procedural model of the same SIZE: an open height-field "face" patch with smooth
# low-frequency deformation modes, and a partial target with a hole (the reference crops its scans around the nose,
# apps/bfm/AlignShapes.scala:90-92).  Nothing here claims to resemble the BFM statistically.

def synthetic_face_model(grid: int = 169, rank: int = 200, seed: int = 2017) -> StatisticalMeshModel:
    """grid×grid vertices (169 -> N = 28,561, T = 56,448; BFM face12 has 28,588 / 56,572), `rank` deformation modes.

    Geometry: a 150 mm × 200 mm patch with a nose-like bump.  Basis: 2-D cosine modes cos(pi p u)·cos(pi q v) on cell-centred
    coordinates (exactly orthogonal on the grid), ordered by frequency; every mode deforms along a seeded random unit
    direction; columns are scaled to squared norm N like Statismo's unscaled eigenfunctions; the variances decay
    with frequency from 25 down to ~0.05 mm²."""
    g = int(grid)
    u = (np.arange(g) + 0.5) / g
    uu, vv = np.meshgrid(u, u, indexing="ij")
    x = 150.0 * (uu - 0.5)
    y = 200.0 * (vv - 0.5)
    z = 45.0 * np.exp(-((uu - 0.5) ** 2 + (vv - 0.45) ** 2) / 0.012) + 12.0 * np.cos(np.pi * (uu - 0.5)) * np.cos(np.pi * (vv - 0.5))
    ref = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    idx = np.arange(g * g).reshape(g, g)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    cells = np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)], axis=0).astype(np.int32)
    n = g * g
    modes = sorted(((p * p + q * q, p, q) for p in range(32) for q in range(32)))[1:rank + 1]   # skip the constant mode
    rng = np.random.Generator(np.random.PCG64(seed))
    basis = np.empty((3 * n, rank))
    var = np.empty(rank)
    for j, (f2, p, q) in enumerate(modes):
        phi = (np.cos(np.pi * p * uu) * np.cos(np.pi * q * vv)).reshape(-1)
        dirn = rng.normal(size=3)
        dirn /= np.linalg.norm(dirn)
        col = (phi[:, None] * dirn[None, :]).reshape(-1)
        basis[:, j] = col * np.sqrt(n / np.dot(col, col))
        var[j] = 25.0 * np.exp(-f2 / 40.0) + 0.05
    return StatisticalMeshModel(ref, cells, np.zeros_like(ref), basis, var)


def synthetic_partial_target(model: StatisticalMeshModel, seed: int = 7, n_remove: int = 1000, coeff_scale: float = 0.5,
                             jitter_mm: float = 0.02) -> TriangleMesh:
    """A model sample (coefficients ~ coeff_scale·N(0, I), seeded) with the `n_remove` vertices nearest to the nose tip cut
    out (and seeded vertex jitter against exact ties): a target with an inner boundary, as in apps/bfm/BfmFittingPartial.scala."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = model.instance(coeff_scale * rng.normal(size=model.rank))
    pts = pts + rng.normal(0.0, jitter_mm, size=pts.shape)
    tip = int(np.argmax(model.ref_points[:, 2]))
    drop = np.zeros(model.n_points, dtype=bool)
    drop[np.argsort(np.linalg.norm(model.ref_points - model.ref_points[tip], axis=1))[:n_remove]] = True
    keep_cells = model.cells[~drop[model.cells].any(axis=1)]
    used = np.zeros(model.n_points, dtype=bool)
    used[keep_cells.ravel()] = True
    remap = -np.ones(model.n_points, dtype=np.int64)
    remap[used] = np.arange(int(used.sum()))
    return TriangleMesh(pts[used], remap[keep_cells].astype(np.int32))



# ---------------------------------------------------------------------------------------------------------------
# Target preparation: what apps/femur/AlignShapes.scala:30-55 and apps/bfm/AlignShapes.scala:33-101 do to a raw scan in front of
# either study — scale, landmark alignment, the cut around a landmark plus an id list, compaction.  The arithmetic runs on the device
# (api.prepare_scans, icp_scans_prepare_many); Kabsch on a handful of landmark pairs stays here.

@dataclasses.dataclass
class ScanTransform:
    """A(x) = R·(s·x − c) + c + t: Scalismo's translation ∘ rotation-about-c behind Scaling(s) (AlignmentTransforms.scala:25-30,
    apps/bfm/AlignShapes.scala:66,77-83)."""
    pre_scale: float = 1.0
    rotation: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(3))   # [3,3]
    centre: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(3))
    translation: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(3))

    def __post_init__(self):
        self.pre_scale = float(self.pre_scale)
        self.rotation = np.ascontiguousarray(self.rotation, dtype=np.float64).reshape(3, 3)
        self.centre = np.ascontiguousarray(self.centre, dtype=np.float64).reshape(3)
        self.translation = np.ascontiguousarray(self.translation, dtype=np.float64).reshape(3)


def landmark_alignment(scan_landmarks, model_landmarks, centre=(0.0, 0.0, 0.0), pre_scale: float = 1.0) -> ScanTransform:
    """AlignmentTransforms.computeTransform (apps/util/AlignmentTransforms.scala:25-30) behind Scaling(pre_scale): both arguments map
    landmark names to points; the pairs are the names common to both, in the scan's order (`lm1.map(_.id) intersect lm2.map(_.id)`);
    Kabsch (rigid_landmark_transform) takes the pre-scaled scan landmarks onto the model's, rotating about `centre`."""
    names = [k for k in scan_landmarks if k in model_landmarks]
    if len(names) < 3:
        raise ValueError("a rigid alignment needs at least three landmark names common to scan and model")
    c = np.ascontiguousarray(centre, dtype=np.float64).reshape(3)
    s = float(pre_scale)
    src = np.asarray([np.asarray(scan_landmarks[k], dtype=np.float64).reshape(3) for k in names]) * s - c
    dst = np.asarray([np.asarray(model_landmarks[k], dtype=np.float64).reshape(3) for k in names]) - c
    if not (np.isfinite(s) and s > 0.0 and np.all(np.isfinite(src)) and np.all(np.isfinite(dst))):
        raise ValueError("pre_scale must be positive and the landmarks finite")
    rot, t = rigid_landmark_transform(src, dst)
    return ScanTransform(s, rot, c, t)


def aligned_and_partial_targets(scans, scan_landmarks, model_landmarks, pre_scale: float = 1.0, cut_landmark=None, cut_count: int = 0,
                                mask_ids=(), drop_landmarks=(), device: int = 0):
    """The two AlignShapes.main loops in one call (apps/femur/AlignShapes.scala:30-55: alignment alone; apps/bfm/AlignShapes.scala:
    71-100: scale, alignment, the `cut_count` vertices nearest the aligned landmark `cut_landmark` plus `mask_ids` cut away, the rest
    compacted).  scans: TriangleMesh per scan; scan_landmarks: a name -> point mapping per scan; model_landmarks: one mapping.
    -> (aligned meshes, partial meshes, aligned landmark dicts, partial landmark dicts: without the names in drop_landmarks, :93).
    The mouth id list of the reference is part of its program text: the caller passes its own ids."""
    from . import api
    scans, scan_landmarks = list(scans), list(scan_landmarks)
    if len(scans) != len(scan_landmarks) or not scans:
        raise ValueError("one landmark mapping per scan, at least one scan")
    transforms, points, cuts = [], [], []
    for lms in scan_landmarks:
        transforms.append(landmark_alignment(lms, model_landmarks, pre_scale=pre_scale))
        points.append(np.asarray([np.asarray(lms[k], dtype=np.float64).reshape(3) for k in lms]).reshape(-1, 3))
        if cut_landmark is None:
            cuts.append([])
        else:
            if cut_landmark not in lms:
                raise ValueError(f"a scan has no landmark {cut_landmark!r} to cut around")
            cuts.append([(list(lms).index(cut_landmark), int(cut_count))])
    got = api.prepare_scans(scans, transforms, points, cuts, [np.asarray(mask_ids, dtype=np.int64).reshape(-1)] * len(scans), device=device,
                            want=("aligned", "partial", "landmarks"))
    aligned_lms = [{k: g["landmarks"][i].copy() for i, k in enumerate(lms)} for g, lms in zip(got, scan_landmarks)]
    dropped = set(drop_landmarks)
    partial_lms = [{k: v for k, v in d.items() if k not in dropped} for d in aligned_lms]
    return [g["aligned"] for g in got], [g["partial"] for g in got], aligned_lms, partial_lms
