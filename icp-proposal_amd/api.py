"""Host-side mirror of the reference's plug-in surface for the closest-point-proposal path.

Same names, argument meaning and error behaviour as the reference's Scala classes (paths relative to the
reference's src/main/scala/), implemented as thin wrappers over the C ABI (include/icp_proposal.h):

    ModelFittingParameters                 api/sampling/ModelFittingParameters.scala:47-66
    NonRigidIcpProposal                    api/sampling/proposals/NonRigidIcpProposal.scala:30-155
    IndependentPointDistanceEvaluator      api/sampling/evaluators/IndependentPointDistanceEvaluator.scala:27-67
    HausdorffDistanceEvaluator             api/sampling/evaluators/HausdorffDistanceEvaluator.scala:25-36
    CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator   …/CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator.scala:27-79
    ModelPriorEvaluator                    api/sampling/evaluators/ModelPriorEvaluator.scala:24-31
    AcceptAllEvaluator                     api/sampling/evaluators/AcceptAllEvaluator.scala:22-28
    ModelSampling / TargetSampling / ModelAndTargetSampling    api/other/IcpProjectionDirection.scala:19-25
    ModelToTargetEvaluation / …            api/sampling/evaluators/EvaluationModeType.scala:20-26

Differences forced by the boundary: the Scalismo mesh decimations inside the reference's
constructors stay outside them — the default is `data.decimated_point_subset`, a stride over the vertex list;
`decimated_meshes` / `data.decimate` (icp_decimate_many: farthest points and their graph-distance cells, a
decimation of this library's own kind, not VTK's) give the points to pass as `decimatedTargetPoints=` —, and the
standard normals of `posterior.sample()` are passed in explicitly (`propose(theta, z)`).
"""
from __future__ import annotations

import ctypes as C
import itertools
import dataclasses
import math

import numpy as np

from . import _native as nat
from . import data as _data

# api/other/IcpProjectionDirection.scala:19-25
ModelSampling, TargetSampling, ModelAndTargetSampling = "ModelSampling", "TargetSampling", "ModelAndTargetSampling"
# api/sampling/evaluators/EvaluationModeType.scala:20-26
ModelToTargetEvaluation, TargetToModelEvaluation, SymmetricEvaluation = 0, 1, 2


def _d(a):
    return a.ctypes.data_as(nat.c_double_p)


def _i(a):
    return a.ctypes.data_as(nat.c_int_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


@dataclasses.dataclass(frozen=True)
class ModelFittingParameters:
    """Chain state: scale, pose (translation, Euler rotation, rotation centre), shape coefficients."""
    scale: float
    translation: tuple
    rotation: tuple
    rotation_center: tuple
    shape: tuple
    generatedBy: str = "Anonymous"

    @property
    def allParameters(self) -> np.ndarray:
        """ModelFittingParameters.scala:64 — [s | t | (phi,theta,psi) | centre | c]."""
        return np.asarray([self.scale, *self.translation, *self.rotation, *self.rotation_center, *self.shape],
                          dtype=np.float64)

    @classmethod
    def from_vector(cls, v, generatedBy="Anonymous"):
        v = np.asarray(v, dtype=np.float64)
        return cls(float(v[0]), tuple(v[1:4]), tuple(v[4:7]), tuple(v[7:10]), tuple(v[10:]), generatedBy)

    def copy_shape(self, shape, generatedBy):
        return dataclasses.replace(self, shape=tuple(np.asarray(shape, dtype=np.float64)), generatedBy=generatedBy)


def _theta(x) -> np.ndarray:
    return _f64(x.allParameters if isinstance(x, ModelFittingParameters) else x)


def initial_parameters(model) -> np.ndarray:
    """api/sampling/SamplingRegistration.scala:40-43: zero pose and shape, rotation centre = mean reference point."""
    theta = np.zeros(10 + model.rank)
    theta[0] = 1.0
    theta[7:10] = model.ref_points.sum(axis=0) * 1.0 / model.n_points
    return theta


_model_keys = itertools.count(1)


def _model_key(model) -> int:
    """icp_ctx_create_keyed's model_key: taken ONCE per model object — a content hash of the basis (xxhash, ≈ 10 ms for the face
    model's 137 MB) where that is importable, the object's number otherwise — so that the contexts of a batch registration (one per
    chain) do not each hash the basis again (6.6 ms per context).  The model's arrays are made read-only when the key is taken: a
    changed model is a new StatisticalMeshModel object (and a new key)."""
    arrays = (model.basis, model.variance, model.ref_points, model.mean_def, model.cells)
    where = tuple(a.__array_interface__["data"][0] for a in arrays)
    cached = getattr(model, "_icp_model_key", None)
    # (the key belongs to THESE arrays, frozen: a copy of the model object — copy.deepcopy carries the attribute along — or an array
    # swapped or made writeable again is hashed anew)
    if cached is not None and cached[1] == where and not any(a.flags.writeable for a in arrays):
        return cached[0]
    try:
        import xxhash
        hx = xxhash.xxh3_64()
        for arr in arrays[:4]:
            hx.update(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).data)
        key = (hx.intdigest() & 0xFFFFFFFFFFFFFFFF) or 1
    except Exception:
        key = (next(_model_keys) << 20) | 0x5A5A5
    try:
        # the key vouches for these arrays (icp_ctx_create_keyed: "equal keys mean equal arrays"): an in-place edit after this
        # point would silently meet the stale device copy, so the arrays are frozen — a changed model is a new object
        for arr in arrays:
            arr.flags.writeable = False
        model._icp_model_key = (key, where)
    except Exception:
        pass
    return key


def expect_contexts(device: int, n_contexts: int) -> None:
    """icp_ctx_expect: a host about to make n_contexts contexts on `device` (−1: LOCAL_RANK) lets their streams be made ahead."""
    nat.check(nat.lib().icp_ctx_expect(int(device), int(n_contexts)), "icp_ctx_expect")


class IcpContext:
    """One StatisticalMeshModel + one target TriangleMesh3D resident on one MI355X (icp_ctx)."""

    def __init__(self, model, target, device: int = -1):
        self.model, self.target = model, target
        L = nat.lib()
        md = nat.ModelDesc(model.n_points, model.cells.shape[0], model.rank, _d(model.ref_points), _d(model.mean_def),
                           _d(model.basis), _d(model.variance), _i(model.cells))
        td = nat.MeshDesc(target.n_points, target.n_cells, _d(target.points), _i(target.cells))
        h = C.c_void_p()
        nat.check(L.icp_ctx_create_keyed(C.byref(md), C.byref(td), device, _model_key(model), C.byref(h)), "icp_ctx_create_keyed")
        self.h = h
        self.rank, self.N = model.rank, model.n_points
        self._children = []  # weak references to the proposals / evaluators / chains created on this context

    def setTarget(self, target):
        """icp_ctx_set_target: the same context (model data, scratch, streams) against another target mesh; every proposal, evaluator
        and chain made on it for the old target is closed first."""
        for ref in reversed(getattr(self, "_children", [])):
            child = ref()
            if child is not None and getattr(child, "h", None):
                child.close()
        self._children = []
        td = nat.MeshDesc(target.n_points, target.n_cells, _d(target.points), _i(target.cells))
        nat.check(nat.lib().icp_ctx_set_target(self.h, C.byref(td)), "icp_ctx_set_target")
        self.target = target
        return self

    def _adopt(self, child):
        import weakref
        self._children.append(weakref.ref(child))

    def close(self):
        """Destroys the context — after every proposal, evaluator and chain that still lives on it (their native objects hold
        device buffers, pinned memory and events of this context: closing the context first would leak them)."""
        if getattr(self, "h", None):
            for ref in reversed(getattr(self, "_children", [])):
                child = ref()
                if child is not None and getattr(child, "h", None):
                    child.close()
            self._children = []
            nat.lib().icp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def runtime_stats(self) -> dict:
        """Fall-back counters of this context (icp_ctx_runtime_stats): all zero in a normal run."""
        return nat.runtime_stats(self.h)

    def step_paths(self) -> dict:
        """How many chain steps of this context took which path (icp_ctx_step_paths)."""
        return nat.step_paths(self.h)

    def twin_stats(self) -> dict:
        """Twin passes issued, second-lane results used and dropped (icp_ctx_twin_stats)."""
        return nat.twin_stats(self.h)

    def twin_eigen_stats(self) -> dict:
        """Second-lane decompositions started early, kept, cancelled by an accepted first lane, started cold (icp_ctx_twin_eigen_stats)."""
        return nat.twin_eigen_stats(self.h)

    def profile_start(self, max_launches: int = 200000, count_searches: bool = False):
        """count_searches: also count the tests the searches execute (rows "count.*" of profile_stop; slows the filter launches
        down — for a short leg of its own, not for timing)."""
        nat.check(nat.lib().icp_ctx_profile_search_counters(self.h, int(count_searches)), "icp_ctx_profile_search_counters")
        nat.check(nat.lib().icp_ctx_profile_start(self.h, max_launches), "icp_ctx_profile_start")

    def profile_stop(self):
        """-> {kernel name: dict(calls, total_ms, avg_us, min_us, max_us)} measured with HIP events on the context stream."""
        stats = (nat.KernelStat * 64)()
        n = C.c_int32()
        nat.check(nat.lib().icp_ctx_profile_stop(self.h, stats, 64, C.byref(n)), "icp_ctx_profile_stop")
        out = {}
        for i in range(n.value):
            s = stats[i]
            out[s.name.decode()] = dict(calls=s.calls, total_ms=s.total_ms, avg_us=1e3 * s.total_ms / max(s.calls, 1),
                                        min_us=1e3 * s.min_ms, max_us=1e3 * s.max_ms)
        return out

    def setRotation(self, angles, R=None):
        """icp_ctx_set_rotation: use the caller's rotation matrix (row-major 3x3, e.g. Scalismo's Rotation(phi, theta, psi)) for every
        theta whose Euler angles equal `angles`; R=None withdraws it."""
        a = _f64(angles).reshape(3)
        m = _f64(R).reshape(9) if R is not None else None
        nat.check(nat.lib().icp_ctx_set_rotation(self.h, _d(a), _d(m) if m is not None else None), "icp_ctx_set_rotation")

    def rotationConvention(self) -> dict:
        """icp_ctx_rotation_convention: how many matrices handed to setRotation agreed with the library's Rz·Ry·Rx (to rounding) and
        how many did not; with mismatched == 0 the on-device loop takes mixtures with pose walks for this context."""
        v, m = C.c_int64(0), C.c_int64(0)
        nat.check(nat.lib().icp_ctx_rotation_convention(self.h, C.byref(v), C.byref(m)), "icp_ctx_rotation_convention")
        return {"verified": v.value, "mismatched": m.value}

    def transformedMesh(self, theta) -> np.ndarray:
        """ModelFittingParameters.transformedMesh (ModelFittingParameters.scala:108-110) -> points [N,3]."""
        th = _theta(theta)
        out = np.empty((self.N, 3))
        nat.check(nat.lib().icp_transformed_mesh(self.h, _d(th), _d(out)), "icp_transformed_mesh")
        return out

    def coefficients(self, mesh, pose=None) -> np.ndarray:
        """Scalismo's model.coefficients(mesh) (σ² = 1e-5) of one mesh [N, 3]; `pose` ([s = 1 | t | angles | centre]): the rigid pose
        taken off first.  One item of model_coefficients."""
        return model_coefficients(self, meshes=[mesh], poses=[pose])[0]

    def project(self, mesh, pose=None) -> np.ndarray:
        """Scalismo's model.project(mesh): the instance of coefficients(mesh, pose), under `pose` where one was taken off -> [N, 3]."""
        return model_coefficients(self, meshes=[mesh], poses=[pose], want_project=True)[1][0]

    def posterior(self, vertex_ids, points, sigma2=None, covariances=None):
        """Scalismo's model.posterior(correspondences, noise) as a model (IcpBasedSurfaceFitting.scala:81 with sigma2,
        NonRigidIcpProposal.scala:152 with covariances [n, 3, 3]; NonRigidIcpProposal.scala:77): the model conditioned on the observed
        positions `points` [n, 3] (model space) of the vertices `vertex_ids` -> data.StatisticalMeshModel over the same reference and
        cells, which a new IcpContext accepts.  One item of posterior_models."""
        res = posterior_models(self, [vertex_ids], [points], sigma2=None if sigma2 is None else [sigma2],
                               covariances=None if covariances is None else [covariances], want=("mean", "basis", "variance"))[0]
        nat.check(res["status"], "icp_posterior_models_many")
        m = self.model
        return _data.StatisticalMeshModel(m.ref_points, m.cells, res["mean"], res["basis"], res["variance"])

    def vertexNormals(self, theta) -> np.ndarray:
        th = _theta(theta)
        out = np.empty((self.N, 3))
        nat.check(nat.lib().icp_vertex_normals(self.h, _d(th), _d(out)), "icp_vertex_normals")
        return out

    def closestPointOnTarget(self, pts):
        q = _f64(pts).reshape(-1, 3)
        n = q.shape[0]
        cp, tri, d2 = np.empty((n, 3)), np.empty(n, dtype=np.int32), np.empty(n)
        nat.check(nat.lib().icp_closest_point_on_target(self.h, n, _d(q), _d(cp), _i(tri), _d(d2)), "icp_closest_point_on_target")
        return cp, tri, d2

    def closestTargetVertex(self, pts):
        q = _f64(pts).reshape(-1, 3)
        n = q.shape[0]
        idx, d2 = np.empty(n, dtype=np.int32), np.empty(n)
        nat.check(nat.lib().icp_closest_target_vertex(self.h, n, _d(q), _i(idx), _d(d2)), "icp_closest_target_vertex")
        return idx, d2

    def closestModelVertex(self, theta, pts):
        th, q = _theta(theta), _f64(pts).reshape(-1, 3)
        n = q.shape[0]
        idx, d2 = np.empty(n, dtype=np.int32), np.empty(n)
        nat.check(nat.lib().icp_closest_model_vertex(self.h, _d(th), n, _d(q), _i(idx), _d(d2)), "icp_closest_model_vertex")
        return idx, d2

    def closestPointOnModel(self, theta, pts):
        th, q = _theta(theta), _f64(pts).reshape(-1, 3)
        n = q.shape[0]
        cp, tri, d2 = np.empty((n, 3)), np.empty(n, dtype=np.int32), np.empty(n)
        nat.check(nat.lib().icp_closest_point_on_model(self.h, _d(th), n, _d(q), _d(cp), _i(tri), _d(d2)), "icp_closest_point_on_model")
        return cp, tri, d2

    def distanceMap(self, theta, want=None) -> dict:
        """The per-vertex result of the registration theta against this context's target: one item of registration_maps."""
        m = registration_maps(self, _theta(theta)[None, :], want=_MAPS_WANT if want is None else want)[0]
        nat.check(int(m["status"]), "icp_registration_maps_many")
        return m


@dataclasses.dataclass
class IcpPosterior:
    corr_id: np.ndarray
    corr_aux: np.ndarray
    corr_point: np.ndarray
    keep: np.ndarray
    alpha: np.ndarray
    M: np.ndarray
    V: np.ndarray
    S: np.ndarray


class NonRigidIcpProposal:
    """NonRigidIcpProposal.scala:30-41.  `projectionDirection` is ModelSampling or TargetSampling.  `decimatedTargetPoints` defaults to
    data.decimated_point_subset(target, numOfSamplePoints); data.decimate(target, numOfSamplePoints).points is the opt-in alternative."""

    def __init__(self, ctx: IcpContext, stepLength: float, tangentialNoise: float, noiseAlongNormal: float,
                 numOfSamplePoints: int, projectionDirection=ModelSampling, boundaryAware: bool = True,
                 generatedBy: str = "ShapeIcpProposal", decimatedTargetPoints=None, numDecimatedModelPoints=None):
        self.ctx, self.stepLength, self.generatedBy = ctx, stepLength, generatedBy
        self.projectionDirection = projectionDirection
        if projectionDirection == TargetSampling:
            # :46 target.operations.decimate(numOfSamplePoints) — the caller's decimation outcome
            tp = _f64(decimatedTargetPoints if decimatedTargetPoints is not None
                      else _data.decimated_point_subset(ctx.target, numOfSamplePoints)).reshape(-1, 3)
            prm = nat.ProposalParams(stepLength, tangentialNoise, noiseAlongNormal, 1, int(boundaryAware), 0, tp.shape[0], _d(tp))
        elif projectionDirection == ModelSampling:
            # :45 model.decimate(numOfSamplePoints): only its point COUNT matters (:94-96)
            k = int(numDecimatedModelPoints if numDecimatedModelPoints is not None else min(numOfSamplePoints, ctx.N))
            prm = nat.ProposalParams(stepLength, tangentialNoise, noiseAlongNormal, 0, int(boundaryAware), k, 0, None)
        else:
            raise ValueError("a NonRigidIcpProposal samples one direction; mix two for ModelAndTargetSampling "
                             "(MixedProposalDistributions.scala:52-65)")
        h = C.c_void_p()
        nat.check(nat.lib().icp_proposal_create(ctx.h, C.byref(prm), C.byref(h)), "icp_proposal_create")
        self.h = h
        self.K = nat.lib().icp_proposal_num_candidates(h)
        ctx._adopt(self)

    def setSampler(self, sampler: str = "eigen"):
        """icp_proposal_set_sampler: "eigen" (default; Scalismo's posterior.sample(), parity with the reference for a given z) or
        "cholesky-root" (opt-in: the same distribution from W = D·L⁻ᵀ, no eigen-decomposition; ranks <= 64)."""
        kind = {"eigen": 0, "cholesky-root": 1}[sampler]
        nat.check(nat.lib().icp_proposal_set_sampler(self.h, kind), "icp_proposal_set_sampler")
        return self

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            nat.lib().icp_proposal_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def propose(self, theta, z, return_correspondences: bool = False):
        """:53-68.  z = the r standard normals `posterior.sample()` draws (:55)."""
        th, z = _theta(theta), _f64(z)
        out = np.empty_like(th)
        corr = np.empty(max(self.K, 1), dtype=np.int32)
        nat.check(nat.lib().icp_proposal_propose(self.h, _d(th), _d(z), _d(out), _i(corr)), "icp_proposal_propose")
        res = out
        if isinstance(theta, ModelFittingParameters):
            res = theta.copy_shape(out[10:], self.generatedBy)
        return (res, corr[:self.K]) if return_correspondences else res

    def logTransitionProbability(self, theta_from, theta_to) -> float:
        """:71-85 (−inf when anything but the shape differs)."""
        a, b = _theta(theta_from), _theta(theta_to)
        out = C.c_double()
        nat.check(nat.lib().icp_proposal_log_transition(self.h, _d(a), _d(b), C.byref(out)), "icp_proposal_log_transition")
        return out.value

    def icpPosterior(self, theta, with_aux: bool = True) -> IcpPosterior:
        """:88-153, diagnostic view."""
        th = _theta(theta)
        r, K = self.ctx.rank, max(self.K, 1)
        p = IcpPosterior(np.empty(K, dtype=np.int32), np.empty(K, dtype=np.int32), np.empty((K, 3)),
                         np.empty(K, dtype=np.uint8), np.empty(r), np.empty((r, r)), np.empty((r, r)), np.empty(r))
        view = nat.PosteriorView(0, _i(p.corr_id), _i(p.corr_aux) if with_aux else None, _d(p.corr_point),
                                 p.keep.ctypes.data_as(nat.c_ubyte_p), _d(p.alpha), _d(p.M), _d(p.V), _d(p.S))
        nat.check(nat.lib().icp_proposal_posterior(self.h, _d(th), C.byref(view)), "icp_proposal_posterior")
        k = view.n_candidates
        p.corr_id, p.corr_aux, p.corr_point, p.keep = p.corr_id[:k], p.corr_aux[:k], p.corr_point[:k], p.keep[:k]
        if not with_aux:
            p.corr_aux = np.full(k, -1, dtype=np.int32)
        return p


class _Evaluator:
    def __init__(self, ctx: IcpContext, kind, mode, n_model_ids, target_pts, gauss_mean, gauss_sigma, exp_rate):
        self.ctx = ctx
        tp = _f64(target_pts).reshape(-1, 3) if target_pts is not None else np.zeros((0, 3))
        prm = nat.EvaluatorParams(kind, mode, int(n_model_ids), tp.shape[0], _d(tp), gauss_mean, gauss_sigma, exp_rate)
        h = C.c_void_p()
        nat.check(nat.lib().icp_evaluator_create(ctx.h, C.byref(prm), C.byref(h)), "icp_evaluator_create")
        self.h = h
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            nat.lib().icp_evaluator_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def logValue(self, sample, return_aux: bool = False):
        th = _theta(sample)
        out = C.c_double()
        aux = np.zeros(4)
        nat.check(nat.lib().icp_evaluator_log_value(self.h, _d(th), C.byref(out), _d(aux)), "icp_evaluator_log_value")
        return (out.value, aux) if return_aux else out.value

    def bindChain(self, proposals):
        """icp_chain_bind: this evaluator and the chain's ICP proposals (in the mixture's order) form ONE Metropolis–Hastings chain
        driven method by method (Scalismo's MetropolisHastings.next, api/sampling/SamplingRegistration.scala:52-58): the first call of
        a step submits the whole step, the calls behind it find their values parked.  An empty list unbinds."""
        n = len(proposals)
        arr = (C.c_void_p * max(n, 1))(*[p.h for p in proposals])
        nat.check(nat.lib().icp_chain_bind(self.h, n, arr), "icp_chain_bind")

    def bindStats(self) -> dict:
        out = (C.c_int64 * 3)()
        nat.check(nat.lib().icp_chain_bind_stats(self.h, out), "icp_chain_bind_stats")
        return {"steps_from_propose": int(out[0]), "steps_from_log_value": int(out[1]), "parked_transition_hits": int(out[2])}


class AcceptAllEvaluator:
    """api/sampling/evaluators/AcceptAllEvaluator.scala:22-28 — logValue is the constant 0.0 whatever the sample (every proposal
    whose transition ratio allows it is accepted); no native call."""

    def logValue(self, sample) -> float:
        return 0.0


def _sides(ctx, numberOfPointsForComparison, decimatedTargetPoints, numDecimatedModelPoints):
    """the evaluators' two sides: `decimatedTargetPoints` defaults to data.decimated_point_subset(target, n); the points of
    data.decimate(target, n) are the opt-in alternative"""
    tp = (decimatedTargetPoints if decimatedTargetPoints is not None
          else _data.decimated_point_subset(ctx.target, numberOfPointsForComparison))
    k = int(numDecimatedModelPoints if numDecimatedModelPoints is not None else min(numberOfPointsForComparison, ctx.N))
    return k, tp


class IndependentPointDistanceEvaluator(_Evaluator):
    """IndependentPointDistanceEvaluator.scala:27-31; likelihoodModel = breeze Gaussian(mean, sigma)
    (ProductEvaluators.scala:39 uses Gaussian(0, uncertainty))."""

    def __init__(self, ctx, likelihoodMean: float, likelihoodSigma: float, evaluationMode, numberOfPointsForComparison: int,
                 decimatedTargetPoints=None, numDecimatedModelPoints=None):
        k, tp = _sides(ctx, numberOfPointsForComparison, decimatedTargetPoints, numDecimatedModelPoints)
        super().__init__(ctx, 0, evaluationMode, k, tp, likelihoodMean, likelihoodSigma, 1.0)


class HausdorffDistanceEvaluator(_Evaluator):
    """HausdorffDistanceEvaluator.scala:25-28; likelihoodModel = breeze Exponential(rate) (ProductEvaluators.scala:58)."""

    def __init__(self, ctx, likelihoodRate: float):
        super().__init__(ctx, 1, 2, 0, None, 0.0, 1.0, likelihoodRate)


class CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator(_Evaluator):
    """CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator.scala:27-32; likelihoodModelAvg = Gaussian(mean, sigma),
    likelihoodModelMax = Exponential(rate) (ProductEvaluators.scala:77-78)."""

    def __init__(self, ctx, avgMean: float, avgSigma: float, maxRate: float, evaluationMode, numberOfPointsForComparison: int,
                 decimatedTargetPoints=None, numDecimatedModelPoints=None):
        k, tp = _sides(ctx, numberOfPointsForComparison, decimatedTargetPoints, numDecimatedModelPoints)
        super().__init__(ctx, 2, evaluationMode, k, tp, avgMean, avgSigma, maxRate)


class ModelPriorEvaluator:
    """ModelPriorEvaluator.scala:24-31 — MultivariateNormalDistribution(0, I_rank).logpdf(shape coefficients)."""

    def __init__(self, rank: int):
        self.rank = rank

    def logValue(self, theta) -> float:
        th = _theta(theta)
        out = C.c_double()
        nat.check(nat.lib().icp_prior_log_value(self.rank, _d(th), C.byref(out)), "icp_prior_log_value")
        return out.value


def chain_eval_step(evaluator: _Evaluator, proposals, theta_cur, theta_prop):
    """icp_chain_eval_step: likelihood of theta_prop + forward/backward transition log-densities of every proposal,
    one device submission, one synchronisation."""
    a, b = _theta(theta_cur), _theta(theta_prop)
    n = len(proposals)
    arr = (C.c_void_p * max(n, 1))(*[p.h for p in proposals])
    val = C.c_double()
    fwd, bwd = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    nat.check(nat.lib().icp_chain_eval_step(evaluator.h, n, arr, _d(a), _d(b), C.byref(val), _d(fwd), _d(bwd)),
              "icp_chain_eval_step")
    return val.value, fwd[:n], bwd[:n]


def chain_step(evaluator: _Evaluator, proposals, theta_cur, generator: int = -1, z=None, theta_prop=None):
    """icp_chain_step: propose from proposals[generator] (or take theta_prop as given when generator < 0) AND evaluate the
    proposal — likelihood + forward/backward transition log-densities of every proposal — in one device submission.
    Returns (theta_prop, log_value, fwd, bwd)."""
    a = _theta(theta_cur)
    n = len(proposals)
    arr = (C.c_void_p * max(n, 1))(*[p.h for p in proposals])
    if generator >= 0:
        zz = np.ascontiguousarray(z, dtype=np.float64)
        b = np.zeros_like(a)
    else:
        zz = np.zeros(1)
        b = _theta(theta_prop).copy()
    val = C.c_double()
    fwd, bwd = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    nat.check(nat.lib().icp_chain_step(evaluator.h, n, arr, int(generator), _d(a), _d(zz), _d(b), C.byref(val), _d(fwd), _d(bwd)),
              "icp_chain_step")
    return b, val.value, fwd[:n], bwd[:n]


def chain_step_batched(evaluators, proposals, theta_cur, generator, z=None, theta_prop=None):
    """icp_chain_step_batched: chain_step for B independent chains (one context each) in one sequence of launches.
    evaluators[b], proposals[b] (list of n_props), theta_cur[b], generator[b]; z[b] where generator[b] >= 0, theta_prop[b]
    where generator[b] < 0.  Returns (theta_prop [B, 10+r], log_value [B], fwd [B, n], bwd [B, n], status [B])."""
    B = len(evaluators)
    n = len(proposals[0])
    cur = [_theta(t) for t in theta_cur]
    P = cur[0].shape[0]
    out = np.zeros((B, P))
    zs = []
    for b in range(B):
        if generator[b] >= 0:
            zs.append(np.ascontiguousarray(z[b], dtype=np.float64))
        else:
            zs.append(np.zeros(1))
            out[b] = _theta(theta_prop[b])
    ev = (C.c_void_p * B)(*[e.h for e in evaluators])
    pr = (C.c_void_p * max(B * n, 1))(*[p.h for ps in proposals for p in ps])
    gen = (C.c_int32 * B)(*[int(g) for g in generator])
    dp = nat.c_double_p
    curp = (dp * B)(*[_d(t) for t in cur])
    zp = (dp * B)(*[_d(t) for t in zs])
    outp = (dp * B)(*[_d(out[b]) for b in range(B)])
    val, fwd, bwd = np.zeros(B), np.zeros((B, max(n, 1))), np.zeros((B, max(n, 1)))
    status = (C.c_int32 * B)()
    rc = nat.lib().icp_chain_step_batched(B, ev, n, pr, gen, curp, zp, outp, _d(val), _d(fwd), _d(bwd), status)
    nat.check(rc, "icp_chain_step_batched")
    return out, val, fwd[:, :n], bwd[:, :n], np.array(list(status), dtype=np.int32)


class BatchedStepTicket:
    """icp_chain_step_batched_issue: a batch in flight.  collect() waits for it and returns what chain_step_batched returns;
    abandon() waits for its launches and drops the step.  Until then the member contexts refuse every other call (ICP_ERR_BUSY)."""

    def __init__(self, evaluators, proposals, theta_cur, generator, z=None, theta_prop=None, launch_ctx=None):
        B = len(evaluators)
        n = len(proposals[0])
        self._n = n
        self._keep = cur = [_theta(t) for t in theta_cur]
        self.out = np.zeros((B, cur[0].shape[0]))
        zs = []
        for b in range(B):
            if generator[b] >= 0:
                zs.append(np.ascontiguousarray(z[b], dtype=np.float64))
            else:
                zs.append(np.zeros(1))
                self.out[b] = _theta(theta_prop[b])
        self._zs = zs
        ev = (C.c_void_p * B)(*[e.h for e in evaluators])
        pr = (C.c_void_p * max(B * n, 1))(*[p.h for ps in proposals for p in ps])
        gen = (C.c_int32 * B)(*[int(g) for g in generator])
        dp = nat.c_double_p
        curp = (dp * B)(*[_d(t) for t in cur])
        zp = (dp * B)(*[_d(t) for t in zs])
        outp = (dp * B)(*[_d(self.out[b]) for b in range(B)])
        self.val, self.fwd, self.bwd = np.zeros(B), np.zeros((B, max(n, 1))), np.zeros((B, max(n, 1)))
        self.status = (C.c_int32 * B)()
        self._h = C.c_void_p()
        rc = nat.lib().icp_chain_step_batched_issue(B, ev, n, pr, gen, curp, zp, outp, _d(self.val), _d(self.fwd), _d(self.bwd), self.status,
                                                    launch_ctx.h if launch_ctx is not None else None, C.byref(self._h))
        nat.check(rc, "icp_chain_step_batched_issue")

    def collect(self):
        h, self._h = self._h, None
        nat.check(nat.lib().icp_chain_step_batched_collect(h), "icp_chain_step_batched_collect")
        return self.out, self.val, self.fwd[:, :self._n], self.bwd[:, :self._n], np.array(list(self.status), dtype=np.int32)

    def abandon(self):
        h, self._h = self._h, None
        if h:
            nat.check(nat.lib().icp_chain_step_batched_abandon(h), "icp_chain_step_batched_abandon")


def chain_step_prelaunch(evaluator: _Evaluator, proposals, theta_cur, generator: int = -1, z=None, theta_prop=None):
    """icp_chain_step_prelaunch: issue the first launches of the step that a later chain_step with exactly these arguments
    will ask for (typically: the next step under the assumption that the step in flight is rejected).  Never changes
    results; proposals == [] drops a pending half step."""
    n = len(proposals)
    if n == 0:
        nat.check(nat.lib().icp_chain_step_prelaunch(evaluator.h, 0, None, -1, None, None), "icp_chain_step_prelaunch")
        return
    a = _theta(theta_cur)
    arr = (C.c_void_p * n)(*[p.h for p in proposals])
    key = np.ascontiguousarray(z, dtype=np.float64) if generator >= 0 else _theta(theta_prop)
    nat.check(nat.lib().icp_chain_step_prelaunch(evaluator.h, n, arr, int(generator), _d(a), _d(key)), "icp_chain_step_prelaunch")


def chain_step_prelaunch2(evaluator: _Evaluator, proposals, theta_cur, generator: int, key, generator2: int, key2) -> int:
    """icp_chain_step_prelaunch2: the next step and the one after it, both from theta_cur, as the two lanes of one set of launches
    (key / key2: z where the generator is >= 0, the proposed state otherwise).  -> lanes issued (0, 1 or 2)."""
    n = len(proposals)
    a = _theta(theta_cur)
    arr = (C.c_void_p * n)(*[p.h for p in proposals])
    k1 = np.ascontiguousarray(key, dtype=np.float64)
    k2 = np.ascontiguousarray(key2, dtype=np.float64)
    lanes = C.c_int32(0)
    nat.check(nat.lib().icp_chain_step_prelaunch2(evaluator.h, n, arr, int(generator), _d(a), _d(k1), int(generator2), _d(k2), C.byref(lanes)),
              "icp_chain_step_prelaunch2")
    return int(lanes.value)


def direction_schedule(n_fits: int, n_recursions: int, seed) -> np.ndarray:
    """ModelAndTargetSampling's per-recursion draw (api/other/IcpBasedSurfaceFitting.scala:63-69): ModelSampling (0) or
    TargetSampling (1) with probability 1/2 each, [n_fits, n_recursions] uint8 from np.random.default_rng(seed).  The reference
    draws from the unseeded global scala.util.Random, so only the distribution of the directions is the reference's; the
    draw of one fit is not (per-fit equality with Scalismo is not defined)."""
    if seed is None:
        raise ValueError("ModelAndTargetSampling without a directions schedule needs a seed")
    if n_fits < 0 or n_recursions < 0:
        raise ValueError("negative size")
    return np.random.default_rng(seed).integers(0, 2, size=(int(n_fits), int(n_recursions))).astype(np.uint8)


def _direction_code(direction) -> int:
    if direction in (ModelSampling, 0):
        return 0
    if direction in (TargetSampling, 1):
        return 1
    raise ValueError(f"unknown projection direction {direction!r}")


def _per_item(contexts, n, what="item", empty_ok=False):
    """The contexts of a batched call: one per item, or one for all; at most 65,535 items."""
    ctxs = list(contexts) if isinstance(contexts, (list, tuple)) else [contexts] * n
    if empty_ok:
        if len(ctxs) != n:
            raise ValueError(f"one context per {what} (or one for all)")
    elif n == 0 or len(ctxs) != n:
        raise ValueError(f"one context per {what} (or one for all) and at least one {what}")
    if n > 65535:
        raise ValueError(f"at most 65,535 {what}s a call")
    return ctxs


def _ptr_array(arrays, ptype=nat.c_double_p, conv=_d):
    """A ctypes array of one pointer per entry (None: a null pointer): `conv` makes a `ptype` of an entry."""
    return (ptype * max(len(arrays), 1))(*[conv(a) if a is not None else None for a in arrays])


def _ctx_array(ctxs):
    return (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])


def icp_fits(contexts, theta_inits, numIterations: int, iterationSeq=(1.0, 0.1, 0.01), projectionDirection=ModelSampling,
             modelPointIds=None, targetPointSamples=None, stepLength: float = 1.0, directions=None, seed=None):
    """Many deterministic ICP fits (IcpBasedSurfaceFitting.runfitting, api/other/IcpBasedSurfaceFitting.scala:46-126) in one call
    (icp_fit_deterministic_many): fit b starts at theta_inits[b] on contexts[b] (one context, or one per fit; the fits of one
    target may share its context).  `targetPointSamples` is one array for every fit or one per fit.
    Directions: ModelSampling / TargetSampling for every recursion, or ModelAndTargetSampling — a fresh draw per recursion as the
    reference makes it (:63-69): `directions` ([n_fits, len(iterationSeq)·(numIterations+1)] of 0 / 1) if given, else drawn by
    direction_schedule(…, seed) (seed required).  The reference draws from the unseeded global scala.util.Random: per-fit equality
    with Scalismo is not defined, only the distribution of the directions.
    Returns (thetas [n_fits, 10+r], status [n_fits]): status 0, or ICP_ERR_NOT_SPD (-4) / ICP_ERR_NOT_FINITE (-3) for that fit
    alone (its row is then theta_init).  Argument errors raise before anything runs."""
    th = _f64(theta_inits)
    if th.ndim != 2:
        raise ValueError("theta_inits must be [n_fits, 10 + rank]")
    n = th.shape[0]
    ctxs = _per_item(contexts, n, "fit")
    r = ctxs[0].rank
    if th.shape[1] != 10 + r or any(c.rank != r for c in ctxs):
        raise ValueError("theta_inits and the contexts' rank disagree")
    sig = _f64(iterationSeq).reshape(-1)
    if numIterations < 0:
        raise ValueError("numIterations must be >= 0")
    R = sig.shape[0] * (int(numIterations) + 1)
    if directions is not None:
        dirs = np.ascontiguousarray(directions, dtype=np.uint8)
        if dirs.shape != (n, R):
            raise ValueError(f"directions must be [{n}, {R}]")
    elif projectionDirection in (ModelAndTargetSampling, 2):
        dirs = direction_schedule(n, R, seed)
    else:
        dirs = None
    ids = np.ascontiguousarray(modelPointIds if modelPointIds is not None else np.zeros(0), dtype=np.int32).reshape(-1)
    if targetPointSamples is None:
        tps = [np.zeros((0, 3))] * n
    elif isinstance(targetPointSamples, (list, tuple)):
        tps = [_f64(t).reshape(-1, 3) for t in targetPointSamples]
    else:
        tps = [_f64(targetPointSamples).reshape(-1, 3)] * n
    if len(tps) != n:
        raise ValueError("targetPointSamples: one array, or one per fit")
    code = _direction_code(projectionDirection) if dirs is None else 0
    fps = [nat.FitParams(code, ids.shape[0], _i(ids), tp.shape[0], _d(tp), float(stepLength)) for tp in tps]
    out = th.copy()
    status = np.zeros(n, dtype=np.int32)
    c_fp = _ptr_array(fps, C.POINTER(nat.FitParams), C.pointer)
    c_dirs = dirs.ctypes.data_as(nat.c_ubyte_p) if dirs is not None else None
    rc = nat.lib().icp_fit_deterministic_many(n, _ctx_array(ctxs), c_fp, _ptr_array(list(th)), c_dirs, int(numIterations), sig.shape[0],
                                              _d(sig), _ptr_array(list(out)), _i(status))
    if rc not in (0, -3, -4) or (rc != 0 and not np.any(status != 0)):
        nat.check(rc, "icp_fit_deterministic_many")
    return out, status


class IcpBasedSurfaceFitting:
    """api/other/IcpBasedSurfaceFitting.scala:32 — the deterministic non-rigid ICP baseline (posterior MEAN, isotropic noise).
    `modelPointIds` / `targetPointSamples` stand for the UniformMeshSampler3D draws of :51-53 (made by the caller: data.fit_samples draws them on the device).
    ModelAndTargetSampling draws the direction afresh for every recursion (:63-69); here from np.random.default_rng(seed)
    (direction_schedule) — the reference draws from the unseeded global scala.util.Random, so only the distribution of the
    directions is the reference's, not one fit's draw."""

    def __init__(self, ctx: IcpContext, stepLength: float = 1.0, projectionDirection=ModelSampling, modelPointIds=None,
                 targetPointSamples=None, seed=1024):
        self.ctx, self.step = ctx, float(stepLength)
        self.mixed = projectionDirection in (ModelAndTargetSampling, 2)
        self.direction = 1 if projectionDirection in (TargetSampling, "TargetSampling", 1) else 0
        self.seed = seed
        self.ids = np.ascontiguousarray(modelPointIds if modelPointIds is not None else np.zeros(0), dtype=np.int32)
        self.tp = _f64(targetPointSamples if targetPointSamples is not None else np.zeros((0, 3))).reshape(-1, 3)

    def runfitting(self, numIterations: int, iterationSeq=(1.0, 0.1, 0.01), initialModelParameters=None) -> np.ndarray:
        """:46-126; returns the final parameter vector (the reference returns the corresponding mesh: ctx.transformedMesh)."""
        th = _theta(initialModelParameters if initialModelParameters is not None else initial_parameters(self.ctx.model))
        sig = _f64(iterationSeq)
        if self.mixed:  # one fit through icp_fit_deterministic_many with a seeded schedule
            out, status = icp_fits(self.ctx, th[None, :], numIterations, sig, ModelAndTargetSampling, self.ids, self.tp, self.step,
                                   seed=self.seed)
            nat.check(int(status[0]), "icp_fit_deterministic_many")
            return out[0]
        out = np.zeros_like(th)
        fp = nat.FitParams(self.direction, self.ids.shape[0], _i(self.ids), self.tp.shape[0], _d(self.tp), self.step)
        nat.check(nat.lib().icp_fit_deterministic(self.ctx.h, C.byref(fp), _d(th), int(numIterations), sig.shape[0], _d(sig), _d(out)),
                  "icp_fit_deterministic")
        return out


def posterior_variability(ctx: IcpContext, thetas, mode: int = 0, theta_ref=None) -> np.ndarray:
    """apps/util/PosteriorVariability.scala:30-73 over logged chain states: per-vertex total variance (mode 0), variance along the
    normals of theta_ref's mesh (1) or along the mean sample normal (2)."""
    th = _f64(thetas).reshape(-1, 10 + ctx.rank)
    ref = _theta(theta_ref if theta_ref is not None else th[0])
    out = np.zeros(ctx.model.n_points)
    nat.check(nat.lib().icp_posterior_variability(ctx.h, th.shape[0], _d(th), int(mode), _d(ref), _d(out)), "icp_posterior_variability")
    return out


def posterior_variability_maps(contexts, sample_sets, mode=0, theta_refs=None, want_mean: bool = False):
    """The variability maps of many chains' samples in one call (icp_posterior_variability_many): map m is
    posterior_variability(contexts[m], sample_sets[m], mode[m], theta_refs[m]), bit for bit.  `contexts`: one context or one per map
    (they may repeat and differ in model and rank; one device); `sample_sets`: per map an array [S_m, 10 + rank] with S_m >= 2;
    `mode`: one int or one per map; `theta_refs`: per map the state whose mesh gives mode 1's normals (None elsewhere).  The sample
    meshes stream through a fixed 64 MiB buffer on the device, so S_m may be every state of a long chain.  Returns the list of [N_m]
    maps; with want_mean also the list of [N_m, 3] mean sample meshes."""
    sets = list(sample_sets)
    n = len(sets)
    ctxs = _per_item(contexts, n, "map", empty_ok=True)
    modes = [int(v) for v in mode] if isinstance(mode, (list, tuple, np.ndarray)) else [int(mode)] * n
    if len(modes) != n:
        raise ValueError("one mode per map (or one for all)")
    refs = list(theta_refs) if theta_refs is not None else [None] * n
    if len(refs) != n:
        raise ValueError("one theta_ref per map")
    th, rf = [], []
    for m in range(n):
        a = _f64(sets[m])
        if a.ndim != 2 or a.shape[1] != 10 + ctxs[m].rank:
            raise ValueError(f"map {m}: samples must be [S, 10 + rank]")
        if a.shape[0] < 2:
            raise ValueError(f"map {m}: at least two samples are needed")
        if modes[m] not in (0, 1, 2):
            raise ValueError(f"map {m}: unknown mode {modes[m]}")
        if modes[m] == 1 and refs[m] is None:
            raise ValueError(f"map {m}: mode 1 needs a theta_ref")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"map {m}: samples contain a non-finite value")
        ref = None
        if modes[m] == 1:
            ref = _f64(refs[m]).reshape(-1)
            if ref.shape[0] != 10 + ctxs[m].rank or not np.all(np.isfinite(ref)):
                raise ValueError(f"map {m}: theta_ref must be 10 + rank finite values")
        th.append(a)
        rf.append(ref)
    outs = [np.zeros(c.N) for c in ctxs]
    means = [np.zeros((c.N, 3)) for c in ctxs] if want_mean else None
    if n > 0:
        c_n = np.array([a.shape[0] for a in th], dtype=np.int32)
        c_mode = np.array(modes, dtype=np.int32)
        c_mean = _ptr_array(means) if want_mean else None
        nat.check(nat.lib().icp_posterior_variability_many(n, _ctx_array(ctxs), _i(c_n), _ptr_array(th), _i(c_mode), _ptr_array(rf),
                                                           _ptr_array(outs), c_mean), "icp_posterior_variability_many")
    return (outs, means) if want_mean else outs


def evaluate_reconstruction_to_ground_truth(ctx: IcpContext, theta) -> dict:
    """api/other/RegistrationComparison.scala:24-49 for the mesh of theta against the context's target."""
    out = np.zeros(5)
    nat.check(nat.lib().icp_mesh_metrics(ctx.h, _d(_theta(theta)), _d(out)), "icp_mesh_metrics")
    return {"average2surface": out[0], "hausdorff": out[1], "average2surface_boundary_aware": out[2], "max_boundary_aware": out[3],
            "kept": int(out[4])}


MAX_DICE_SAMPLES = 1 << 24


def registration_metrics(contexts, thetas, dice_samples: int = 10000, seed: int = 1024) -> dict:
    """The experiment summary's distance measures (apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:43-64) of many meshes
    in one call (icp_mesh_metrics_many): item b scores the mesh of thetas[b] against the target of contexts[b] (one context, or one
    per item; contexts may repeat).  Returns arrays of n_items keyed "avg", "hausdorff", "dice", "average2surface_boundary_aware",
    "max_boundary_aware", "kept", "n_inside_reconstruction", "n_inside_target", "n_inside_both".  avg / hausdorff / the
    boundary-aware pair / kept are the bits of evaluate_reconstruction_to_ground_truth.  Dice: MeshMetrics.diceCoefficient as
    recalled [SCALISMO-UNVERIFIED] — dice_samples points uniform in the union of the two boxes, drawn from orc_rng_uniform(seed, s, k),
    each classified by the vertex normal of its nearest vertex (include/icp_proposal.h); meaningful for closed meshes only.
    dice_samples = 0 skips it (NaN).  An item whose mesh is not finite has NaN everywhere and "status" != 0."""
    th = _f64(thetas)
    if th.ndim == 1:
        th = th[None, :]
    if th.ndim != 2:
        raise ValueError("thetas must be [n_items, 10 + rank]")
    n = th.shape[0]
    ctxs = _per_item(contexts, n)
    r = ctxs[0].rank
    if th.shape[1] != 10 + r or any(c.rank != r for c in ctxs):
        raise ValueError("thetas and the contexts' rank disagree")
    if not np.all(np.isfinite(th)):
        raise ValueError("thetas contain a non-finite value")
    dice_samples = int(dice_samples)
    if not 0 <= dice_samples <= MAX_DICE_SAMPLES:
        raise ValueError(f"dice_samples must lie in [0, {MAX_DICE_SAMPLES}]")
    seed = int(seed)
    if not 0 <= seed < (1 << 64):
        raise ValueError("seed must be an unsigned 64-bit integer")
    out = np.zeros((n, 9))
    status = np.zeros(n, dtype=np.int32)
    rc = nat.lib().icp_mesh_metrics_many(n, _ctx_array(ctxs), _ptr_array(list(th)), dice_samples, seed, _d(out), _i(status))
    if rc not in (0, -3) or (rc != 0 and not np.any(status != 0)):
        nat.check(rc, "icp_mesh_metrics_many")
    return {"avg": out[:, 0].copy(), "hausdorff": out[:, 1].copy(), "dice": out[:, 5].copy(),
            "average2surface_boundary_aware": out[:, 2].copy(), "max_boundary_aware": out[:, 3].copy(), "kept": out[:, 4].copy(),
            "n_inside_reconstruction": out[:, 6].copy(), "n_inside_target": out[:, 7].copy(), "n_inside_both": out[:, 8].copy(),
            "status": status}


def dice_coefficient(ctx: IcpContext, theta, samples: int = 10000, seed: int = 1024) -> float:
    """MeshMetrics.diceCoefficient(mesh of theta, ctx's target) [SCALISMO-UNVERIFIED], one item of registration_metrics."""
    m = registration_metrics(ctx, _theta(theta)[None, :], samples, seed)
    nat.check(int(m["status"][0]), "icp_mesh_metrics_many")
    return float(m["dice"][0])


_MAPS_WANT = ("m2t_point", "m2t_triangle", "m2t_distance", "m2t_on_boundary", "t2m_point", "t2m_triangle", "t2m_distance")
_SUMMARY_WANT = ("m2t_mean", "m2t_max", "t2m_mean", "t2m_max")


def _ubyte_p(a):
    return a.ctypes.data_as(nat.c_ubyte_p)


def _want(want, known):
    want = tuple(want)
    if not want:
        raise ValueError(f"ask for at least one output of {known}")
    for w in want:
        if w not in known:
            raise ValueError(f"unknown output {w!r}: one of {known}")
    return want


def _rows_of(block, counts, width):
    """Per-item views [count, width] (width 0: [count]) of one contiguous block: the items' rows lie side by side in memory."""
    views, at = [], 0
    for k in counts:
        views.append(block[at:at + k * max(width, 1)].reshape((k, width) if width else (k,)))
        at += k * max(width, 1)
    return views


def registration_maps(contexts, thetas, want=_MAPS_WANT) -> list:
    """The per-vertex result of many registrations in one call (icp_registration_maps_many): item b is the mesh of thetas[b] against
    the target of contexts[b] (one context, or one per item; contexts may repeat, one model).  `want` names the outputs to fetch; a
    direction none of whose outputs is wanted is not searched.  Returns one dict per item with "status" (0, or -3 for a mesh that is
    not finite: NaN rows, triangles -1, flags 0) and the wanted ones of
      "m2t_point" [N, 3], "m2t_triangle" [N], "m2t_distance" [N]: closestPointOnTarget(transformedMesh(theta)) and sqrt of its
        squared distances — the colour-coded distance map of a fit, a dense correspondence set for posterior_models;
      "m2t_on_boundary" [N] uint8: the nearest target vertex of that point is a boundary vertex of the target
        (RegistrationComparison.scala:31-42; all 0 for a closed target);
      "t2m_point" [M, 3], "t2m_triangle" [M], "t2m_distance" [M]: closestPointOnModel(theta, target vertices), likewise.
    The arrays of one output are views of one block, item after item."""
    th = _f64(thetas)
    if th.ndim == 1:
        th = th[None, :]
    if th.ndim != 2:
        raise ValueError("thetas must be [n_items, 10 + rank]")
    n = th.shape[0]
    ctxs = _per_item(contexts, n)
    r = ctxs[0].rank
    if th.shape[1] != 10 + r or any(c.rank != r for c in ctxs):
        raise ValueError("thetas and the contexts' rank disagree")
    if not np.all(np.isfinite(th)):
        raise ValueError("thetas contain a non-finite value")
    want = _want(want, _MAPS_WANT)
    spec = {"m2t_point": (np.float64, 3, nat.c_double_p, _d), "m2t_triangle": (np.int32, 0, nat.c_int_p, _i),
            "m2t_distance": (np.float64, 0, nat.c_double_p, _d), "m2t_on_boundary": (np.uint8, 0, nat.c_ubyte_p, _ubyte_p),
            "t2m_point": (np.float64, 3, nat.c_double_p, _d), "t2m_triangle": (np.int32, 0, nat.c_int_p, _i),
            "t2m_distance": (np.float64, 0, nat.c_double_p, _d)}
    rows, args = {}, []
    for w in _MAPS_WANT:
        if w not in want:
            args.append(None)
            continue
        dtype, width, ptype, conv = spec[w]
        counts = [c.N if w.startswith("m2t") else c.target.n_points for c in ctxs]
        rows[w] = _rows_of(np.zeros(sum(counts) * max(width, 1), dtype=dtype), counts, width)
        args.append(_ptr_array(rows[w], ptype, conv))
    status = np.zeros(n, dtype=np.int32)
    rc = nat.lib().icp_registration_maps_many(n, _ctx_array(ctxs), _ptr_array(list(th)), *args, _i(status))
    if rc not in (0, -3) or (rc != 0 and not np.any(status != 0)):
        nat.check(rc, "icp_registration_maps_many")
    out = []
    for b in range(n):
        item = {w: rows[w][b] for w in want}
        item["status"] = int(status[b])
        out.append(item)
    return out


def distance_summaries(contexts, sample_sets, want=_SUMMARY_WANT) -> list:
    """The distance maps many chains' samples imply, in one call (icp_distance_summaries_many): set m holds the states sample_sets[m]
    ([S_m, 10 + rank], S_m >= 1) on contexts[m] (one context, or one per set).  Per vertex, "m2t_mean" / "t2m_mean" are the
    registration_maps distances of the set's states added left to right in sample order and divided once by S_m, "m2t_max" /
    "t2m_max" their maximum: where the posterior stays off the target, beside posterior_variability_maps' where it is wide.  The
    per-state maps never leave the device.  Returns one dict per set: the wanted arrays ([N] / [M]) and "status" (0, or -3 for a set
    with a sample whose mesh is not finite: NaN rows)."""
    sets = [_f64(a) for a in sample_sets]
    n = len(sets)
    ctxs = _per_item(contexts, n, "set")
    r = ctxs[0].rank
    for m, a in enumerate(sets):
        if a.ndim != 2 or a.shape[1] != 10 + r or ctxs[m].rank != r:
            raise ValueError(f"set {m}: samples must be [S, 10 + rank] of the contexts' one rank")
        if a.shape[0] < 1:
            raise ValueError(f"set {m}: at least one sample")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"set {m}: samples contain a non-finite value")
    want = _want(want, _SUMMARY_WANT)
    rows, args = {}, []
    for w in _SUMMARY_WANT:
        if w not in want:
            args.append(None)
            continue
        counts = [c.N if w.startswith("m2t") else c.target.n_points for c in ctxs]
        rows[w] = _rows_of(np.zeros(sum(counts)), counts, 0)
        args.append(_ptr_array(rows[w]))
    status = np.zeros(n, dtype=np.int32)
    c_n = np.array([a.shape[0] for a in sets], dtype=np.int32)
    rc = nat.lib().icp_distance_summaries_many(n, _ctx_array(ctxs), _i(c_n), _ptr_array(sets), *args, _i(status))
    if rc not in (0, -3) or (rc != 0 and not np.any(status != 0)):
        nat.check(rc, "icp_distance_summaries_many")
    out = []
    for m in range(n):
        item = {w: rows[w][m] for w in want}
        item["status"] = int(status[m])
        out.append(item)
    return out


def log_values(evaluators, thetas, return_aux: bool = False) -> dict:
    """The log values of many states under many evaluators in one call (icp_evaluator_log_values_many): item b is
    evaluators[b].logValue(thetas[b], return_aux=True) of a fresh evaluator bit for bit — re-scoring a chain's log under another
    likelihood, or under every named evaluator as the reference's logger does (JSONAcceptRejectLogger.scala:84-106).  `evaluators`:
    one evaluator or one per item; they may repeat, differ in kind, mode and parameters and belong to contexts of different targets
    (one device, one model).  `thetas`: [n_items, 10 + rank].  Returns {"value": [n], "aux": [n, 4] (None without return_aux),
    "status": [n]}: status 0, or -5 for an item whose boundary-aware evaluator dropped every point (its value is NaN); any other
    per-item failure raises.  The evaluators and their chains are left as they were."""
    th = _f64(thetas)
    if th.ndim == 1:
        th = th[None, :]
    if th.ndim != 2:
        raise ValueError("thetas must be [n_items, 10 + rank]")
    n = th.shape[0]
    evs = _per_item(evaluators, n, what="evaluator")
    r = evs[0].ctx.rank
    if th.shape[1] != 10 + r or any(e.ctx.rank != r for e in evs):
        raise ValueError("thetas and the evaluators' rank disagree")
    if not np.all(np.isfinite(th)):
        raise ValueError("thetas contain a non-finite value")
    value = np.zeros(n)
    aux = np.zeros((n, 4)) if return_aux else None
    status = np.zeros(n, dtype=np.int32)
    rc = nat.lib().icp_evaluator_log_values_many(n, _ctx_array(evs), _ptr_array(list(th)), _d(value), _d(aux) if return_aux else None,
                                                 _i(status))
    nat.check(rc, "icp_evaluator_log_values_many")
    return {"value": value, "aux": aux, "status": status}



def transformed_meshes(contexts, thetas) -> np.ndarray:
    """ModelFittingParameters.transformedMesh of many states in one call (icp_model_instances_many): row b is
    contexts[b].transformedMesh(thetas[b]) bit for bit, pose and registered rotation matrices included.  `contexts`: one context or
    one per item (they may repeat and differ in target, model and rank; the models of one call have one vertex count, so that the
    result is one array [n, N, 3] — ReplayFittingFromLog's and RandomSamplesFromModel's loops over logged states); `thetas`:
    [n, 10 + rank] or a list of states."""
    th = [_f64(t).reshape(-1) for t in thetas]
    ctxs = _per_item(contexts, len(th))
    N = ctxs[0].N
    for b, (c, t) in enumerate(zip(ctxs, th)):
        if t.shape[0] != 10 + c.rank:
            raise ValueError(f"item {b}: a state has 10 + rank values")
        if c.N != N:
            raise ValueError(f"item {b}: the contexts' models differ in their vertex count")
        if not np.all(np.isfinite(t)):
            raise ValueError(f"item {b}: theta contains a non-finite value")
    n = len(th)
    out = np.empty((n, N, 3))
    nat.check(nat.lib().icp_model_instances_many(n, _ctx_array(ctxs), _ptr_array(th), _ptr_array(list(out))), "icp_model_instances_many")
    return out


def model_coefficients(contexts, meshes=None, thetas=None, poses=None, want_project: bool = False):
    """Scalismo's model.coefficients(mesh) — and model.project(mesh) — of many meshes in one call (icp_model_coefficients_many):
    c = (QᵀQ + σ²I)⁻¹ Qᵀ(x − x̄ − μ), σ² = 1e-5, as NonRigidIcpProposal.scala:59 and IcpBasedSurfaceFitting.scala:84 use it.
    `contexts`: one context or one per item, all of ONE model.  Item b's mesh is meshes[b] ([N, 3], the model's vertex order) or the
    transformedMesh of thetas[b] (instanced on the device): give `meshes`, or `thetas`, or both as lists with None where the other
    one holds the item.  `poses`: None, or per item None or [s | t | angles | centre] with s exactly 1 — the rigid pose taken off the
    vertices first (a chain state's theta[:10]); without one the mesh is taken to be in model space.  Returns the coefficients
    [n, rank]; with want_project also the projections [n, N, 3] (the instance of c, under the item's pose where one was taken off:
    the bits of transformedMesh([pose or identity | c])).  An item with a non-finite vertex raises IcpNativeError (-3)."""
    ms = list(meshes) if meshes is not None else None
    ts = list(thetas) if thetas is not None else None
    if ms is None and ts is None:
        raise ValueError("give meshes, thetas, or both")
    n = len(ms) if ms is not None else len(ts)
    if ts is not None and len(ts) != n:
        raise ValueError("meshes and thetas must have one entry per item")
    ctxs = _per_item(contexts, n)
    ps = list(poses) if poses is not None else [None] * n
    if len(ps) != n:
        raise ValueError("one pose per item (None where there is none)")
    r, N = ctxs[0].rank, ctxs[0].N
    pts, th, po = [], [], []
    for b in range(n):
        if ctxs[b].rank != r or ctxs[b].N != N:
            raise ValueError(f"item {b}: the items of one call share a model")
        m = ms[b] if ms is not None else None
        t = ts[b] if ts is not None else None
        if (m is None) == (t is None):
            raise ValueError(f"item {b}: a mesh or a theta, one of the two")
        if m is not None:
            m = _f64(m)
            if m.size != 3 * N:
                raise ValueError(f"item {b}: a mesh has the model's {N} vertices")
            m = m.reshape(N, 3)
        else:
            t = _f64(t).reshape(-1)
            if t.shape[0] != 10 + r or not np.all(np.isfinite(t)):
                raise ValueError(f"item {b}: theta must be 10 + rank finite values")
        p = ps[b]
        if p is not None:
            p = _f64(p).reshape(-1)
            if p.shape[0] != 10 or not np.all(np.isfinite(p)):
                raise ValueError(f"item {b}: a pose is 10 finite values [s | t | angles | centre]")
            if p[0] != 1.0:
                raise ValueError(f"item {b}: the scale of a pose to take off must be exactly 1")
        pts.append(m)
        th.append(t)
        po.append(p)
    coeffs = np.zeros((n, r))
    proj = np.zeros((n, N, 3)) if want_project else None
    status = np.zeros(n, dtype=np.int32)
    c_proj = _ptr_array(list(proj)) if want_project else None
    rc = nat.lib().icp_model_coefficients_many(n, _ctx_array(ctxs), _ptr_array(pts), _ptr_array(th), _ptr_array(po), _d(coeffs), c_proj,
                                               _i(status))
    nat.check(rc, "icp_model_coefficients_many")
    return (coeffs, proj) if want_project else coeffs


_POSTERIOR_WANT = ("alpha", "mean", "basis", "variance", "point_variance")


def posterior_models(contexts, vertex_ids, points, sigma2=None, covariances=None, want=_POSTERIOR_WANT):
    """Posterior shape models of many sets of correspondences in one call (icp_posterior_models_many): item b conditions
    contexts[b]'s model on the observed positions points[b] ([n_b, 3], model space) of its vertices vertex_ids[b] ([n_b], repeats
    allowed), with the noise in exactly one of two forms per item — sigma2[b] (one positive number, isotropic:
    IcpBasedSurfaceFitting.scala:81) or covariances[b] ([n_b, 3, 3] symmetric positive definite: NonRigidIcpProposal.scala:152);
    `sigma2` / `covariances` are None or lists with None where the other one holds the item.  `contexts`: one context or one per item
    (they may repeat and differ in model and rank).  `want` names the outputs to fetch.  Returns one dict per item: "status" (0, or −3
    for a covariance that is not positive definite — that item's arrays are NaN —, or −1 for a rank above 256 — its arrays are
    absent) and the wanted ones of "alpha" [r], "mean" [N, 3] (the posterior model's mean deformation μ + Q·α), "basis" [3N, r]
    (Φ·V, unscaled), "variance" [r] (descending), "point_variance" [N] (trace of every vertex's 3 × 3 posterior covariance)."""
    ids = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in vertex_ids]
    n = len(ids)
    ctxs = _per_item(contexts, n)
    pts = list(points)
    s2 = list(sigma2) if sigma2 is not None else [None] * n
    cov = list(covariances) if covariances is not None else [None] * n
    if len(pts) != n or len(s2) != n or len(cov) != n:
        raise ValueError("vertex_ids, points and the noise have one entry per item")
    want = tuple(want)
    for w in want:
        if w not in _POSTERIOR_WANT:
            raise ValueError(f"unknown output {w!r}: one of {_POSTERIOR_WANT}")
    p_arr, s_arr, c_arr = [], [], []
    for b in range(n):
        k = ids[b].shape[0]
        if k < 1:
            raise ValueError(f"item {b}: at least one observation")
        if ids[b].min() < 0 or ids[b].max() >= ctxs[b].N:
            raise ValueError(f"item {b}: vertex id out of range")
        p = _f64(pts[b])
        if p.size != 3 * k:
            raise ValueError(f"item {b}: one observed position [3] per vertex id")
        if not np.all(np.isfinite(p)):
            raise ValueError(f"item {b}: points contain a non-finite value")
        if (s2[b] is None) == (cov[b] is None):
            raise ValueError(f"item {b}: the noise is sigma2 or covariances, one of the two")
        if s2[b] is not None:
            v = float(s2[b])
            if not (math.isfinite(v) and v > 0.0):
                raise ValueError(f"item {b}: sigma2 must be finite and positive")
            s_arr.append(np.array([v]))
            c_arr.append(None)
        else:
            c = _f64(cov[b])
            if c.size != 9 * k:
                raise ValueError(f"item {b}: one 3 x 3 covariance per observation")
            if not np.all(np.isfinite(c)):
                raise ValueError(f"item {b}: covariances contain a non-finite value")
            s_arr.append(None)
            c_arr.append(c.reshape(k, 3, 3))
        p_arr.append(p.reshape(k, 3))
    shapes = {"alpha": lambda c: (c.rank,), "mean": lambda c: (c.N, 3), "basis": lambda c: (3 * c.N, c.rank),
              "variance": lambda c: (c.rank,), "point_variance": lambda c: (c.N,)}
    out = [{w: np.zeros(shapes[w](c)) for w in want} for c in ctxs]
    outs = [_ptr_array([o[w] for o in out]) if w in want else None for w in _POSTERIOR_WANT]
    status = np.zeros(n, dtype=np.int32)
    n_obs = np.array([a.shape[0] for a in ids], dtype=np.int32)
    c_ids = _ptr_array(ids, nat.c_int_p, _i)
    rc = nat.lib().icp_posterior_models_many(n, _ctx_array(ctxs), _i(n_obs), c_ids, _ptr_array(p_arr), _ptr_array(s_arr),
                                             _ptr_array(c_arr), *outs, _i(status))
    if rc != 0 and not status.any():
        nat.check(rc, "icp_posterior_models_many")  # a whole-call error: nothing has run
    for b in range(n):
        out[b]["status"] = int(status[b])
        if status[b] == -1:
            for w in want:
                del out[b][w]
    return out


_GP_WANT = ("variance", "basis", "pivots", "residual")
GP_MAX_PIVOTS, GP_MAX_TERMS = 256, 8
GP_MAX_LEVEL = 32    # B-spline levels lie in [-32, 32]
GP_NOT_FINITE = -3   # ICP_ERR_NOT_FINITE: an item of a general call whose pivot loop left no column (trace K = 0)
_KERNEL_TERMS = (_data.GaussianKernelTerm, _data.BSplineKernelTerm)


def _psd3(a):
    """exactly symmetric, positive semi-definite (principal minors in closed form, a rounding's slack) and not zero — the library's test"""
    if not np.all(np.isfinite(a)) or a[0, 1] != a[1, 0] or a[0, 2] != a[2, 0] or a[1, 2] != a[2, 1]:
        return False
    p, b, d, e, f, g = a[0, 0], a[0, 1], a[0, 2], a[1, 1], a[1, 2], a[2, 2]
    eps = 2.0 ** -48
    if p < 0 or e < 0 or g < 0 or not (p + e + g > 0):
        return False
    if p * e - b * b < -eps * (p * e + b * b) or p * g - d * d < -eps * (p * g + d * d) or e * g - f * f < -eps * (e * g + f * f):
        return False
    det = (p * (e * g - f * f) - b * (b * g - d * f)) + d * (b * f - d * e)
    mag = (p * (e * g + f * f) + abs(b) * (abs(b) * g + abs(d * f))) + abs(d) * (abs(b * f) + abs(d) * e)
    return bool(det >= -eps * mag)


def _kernel_terms(b, kb, p, general, keep, lattice=None):
    """the checked ctypes terms of item b's kernel `kb` on the points p [N, 3] (nat.KernelTermGeneral if `general`, else nat.KernelTerm);
    the weights' arrays go into `keep`, alive while the library reads them.  `lattice`: the largest |coordinate| the B-spline lattice has to
    hold, where that is more than p's"""
    kb = list(kb)
    if not (1 <= len(kb) <= GP_MAX_TERMS):
        raise ValueError(f"item {b}: a kernel has 1 to {GP_MAX_TERMS} terms")
    arr = ((nat.KernelTermGeneral if general else nat.KernelTerm) * len(kb))()
    for t, k in enumerate(kb):
        if not isinstance(k, _KERNEL_TERMS):
            raise ValueError(f"item {b}, term {t}: a data.GaussianKernelTerm or a data.BSplineKernelTerm")
        gauss = isinstance(k, _data.GaussianKernelTerm)
        if gauss and not (math.isfinite(k.scale) and k.scale > 0.0 and math.isfinite(k.sigma) and k.sigma > 0.0
                          and math.isfinite(k.sigma * k.sigma) and k.sigma * k.sigma > 0.0):
            raise ValueError(f"item {b}, term {t}: scale and sigma must be finite and positive")
        if not gauss:
            if not (math.isfinite(k.scale) and k.scale > 0.0):
                raise ValueError(f"item {b}, term {t}: scale must be finite and positive")
            if not (-GP_MAX_LEVEL <= k.level <= GP_MAX_LEVEL) or not (math.ldexp(float(np.abs(p).max()) if lattice is None else lattice, k.level) < 2.0 ** 31):
                raise ValueError(f"item {b}, term {t}: -{GP_MAX_LEVEL} <= level <= {GP_MAX_LEVEL} and |coordinate| * 2^level < 2^31")
        a = _f64(k.A)
        if a.shape != (3, 3) or not _psd3(a):
            raise ValueError(f"item {b}, term {t}: A must be an exactly symmetric, positive semi-definite, non-zero 3 x 3 matrix")
        arr[t].scale = k.scale
        arr[t].A[:] = a.reshape(-1).tolist()
        if not general:
            arr[t].sigma = k.sigma
            continue
        if k.mirror_axis not in (0, 1, 2) or not (0.0 <= k.mirror_gain <= 1.0):
            raise ValueError(f"item {b}, term {t}: mirror_axis is 0, 1 or 2 and 0 <= mirror_gain <= 1")
        ax = k.mirror_axis
        if k.mirror_gain > 0.0 and any(a[ax, c] != 0.0 or a[c, ax] != 0.0 for c in range(3) if c != ax):
            raise ValueError(f"item {b}, term {t}: with a mirror gain, A must not couple the mirror axis to the others")
        arr[t].struct_size = C.sizeof(nat.KernelTermGeneral)
        arr[t].kind = nat.KERNEL_GAUSSIAN if gauss else nat.KERNEL_BSPLINE3
        arr[t].sigma, arr[t].level = (k.sigma, 0) if gauss else (0.0, k.level)
        arr[t].mirror_axis, arr[t].mirror_gain = ax, k.mirror_gain
        if k.weights is not None:
            w = _f64(k.weights)
            if w.shape != (p.shape[0],) or not np.all(np.isfinite(w)) or not np.all(w >= 0.0) or not np.any(w > 0.0):
                raise ValueError(f"item {b}, term {t}: weights are [N], finite, >= 0 and not all zero")
            keep.append(w)
            arr[t].weights = _d(w)
    return arr


def gp_models(meshes, kernels, n_pivots, rank=None, rel_tolerance=0.0, device=0, want=_GP_WANT):
    """Gaussian-process shape models of analytic kernels on many reference meshes in one call (icp_gp_models_many): what
    apps/femur/CreateGPModel.scala makes, by Scalismo's pivoted Cholesky approximation instead of the Nyström one.  Item b: the model
    of kernels[b] — a list of 1..8 data.GaussianKernelTerm, k(x, y) = Σ_t scale_t·exp(−‖x−y‖²/σ_t²)·A_t — on the points of meshes[b] (a
    data.TriangleMesh), from at most n_pivots[b] <= min(256, 3N) pivots, keeping the leading rank[b] <= n_pivots[b] eigenpairs (None:
    n_pivots); the pivot loop also stops when the residual trace is <= rel_tolerance[b] · trace(K) or the numerical rank is reached.
    `kernels`: one list of terms for every mesh, or one list per mesh; n_pivots, rank, rel_tolerance: a number for all, or one per item.
    `want` names the arrays to fetch.  Returns one (model, info) per item: a data.StatisticalMeshModel (zero mean deformation, columns of
    squared norm N; None unless "variance" and "basis" are wanted) of the effective rank min(rank, effective pivots), and a dict with
    "n_pivots" (effective), "rank" (effective), "total_variance" trace(K)/N, "approximated_variance" Σ variance, and the wanted ones of
    "variance" [rank], "pivots" [effective] (rows 3·vertex + coordinate in the order chosen), "residual" [3N] (the residual diagonal
    when the loop stopped).
    A kernel may also hold general terms — data.BSplineKernelTerm, or a data.GaussianKernelTerm with weights or a mirror gain (the face
    kernel of apps/bfm: face_kernel) —, mixed freely with plain ones: such a call goes through icp_gp_models_general_many, and every
    info dict then has "status": 0, or -3 (ICP_ERR_NOT_FINITE; model None, NaN arrays, the counts zero) for an item whose kernel
    matrix has trace 0 (a mirror gain of 1, or weights that vanish), beside which the other items are computed."""
    ms = list(meshes)
    n = len(ms)
    if n == 0 or n > 65535:
        raise ValueError("at least one mesh, at most 65,535 a call")
    ks = list(kernels)
    if ks and isinstance(ks[0], _KERNEL_TERMS):
        ks = [ks] * n
    if len(ks) != n:
        raise ValueError("one kernel (a list of terms) per mesh, or one for all")

    def per_item(v, name):
        v = list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n
        if len(v) != n:
            raise ValueError(f"{name}: a number, or one per item")
        return v
    mp = [int(v) for v in per_item(n_pivots, "n_pivots")]
    rk = [mp[b] if v is None else int(v) for b, v in enumerate(per_item(rank, "rank"))]
    tol = [float(v) for v in per_item(rel_tolerance, "rel_tolerance")]
    want = tuple(want)
    for w in want:
        if w not in _GP_WANT:
            raise ValueError(f"unknown output {w!r}: one of {_GP_WANT}")
    pts, terms = [], []
    # a call whose every term is a plain Gaussian one goes through icp_gp_models_many, any other through icp_gp_models_general_many
    general = not all(isinstance(k, _data.GaussianKernelTerm) and k.plain for kb in ks for k in kb)
    keep = []  # (the weights' arrays, alive while the library reads them)
    for b in range(n):
        p = _f64(ms[b].points)
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError(f"item {b}: a mesh has points [N, 3]")
        if not np.all(np.isfinite(p)):
            raise ValueError(f"item {b}: points contain a non-finite value")
        if not (1 <= rk[b] <= mp[b] <= min(GP_MAX_PIVOTS, 3 * p.shape[0])):
            raise ValueError(f"item {b}: 1 <= rank <= n_pivots <= min({GP_MAX_PIVOTS}, 3N)")
        if not (0.0 <= tol[b] < 1.0):
            raise ValueError(f"item {b}: rel_tolerance lies in [0, 1)")
        arr = _kernel_terms(b, ks[b], p, general, keep)
        pts.append(p)
        terms.append(arr)
    shapes = {"variance": lambda b: (rk[b],), "basis": lambda b: (3 * pts[b].shape[0], rk[b]), "pivots": lambda b: (mp[b],),
              "residual": lambda b: (3 * pts[b].shape[0],)}
    out = [{w: np.zeros(shapes[w](b), dtype=np.int32 if w == "pivots" else np.float64) for w in want} for b in range(n)]
    info = np.zeros((n, 4))
    status = np.zeros(n, dtype=np.int32)
    outs = [None if w not in want else _ptr_array([o[w] for o in out], nat.c_int_p, _i) if w == "pivots"
            else _ptr_array([o[w] for o in out]) for w in _GP_WANT]
    term_t = nat.KernelTermGeneral if general else nat.KernelTerm
    c_terms = (C.POINTER(term_t) * n)(*[C.cast(a, C.POINTER(term_t)) for a in terms])
    n_pts = np.array([p.shape[0] for p in pts], dtype=np.int32)
    n_terms = np.array([len(a) for a in terms], dtype=np.int32)
    a_mp, a_rk, a_tol = np.array(mp, dtype=np.int32), np.array(rk, dtype=np.int32), np.array(tol, dtype=np.float64)
    if general:
        rc = nat.lib().icp_gp_models_general_many(n, int(device), _i(n_pts), _ptr_array(pts), _i(n_terms), c_terms, _i(a_mp), _i(a_rk),
                                                  _d(a_tol), outs[0], outs[1], outs[2], outs[3], _ptr_array(list(info)), _i(status))
        if rc != 0 and (not status.any() or not np.all((status == 0) | (status == GP_NOT_FINITE))):
            nat.check(rc, "icp_gp_models_general_many")  # a whole-call error, or an item the checks above should have refused
    else:
        rc = nat.lib().icp_gp_models_many(n, int(device), _i(n_pts), _ptr_array(pts), _i(n_terms), c_terms, _i(a_mp), _i(a_rk), _d(a_tol),
                                          outs[0], outs[1], outs[2], outs[3], _ptr_array(list(info)), _i(status))
        nat.check(rc, "icp_gp_models_many")
    res = []
    for b in range(n):
        me, re = int(info[b, 0]), int(info[b, 1])
        d = {"n_pivots": me, "rank": re, "total_variance": float(info[b, 2]), "approximated_variance": float(info[b, 3])}
        if general:
            d["status"] = int(status[b])
        if "variance" in want:
            d["variance"] = out[b]["variance"][:re].copy()
        if "pivots" in want:
            d["pivots"] = out[b]["pivots"][:me].copy()
        if "residual" in want:
            d["residual"] = out[b]["residual"]
        model = None
        if "variance" in want and "basis" in want and status[b] == 0:
            model = _data.StatisticalMeshModel(pts[b], ms[b].cells, np.zeros_like(pts[b]), out[b]["basis"][:, :re], d["variance"])
        res.append((model, d))
    return res


def gp_model(mesh, kernel, n_pivots, rank=None, rel_tolerance=0.0, device=0, want=_GP_WANT):
    """One item of gp_models: (model, info) of `kernel` (a list of data.GaussianKernelTerm and data.BSplineKernelTerm) on `mesh`."""
    return gp_models([mesh], [list(kernel)], n_pivots, rank, rel_tolerance, device, want)[0]


_NYS_WANT = ("variance", "basis", "sample_eigenvalues", "sample_eigenvectors")
NYSTROM_MAX_ROWS, NYSTROM_MAX_RANK = 2400, 256
NYSTROM_NOT_CONVERGED = -7  # ICP_ERR_NOT_CONVERGED: the iteration hit its cap on sweeps; the item's outputs are written all the same


def nystrom_models(items, min_variance=1e-8, device=0, want=_NYS_WANT):
    """Gaussian-process shape models by the Nyström approximation on sample points, many in one call (icp_nystrom_models_many): what
    apps/femur/CreateGPModel.scala and apps/bfm/CreateGPModel.scala call, LowRankGaussianProcess.approximateGPNystrom.  An item is
    (mesh, samples, terms, rank) or (mesh, samples, terms, rank, sample_weights): a data.TriangleMesh, sample points [n, 3] (the
    caller's choice; data.surface_samples draws them on the device, data.uniform_mesh_samples on the host), a kernel as gp_models takes it (a list of
    data.GaussianKernelTerm and data.BSplineKernelTerm, plain or general) and the number of basis functions, 1 <= rank <= min(256, 3n)
    with 3n <= 2,400.  A term with weights — they are the region weights at the mesh points — needs the same region weights at the sample
    points: sample_weights, one entry per term, None or [n].  K = k(S, S) = U·Λ·Uᵀ; variance_i = λ_i/n; basis column i =
    k(X, S)·u_i·√n/λ_i; the rank kept, k_eff, is the number of i < rank with λ_i/n >= min_variance (a number for all, or one per item).
    Returns one (model, info) per item: a data.StatisticalMeshModel of k_eff components with zero mean deformation (its columns are not
    orthonormal on the mesh; None unless "variance" and "basis" are wanted and the item was computed), and a dict with "rank" (k_eff),
    "sweeps", "trace", "off_diagonal_mass", "status" (0; -7 where the iteration hit its cap on sweeps, the outputs written all the
    same) and the wanted ones of "variance" [rank] (λ_i/n, all of them), "sample_eigenvalues" [3n], "sample_eigenvectors" [3n, rank]."""
    its = [tuple(i) for i in items]
    n = len(its)
    if n == 0 or n > 65535:
        raise ValueError("at least one item, at most 65,535 a call")
    mv = list(min_variance) if isinstance(min_variance, (list, tuple, np.ndarray)) else [min_variance] * n
    if len(mv) != n:
        raise ValueError("min_variance: a number, or one per item")
    mv = np.array([float(v) for v in mv], dtype=np.float64)
    want = tuple(want)
    for w in want:
        if w not in _NYS_WANT:
            raise ValueError(f"unknown output {w!r}: one of {_NYS_WANT}")
    pts, smp, terms, rk, sws, keep = [], [], [], [], [], []
    for b, item in enumerate(its):
        if len(item) not in (4, 5):
            raise ValueError(f"item {b}: (mesh, samples, terms, rank) or (mesh, samples, terms, rank, sample_weights)")
        mesh, samples, kb, rank = item[:4]
        p, s = _f64(mesh.points), _f64(samples)
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError(f"item {b}: a mesh has points [N, 3]")
        if s.ndim != 2 or s.shape[1] != 3 or s.shape[0] < 1:
            raise ValueError(f"item {b}: samples are [n, 3]")
        if int(rank) != rank:
            raise ValueError(f"item {b}: rank is a whole number")
        if not np.all(np.isfinite(p)) or not np.all(np.isfinite(s)):
            raise ValueError(f"item {b}: points or samples contain a non-finite value")
        if 3 * s.shape[0] > NYSTROM_MAX_ROWS:
            raise ValueError(f"item {b}: at most {NYSTROM_MAX_ROWS // 3} sample points")
        if not (1 <= rank <= min(NYSTROM_MAX_RANK, 3 * s.shape[0])):
            raise ValueError(f"item {b}: 1 <= rank <= min({NYSTROM_MAX_RANK}, 3n)")
        if not (math.isfinite(mv[b]) and mv[b] >= 0.0):
            raise ValueError(f"item {b}: min_variance must be finite and >= 0")
        arr = _kernel_terms(b, kb, p, True, keep, max(float(np.abs(p).max()), float(np.abs(s).max())))
        sw = list(item[4]) if len(item) == 5 and item[4] is not None else [None] * len(arr)
        if len(sw) != len(arr):
            raise ValueError(f"item {b}: sample_weights has one entry (None or [n]) per term")
        c_sw = (nat.c_double_p * len(arr))()
        for t in range(len(arr)):
            if bool(arr[t].weights) != (sw[t] is not None):
                raise ValueError(f"item {b}, term {t}: a term has weights at the mesh points and at the sample points, or neither")
            if sw[t] is None:
                continue
            w = _f64(sw[t])
            if w.shape != (s.shape[0],) or not np.all(np.isfinite(w)) or not np.all(w >= 0.0) or not np.any(w > 0.0):
                raise ValueError(f"item {b}, term {t}: sample weights are [n], finite, >= 0 and not all zero")
            keep.append(w)
            c_sw[t] = _d(w)
        pts.append(p); smp.append(s); terms.append(arr); rk.append(int(rank)); sws.append(c_sw)
    R = [3 * s.shape[0] for s in smp]
    shapes = {"variance": lambda b: (rk[b],), "basis": lambda b: (3 * pts[b].shape[0], rk[b]), "sample_eigenvalues": lambda b: (R[b],),
              "sample_eigenvectors": lambda b: (R[b], rk[b])}
    out = [{w: np.zeros(shapes[w](b)) for w in want} for b in range(n)]
    info = np.zeros((n, 4))
    status = np.zeros(n, dtype=np.int32)
    outs = [None if w not in want else _ptr_array([o[w] for o in out]) for w in _NYS_WANT]
    term_t = nat.KernelTermGeneral
    c_terms = (C.POINTER(term_t) * n)(*[C.cast(a, C.POINTER(term_t)) for a in terms])
    c_sws = (C.POINTER(nat.c_double_p) * n)(*[C.cast(a, C.POINTER(nat.c_double_p)) for a in sws])
    n_pts = np.array([p.shape[0] for p in pts], dtype=np.int32)
    n_smp = np.array([s.shape[0] for s in smp], dtype=np.int32)
    n_terms = np.array([len(a) for a in terms], dtype=np.int32)
    a_rk = np.array(rk, dtype=np.int32)
    rc = nat.lib().icp_nystrom_models_many(n, int(device), _i(n_pts), _ptr_array(pts), _i(n_smp), _ptr_array(smp), _i(n_terms), c_terms, c_sws,
                                           _i(a_rk), _d(mv), outs[0], outs[1], outs[2], outs[3], _ptr_array(list(info)), _i(status))
    if rc != 0 and (not status.any() or not np.all((status == 0) | (status == NYSTROM_NOT_CONVERGED))):
        nat.check(rc, "icp_nystrom_models_many")  # a whole-call error, or an item the checks above should have refused
    res = []
    for b in range(n):
        ke = int(info[b, 0])
        d = {"rank": ke, "sweeps": int(info[b, 1]), "trace": float(info[b, 2]), "off_diagonal_mass": float(info[b, 3]), "status": int(status[b])}
        for w in want:
            if w != "basis":
                d[w] = out[b][w]
        model = None
        if "variance" in want and "basis" in want:
            model = _data.StatisticalMeshModel(pts[b], its[b][0].cells, np.zeros_like(pts[b]), out[b]["basis"][:, :ke], out[b]["variance"][:ke])
        res.append((model, d))
    return res


def nystrom_model(mesh, samples, terms, rank, sample_weights=None, min_variance=1e-8, device=0, want=_NYS_WANT):
    """One item of nystrom_models: (model, info) of the kernel `terms` on `mesh`, approximated on the sample points `samples`."""
    return nystrom_models([(mesh, samples, list(terms), rank, sample_weights)], min_variance, device, want)[0]


_PCA_WANT = ("variance", "mean", "transforms")
PCA_MAX_MESHES, PCA_MAX_ROUNDS = 256, 32
PCA_NOT_FINITE = -3  # ICP_ERR_NOT_FINITE: an item whose meshes are all equal (no component is left)


def pca_models(mesh_sets, rank=None, gpa_iterations=3, halt_distance=1e-5, reference=None, cells=None, device=0, want=_PCA_WANT):
    """PCA shape models of meshes in correspondence, with generalised Procrustes alignment, many in one call (icp_pca_models_many;
    Scalismo's DataCollection.gpa followed by StatisticalMeshModel.createUsingPCA).  `mesh_sets`: a list of items, each
    a list of 2..256 [N, 3] arrays or data.TriangleMesh of one N; arrays that are the same object go into the call's pool once.  Item b:
    at most gpa_iterations[b] <= 32 rounds of rigid alignment to the mean shape, stopped behind the round that moves the mean shape by
    less than halt_distance[b] (RMS); then the leading rank[b] <= n − 1 (None: n − 1) eigenpairs of the covariance of the aligned
    meshes.  rank, gpa_iterations, halt_distance: one for all, or one per item.  reference: None, one [N, 3] array or mesh for all, or a
    list of one (or None) per item: the model's reference points, its mean deformation being mean shape − reference; None: the mean
    shape is the reference.  cells: the triangles, one array for all or one per item (None: those of the item's first data.TriangleMesh,
    else none).  Returns one (model, info) per item: a data.StatisticalMeshModel of the effective rank with columns of squared norm N
    (None for an item that failed), and a dict with "n_meshes", "rank" (effective), "total_variance" trace(G)/N, "approximated_variance"
    Σ variance, "rounds", "rms" (the last round's RMS displacement of the mean shape), "status" (0, or -3 with NaN arrays for an item
    whose meshes are all equal, beside which the others are computed) and the wanted ones of "variance" [rank], "mean" [N, 3],
    "transforms" [n, 12] (each mesh's composite rotation by rows, then its translation)."""
    want = tuple(want)
    for w in want:
        if w not in _PCA_WANT:
            raise ValueError(f"unknown output {w!r}: one of {_PCA_WANT}")
    sets = [list(s) for s in mesh_sets]
    n = len(sets)
    if n == 0 or n > 65535:
        raise ValueError("at least one item, at most 65,535 a call")

    def per_item(v, name, single):
        v = [v] * n if single(v) else list(v)
        if len(v) != n:
            raise ValueError(f"{name}: one for all items, or one per item")
        return v
    scalar = lambda v: v is None or not isinstance(v, (list, tuple, np.ndarray))  # noqa: E731
    array = lambda v: v is None or isinstance(v, (np.ndarray, _data.TriangleMesh))  # noqa: E731
    rk = per_item(rank, "rank", scalar)
    it = [int(v) for v in per_item(gpa_iterations, "gpa_iterations", scalar)]
    hd = [float(v) for v in per_item(halt_distance, "halt_distance", scalar)]
    refs = per_item(reference, "reference", array)
    cls = per_item(cells, "cells", lambda v: v is None or isinstance(v, np.ndarray))
    pool, pool_index, ids = [], {}, []
    for b, ms in enumerate(sets):
        if not (2 <= len(ms) <= PCA_MAX_MESHES):
            raise ValueError(f"item {b}: 2 to {PCA_MAX_MESHES} meshes")
        row = []
        for m in ms:
            src = m.points if isinstance(m, _data.TriangleMesh) else m
            if id(src) not in pool_index:
                p = _f64(src)
                if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
                    raise ValueError(f"item {b}: a mesh has points [N, 3]")
                if not np.all(np.isfinite(p)):
                    raise ValueError(f"item {b}: points contain a non-finite value")
                pool_index[id(src)] = len(pool)
                pool.append((src, p))  # (src: kept alive, so that its id stays its own)
            row.append(pool_index[id(src)])
        N = pool[row[0]][1].shape[0]
        if any(pool[k][1].shape[0] != N for k in row):
            raise ValueError(f"item {b}: the meshes of an item have one N")
        rk[b] = len(ms) - 1 if rk[b] is None else int(rk[b])
        if not (1 <= rk[b] <= len(ms) - 1):
            raise ValueError(f"item {b}: 1 <= rank <= n - 1")
        if not (0 <= it[b] <= PCA_MAX_ROUNDS):
            raise ValueError(f"item {b}: 0 <= gpa_iterations <= {PCA_MAX_ROUNDS}")
        if not (math.isfinite(hd[b]) and hd[b] >= 0.0):
            raise ValueError(f"item {b}: halt_distance must be finite and >= 0")
        if refs[b] is not None:
            r = _f64(refs[b].points if isinstance(refs[b], _data.TriangleMesh) else refs[b])
            if r.shape != (N, 3) or not np.all(np.isfinite(r)):
                raise ValueError(f"item {b}: the reference is [N, 3] and finite")
            refs[b] = r
        if cls[b] is None:
            first = next((m for m in ms if isinstance(m, _data.TriangleMesh)), None)
            cls[b] = first.cells if first is not None else np.zeros((0, 3), dtype=np.int32)
        ids.append(np.array(row, dtype=np.int32))
    n_pts = [pool[row[0]][1].shape[0] for row in ids]
    var = [np.zeros(rk[b]) for b in range(n)]
    basis = [np.zeros((3 * n_pts[b], rk[b])) for b in range(n)]
    mean = [np.zeros((n_pts[b], 3)) for b in range(n)]
    tfs = [np.zeros((len(sets[b]), 12)) for b in range(n)] if "transforms" in want else None
    info = np.zeros((n, 8))
    status = np.zeros(n, dtype=np.int32)
    pool_pts = np.array([p.shape[0] for _, p in pool], dtype=np.int32)
    n_meshes = np.array([len(s) for s in sets], dtype=np.int32)
    a_rk, a_it, a_hd = np.array(rk, dtype=np.int32), np.array(it, dtype=np.int32), np.array(hd, dtype=np.float64)
    rc = nat.lib().icp_pca_models_many(n, int(device), len(pool), _i(pool_pts), _ptr_array([p for _, p in pool]), _i(n_meshes),
                                       _ptr_array(ids, nat.c_int_p, _i), _ptr_array(refs), _i(a_rk), _i(a_it), _d(a_hd), _ptr_array(var),
                                       _ptr_array(basis), _ptr_array(mean), None if tfs is None else _ptr_array(tfs),
                                       _ptr_array(list(info)), _i(status))
    if rc != 0 and (not status.any() or not np.all((status == 0) | (status == PCA_NOT_FINITE))):
        nat.check(rc, "icp_pca_models_many")  # a whole-call error, or an item the checks above should have refused
    res = []
    for b in range(n):
        ok = status[b] == 0
        re = int(info[b, 1]) if ok else 0
        d = {"n_meshes": len(sets[b]), "rank": re, "total_variance": float(info[b, 2]), "approximated_variance": float(info[b, 3]),
             "rounds": int(info[b, 4]) if ok else 0, "rms": float(info[b, 5]), "status": int(status[b])}
        if "variance" in want:
            d["variance"] = var[b][:re].copy() if ok else var[b]
        if "mean" in want:
            d["mean"] = mean[b]
        if "transforms" in want:
            d["transforms"] = tfs[b]
        model = None
        if ok:
            ref = mean[b] if refs[b] is None else refs[b]
            model = _data.StatisticalMeshModel(ref, cls[b], mean[b] - ref, basis[b][:, :re], var[b][:re].copy())
        res.append((model, d))
    return res


def pca_model(meshes, rank=None, gpa_iterations=3, halt_distance=1e-5, reference=None, cells=None, device=0, want=_PCA_WANT):
    """One item of pca_models: (model, info) of the meshes in correspondence `meshes`."""
    return pca_models([list(meshes)], rank, gpa_iterations, halt_distance, reference, cells, device, want)[0]


def leave_one_out_pca_models(meshes, rank=None, gpa_iterations=3, halt_distance=1e-5, reference=None, cells=None, device=0, want=_PCA_WANT):
    """The n leave-one-out models of n >= 3 meshes in ONE pca_models call over one pool (n uploads, not n·(n−1)): item i is the model
    of all meshes but mesh i — what generalisation and specificity of a learned model are measured on."""
    ms = list(meshes)
    if len(ms) < 3:
        raise ValueError("leave-one-out models need at least three meshes")
    return pca_models([ms[:i] + ms[i + 1:] for i in range(len(ms))], rank, gpa_iterations, halt_distance, reference, cells, device, want)


def region_weights(points, region_points, stddev=40.0, device=0):
    """Smoothed region weights (icp_region_weights_many; apps/bfm/FaceMask.scala computeSmoothedRegions): w[i] = exp(−d²/stddev²), d the
    distance from points[i] to the nearest of region_points; exactly 1 at a region point.  One item — points [N, 3], region_points
    [M, 3], M >= 1 -> [N] — or lists of them -> a list; stddev a number for all or one per item.  One launch for the whole call."""
    single = not isinstance(points, (list, tuple))
    ps = [points] if single else list(points)
    rs = [region_points] if single else list(region_points)
    n = len(ps)
    if n == 0 or n > 65535 or len(rs) != n:
        raise ValueError("at least one item, at most 65,535 a call, and one region per item")
    sd = list(stddev) if isinstance(stddev, (list, tuple, np.ndarray)) else [stddev] * n
    if len(sd) != n:
        raise ValueError("stddev: a number, or one per item")
    ps, rs = [_f64(p) for p in ps], [_f64(r) for r in rs]
    sd = np.array([float(s) for s in sd], dtype=np.float64)
    for b in range(n):
        for a, name in ((ps[b], "points"), (rs[b], "region_points")):
            if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1 or not np.all(np.isfinite(a)):
                raise ValueError(f"item {b}: {name} are [n >= 1, 3] and finite")
        if not (math.isfinite(sd[b]) and sd[b] > 0.0 and math.isfinite(sd[b] * sd[b]) and sd[b] * sd[b] > 0.0):
            raise ValueError(f"item {b}: stddev must be finite and positive")
    out = [np.zeros(p.shape[0]) for p in ps]
    status = np.zeros(n, dtype=np.int32)
    n_pts = np.array([p.shape[0] for p in ps], dtype=np.int32)
    n_reg = np.array([r.shape[0] for r in rs], dtype=np.int32)
    rc = nat.lib().icp_region_weights_many(n, int(device), _i(n_pts), _ptr_array(ps), _i(n_reg), _ptr_array(rs), _d(sd), _ptr_array(out),
                                           _i(status))
    nat.check(rc, "icp_region_weights_many")
    return out[0] if single else out


def face_kernel(mesh, mask=None, device=0):
    """The kernel of apps/bfm/FaceKernel.scala on `mesh` (a data.TriangleMesh): five data.BSplineKernelTerm, (level, scale) = (−6, 128),
    (−5, 64), (−4, 32), (−3, 10), (−2, 4), A = I, mirrored about x = 0 with gain 0.7 (0.7·symmetrize(k) + 0.3·k), each weighted by the
    smoothed region of its level in `mask` (a data.FaceMask; stddev 40).  mask=None is bfm/CreateGPModel.scala's mask of 3 everywhere:
    weights 1, nothing runs on the device.  Otherwise the five levels' weights come from ONE icp_region_weights_many call."""
    levels = _data.FACE_KERNEL_LEVELS
    weights = [None] * len(levels)
    if mask is not None:
        regions = [mask.region(mesh, level) for level, _ in levels]
        weights = region_weights([mesh.points] * len(levels), regions, 40.0, device)
    return [_data.BSplineKernelTerm(scale, level, np.eye(3), w, _data.FACE_KERNEL_MIRROR_GAIN, 0) for (level, scale), w in zip(levels, weights)]


_SCAN_WANT = ("aligned", "partial", "kept_ids", "landmarks", "cut_flags")
_SCAN_MAX_POINTS, _SCAN_MAX_CUTS, _SCAN_MAX_MAGNITUDE = 1 << 26, 7, 2.0 ** 400


def _is_int_like(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_cut_list(v):
    """one item's cuts: a list or tuple of (landmark index, count) pairs, possibly empty"""
    return isinstance(v, (list, tuple)) and all(isinstance(q, (list, tuple)) and len(q) == 2 and all(_is_int_like(x) for x in q) for q in v)


def _scan_per_item(value, n, is_single, name):
    """`value` for every item: one value (is_single) is repeated, a list or tuple has one entry per item"""
    if value is None or is_single(value):
        return [value] * n
    if not isinstance(value, (list, tuple)) or len(value) != n:
        raise ValueError(f"{name}: one for all items, or one per item")
    return list(value)


def prepare_scans(scans, transforms, landmarks=None, cuts=None, mask_ids=None, device=0, want=_SCAN_WANT) -> list:
    """Aligned and partial targets of many raw scans in one call (icp_scans_prepare_many; apps/femur/AlignShapes.scala:30-55,
    apps/bfm/AlignShapes.scala:33-101).  Per item: `scans[b]` (a data.TriangleMesh) under `transforms[b]` (a
    data.ScanTransform: A(x) = R·(s·x − c) + c + t), its `landmarks[b]` [L, 3] under the same transform, `cuts[b]` — up to seven
    pairs (landmark index, count): the count vertices nearest the aligned landmark, equal distances going to the lowest ids — and
    `mask_ids[b]`, vertex ids to cut away besides (repeats are fine, ids >= the vertex count match nothing).  What no cut took is
    compacted as maskPoints(...).transformedMesh does: triangles without a cut vertex, and the vertices they use.
    One transform, landmark array, cut list or id list serves every item; a list or tuple holds one per item.
    -> one dict per item with the keys of `want`: "aligned" (TriangleMesh, all vertices), "partial" (TriangleMesh), "kept_ids" [n_kept]
    (kept_ids[new] = old), "landmarks" [L, 3], "cut_flags" [M] uint8 (bit j: cut j; bit 7: the id list)."""
    want = _want(want, _SCAN_WANT)
    scans = [scans] if isinstance(scans, _data.TriangleMesh) else list(scans)
    n = len(scans)
    if n == 0 or n > 65535:
        raise ValueError("at least one scan, at most 65,535 a call")
    tfs = _scan_per_item(transforms, n, lambda v: isinstance(v, _data.ScanTransform), "transforms")
    lms = _scan_per_item(landmarks, n, lambda v: isinstance(v, np.ndarray), "landmarks")
    cts = _scan_per_item(cuts, n, _is_cut_list, "cuts")
    mks = _scan_per_item(mask_ids, n, lambda v: isinstance(v, np.ndarray) or (isinstance(v, (list, tuple)) and all(_is_int_like(x) for x in v)),
                         "mask_ids")
    pts, cells, tf_arr, lm_arr, cl_arr, cc_arr, mk_arr = [], [], (nat.ScanTransform * n)(), [], [], [], []
    for b in range(n):
        mesh, tf = scans[b], tfs[b]
        if not isinstance(mesh, _data.TriangleMesh) or not isinstance(tf, _data.ScanTransform):
            raise ValueError(f"item {b}: a data.TriangleMesh and a data.ScanTransform")
        p, c = mesh.points, mesh.cells.reshape(-1, 3)
        M = p.shape[0]
        if p.ndim != 2 or p.shape[1] != 3 or M < 1 or M > _SCAN_MAX_POINTS or c.shape[0] > _SCAN_MAX_POINTS:
            raise ValueError(f"item {b}: points are [1 .. 2^26, 3], at most 2^26 triangles")
        if c.size and (c.min() < 0 or c.max() >= M):
            raise ValueError(f"item {b}: a triangle's vertex id is out of range")
        s = tf.pre_scale
        if not (math.isfinite(s) and s > 0.0):
            raise ValueError(f"item {b}: pre_scale must be finite and positive")
        lm = np.zeros((0, 3)) if lms[b] is None else _f64(lms[b]).reshape(-1, 3)
        with np.errstate(over="ignore", invalid="ignore"):
            small = all(np.all(np.abs(a) <= _SCAN_MAX_MAGNITUDE) for a in (tf.rotation, tf.centre, tf.translation, p, lm, s * p, s * lm))
        if not small:
            raise ValueError(f"item {b}: every value is finite, and |s·x|, |c|, |t| and |R_ij| are at most 2^400")
        ct = [] if cts[b] is None else list(cts[b])
        if len(ct) > _SCAN_MAX_CUTS:
            raise ValueError(f"item {b}: at most {_SCAN_MAX_CUTS} cuts")
        for pair in ct:
            if len(pair) != 2 or not all(_is_int_like(x) for x in pair) or not (0 <= pair[0] < lm.shape[0]) or not (0 <= pair[1] <= 2 ** 31 - 1):
                raise ValueError(f"item {b}: a cut is (landmark index in [0, {lm.shape[0]}), count >= 0)")
        mk = np.zeros(0, dtype=np.int64) if mks[b] is None else np.asarray(mks[b])
        if mk.size and (mk.ndim != 1 or mk.dtype.kind not in "iu" or mk.min() < 0 or mk.max() > 2 ** 31 - 1):
            raise ValueError(f"item {b}: mask ids are int32 values >= 0")
        pts.append(p); cells.append(np.ascontiguousarray(c, dtype=np.int32)); lm_arr.append(lm)
        cl_arr.append(np.array([q[0] for q in ct], dtype=np.int32)); cc_arr.append(np.array([q[1] for q in ct], dtype=np.int32))
        mk_arr.append(np.ascontiguousarray(mk.reshape(-1), dtype=np.int32))
        tf_arr[b].struct_size, tf_arr[b].pre_scale = C.sizeof(nat.ScanTransform), s
        tf_arr[b].rotation[:] = tf.rotation.reshape(-1).tolist()
        tf_arr[b].centre[:] = tf.centre.tolist()
        tf_arr[b].translation[:] = tf.translation.tolist()
    counts = lambda arrays, width=1: np.array([a.shape[0] // width if a.ndim == 1 else a.shape[0] for a in arrays], dtype=np.int32)  # noqa: E731
    n_pts, n_tri, n_lm, n_ct, n_mk = counts(pts), counts(cells), counts(lm_arr), counts(cl_arr), counts(mk_arr)
    partial = "partial" in want
    aligned = [np.zeros((p.shape[0], 3)) for p in pts] if "aligned" in want else None
    lm_out = [np.zeros((a.shape[0], 3)) for a in lm_arr] if "landmarks" in want else None
    flags = [np.zeros(p.shape[0], dtype=np.uint8) for p in pts] if "cut_flags" in want else None
    ppts = [np.zeros((p.shape[0], 3)) for p in pts] if partial else None
    ptris = [np.zeros((c.shape[0], 3), dtype=np.int32) for c in cells] if partial else None
    kept = [np.zeros(p.shape[0], dtype=np.int32) for p in pts] if (partial or "kept_ids" in want) else None
    cnt = np.zeros(2 * n, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    out_d = lambda a: None if a is None else _ptr_array(a)  # noqa: E731
    out_i = lambda a: None if a is None else _ptr_array(a, nat.c_int_p, _i)  # noqa: E731
    rc = nat.lib().icp_scans_prepare_many(n, int(device), _i(n_pts), _ptr_array(pts), _i(n_tri), _ptr_array(cells, nat.c_int_p, _i), tf_arr,
                                          _i(n_lm), _ptr_array(lm_arr), _i(n_ct), _ptr_array(cl_arr, nat.c_int_p, _i),
                                          _ptr_array(cc_arr, nat.c_int_p, _i), _i(n_mk), _ptr_array(mk_arr, nat.c_int_p, _i), out_d(aligned),
                                          out_d(lm_out), None if flags is None else _ptr_array(flags, nat.c_ubyte_p, _ubyte_p), out_d(ppts),
                                          out_i(ptris), out_i(kept), _i(cnt), _i(status))
    nat.check(rc, "icp_scans_prepare_many")
    out = []
    for b in range(n):
        nk, tk = int(cnt[2 * b]), int(cnt[2 * b + 1])
        item = {}
        if "aligned" in want:
            item["aligned"] = _data.TriangleMesh(aligned[b], cells[b])
        if partial:
            item["partial"] = _data.TriangleMesh(ppts[b][:nk].copy(), ptris[b][:tk].copy())
        if "kept_ids" in want:
            item["kept_ids"] = kept[b][:nk].copy()
        if "landmarks" in want:
            item["landmarks"] = lm_out[b]
        if "cut_flags" in want:
            item["cut_flags"] = flags[b]
        out.append(item)
    return out


_DECIMATE_WANT = ("ids", "points", "cells", "labels", "cover2", "counts")
_DECIMATE_MAX_VERTICES, _DECIMATE_MAX_TRIANGLES, _DECIMATE_MAX_POINTS, _DECIMATE_MAX_MAGNITUDE = 1 << 24, 1 << 26, 65535, 2.0 ** 60


def decimated_meshes(meshes, counts, starts=None, device=0, want=_DECIMATE_WANT) -> list:
    """Many meshes decimated to vertex subsets in one call (icp_decimate_many): per item min(counts[b], M)
    farthest-point samples from vertex starts[b] (default 0; equal distances go to the lowest id), every vertex labelled with the
    sample nearest along mesh edges, and the dual triangles of those cells.  A decimation of this library's own kind — VTK's quadric
    decimation is not reproduced —, deterministic to the bit, whose points are vertices of the input.  Any prefix of "ids" is the
    decimation to that smaller count: one call at the largest count serves a whole ladder of counts (the triangles and labels belong
    to the full count).  One count or start serves every item; a list holds one per item.
    -> one dict per item with the keys of `want`: "ids" [k_eff] int32, "points" [k_eff, 3], "cells" [T_out, 3] int32 (ids into "ids"),
    "labels" [M] int32 (−1: no sample reaches the vertex), "cover2" [k_eff] (squared covering radius after j + 1 samples), "counts"
    (k_eff, T_out, sweeps).  The result need not be a manifold: data.mesh_edge_census counts the edges by their triangles."""
    want = _want(want, _DECIMATE_WANT)
    meshes = [meshes] if isinstance(meshes, _data.TriangleMesh) else list(meshes)
    n = len(meshes)
    if n == 0 or n > 65535:
        raise ValueError("at least one mesh, at most 65,535 a call")
    ks = _scan_per_item(counts, n, _is_int_like, "counts")
    ss = _scan_per_item(0 if starts is None else starts, n, _is_int_like, "starts")
    pts, cells = [], []
    for b in range(n):
        mesh = meshes[b]
        if not isinstance(mesh, _data.TriangleMesh):
            raise ValueError(f"item {b}: a data.TriangleMesh")
        p, c = mesh.points, mesh.cells.reshape(-1, 3)
        M = p.shape[0]
        if p.ndim != 2 or p.shape[1] != 3 or M < 1 or M > _DECIMATE_MAX_VERTICES or c.shape[0] > _DECIMATE_MAX_TRIANGLES:
            raise ValueError(f"item {b}: points are [1 .. 2^24, 3], at most 2^26 triangles")
        if c.size and (c.min() < 0 or c.max() >= M):
            raise ValueError(f"item {b}: a triangle's vertex id is out of range")
        if not (_is_int_like(ks[b]) and 1 <= ks[b] <= _DECIMATE_MAX_POINTS):
            raise ValueError(f"item {b}: the count is an integer in [1, {_DECIMATE_MAX_POINTS}]")
        if not (_is_int_like(ss[b]) and 0 <= ss[b] < M):
            raise ValueError(f"item {b}: the start is a vertex id in [0, {M})")
        with np.errstate(invalid="ignore"):
            if not np.all(np.abs(p) <= _DECIMATE_MAX_MAGNITUDE):
                raise ValueError(f"item {b}: every coordinate is finite and at most 2^60 in magnitude")
        pts.append(p); cells.append(np.ascontiguousarray(c, dtype=np.int32))
    n_pts = np.array([p.shape[0] for p in pts], dtype=np.int32)
    n_tri = np.array([c.shape[0] for c in cells], dtype=np.int32)
    k_arr, s_arr = np.array(ks, dtype=np.int32), np.array(ss, dtype=np.int32)
    ids = [np.zeros(k, dtype=np.int32) for k in ks] if "ids" in want else None
    spts = [np.zeros((k, 3)) for k in ks] if "points" in want else None
    cover = [np.zeros(k) for k in ks] if "cover2" in want else None
    labels = [np.zeros(p.shape[0], dtype=np.int32) for p in pts] if "labels" in want else None
    tris = [np.zeros((c.shape[0], 3), dtype=np.int32) for c in cells] if "cells" in want else None
    cnt = np.zeros(3 * n, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    out_d = lambda a: None if a is None else _ptr_array(a)  # noqa: E731
    out_i = lambda a: None if a is None else _ptr_array(a, nat.c_int_p, _i)  # noqa: E731
    rc = nat.lib().icp_decimate_many(n, int(device), _i(n_pts), _ptr_array(pts), _i(n_tri), _ptr_array(cells, nat.c_int_p, _i), _i(k_arr),
                                     _i(s_arr), _i(cnt), out_i(ids), out_d(spts), out_d(cover), out_i(labels), out_i(tris), _i(status))
    nat.check(rc, "icp_decimate_many")
    out = []
    for b in range(n):
        ke, to, sw = (int(x) for x in cnt[3 * b:3 * b + 3])
        item = {}
        if "ids" in want:
            item["ids"] = ids[b][:ke].copy()
        if "points" in want:
            item["points"] = spts[b][:ke].copy()
        if "cells" in want:
            item["cells"] = tris[b][:to].copy()
        if "labels" in want:
            item["labels"] = labels[b]
        if "cover2" in want:
            item["cover2"] = cover[b][:ke].copy()
        if "counts" in want:
            item["counts"] = (ke, to, sw)
        out.append(item)
    return out


def decimated_mesh(mesh, k, start=0, device=0, want=_DECIMATE_WANT) -> dict:
    """decimated_meshes for one mesh"""
    return decimated_meshes([mesh], [k], [start], device, want)[0]


_SAMPLES_MAX_VERTICES, _SAMPLES_MAX_TRIANGLES, _SAMPLES_MAX_COUNT, _SAMPLES_MAX_MAGNITUDE = 1 << 24, 1 << 26, 1 << 24, 2.0 ** 60
SAMPLES_NO_AREA = -3  # ICP_ERR_NOT_FINITE: an item whose every triangle is degenerate has nothing to draw from


@dataclasses.dataclass
class SurfaceSamples:
    """One item of surface_samples: `points` [n, 3], the triangle of every sample `cells` [n] int32, its barycentric weights `bary`
    [n, 3] (point = w0·a + w1·b + w2·c), the nearest vertex of every sample `vertex_ids` [n] int32 (None if not asked for; equal
    distances go to the lowest id), `info` = {"triangles": those with a positive weight, "largest_area", "area"} and `status`: 0, or
    -3 for a mesh without area (NaN points and weights, −1 ids)."""
    points: np.ndarray
    cells: np.ndarray
    bary: np.ndarray
    vertex_ids: np.ndarray
    info: dict
    status: int = 0


def surface_samples(meshes, counts, seeds, device=0, vertex_ids=True) -> list:
    """Uniform random points on the surfaces of many meshes in one call (icp_surface_samples_many; Scalismo's UniformMeshSampler3D;
    DESIGN.md §5.19): per item counts[b] points, a triangle drawn in proportion to its area and a point uniform in it, from the
    counter-based generator of the Dice samples under seeds[b] (0 <= seed < 2^64) — deterministic to the bit, and an item's points
    depend on nothing but its mesh, count and seed.  Areas are quantised to 2^-32 of the largest triangle: a smaller triangle is never
    drawn.  With `vertex_ids` every sample also gets its nearest vertex over the whole mesh (findClosestPoint(p).id; equal distances go
    to the lowest id); one flag for all items, or one per item.  One count or seed serves every item; a list holds one per item.
    -> one SurfaceSamples per item."""
    meshes = [meshes] if isinstance(meshes, _data.TriangleMesh) else list(meshes)
    n = len(meshes)
    if n == 0 or n > 65535:
        raise ValueError("at least one mesh, at most 65,535 a call")
    ks = _scan_per_item(counts, n, _is_int_like, "counts")
    sd = _scan_per_item(seeds, n, _is_int_like, "seeds")
    ids_wanted = _scan_per_item(vertex_ids, n, lambda v: isinstance(v, (bool, np.bool_)), "vertex_ids")
    pts, cells = [], []
    for b in range(n):
        mesh = meshes[b]
        if not isinstance(mesh, _data.TriangleMesh):
            raise ValueError(f"item {b}: a data.TriangleMesh")
        p, c = mesh.points, mesh.cells.reshape(-1, 3)
        M = p.shape[0]
        if p.ndim != 2 or p.shape[1] != 3 or M < 1 or M > _SAMPLES_MAX_VERTICES or not (1 <= c.shape[0] <= _SAMPLES_MAX_TRIANGLES):
            raise ValueError(f"item {b}: points are [1 .. 2^24, 3], 1 to 2^26 triangles")
        if c.min() < 0 or c.max() >= M:
            raise ValueError(f"item {b}: a triangle's vertex id is out of range")
        if not (_is_int_like(ks[b]) and 1 <= ks[b] <= _SAMPLES_MAX_COUNT):
            raise ValueError(f"item {b}: the count is an integer in [1, 2^24]")
        if not (_is_int_like(sd[b]) and 0 <= sd[b] < 2 ** 64):
            raise ValueError(f"item {b}: the seed is an integer in [0, 2^64)")
        if not isinstance(ids_wanted[b], (bool, np.bool_)):
            raise ValueError(f"item {b}: vertex_ids is True or False")
        with np.errstate(invalid="ignore"):
            if not np.all(np.abs(p) <= _SAMPLES_MAX_MAGNITUDE):
                raise ValueError(f"item {b}: every coordinate is finite and at most 2^60 in magnitude")
        pts.append(p); cells.append(np.ascontiguousarray(c, dtype=np.int32))
    n_pts = np.array([p.shape[0] for p in pts], dtype=np.int32)
    n_tri = np.array([c.shape[0] for c in cells], dtype=np.int32)
    k_arr, s_arr = np.array(ks, dtype=np.int32), np.array([int(s) for s in sd], dtype=np.uint64)
    spts = [np.zeros((k, 3)) for k in ks]
    scells = [np.zeros(k, dtype=np.int32) for k in ks]
    bary = [np.zeros((k, 3)) for k in ks]
    vids = [np.zeros(k, dtype=np.int32) if ids_wanted[b] else None for b, k in enumerate(ks)]
    info = np.zeros((n, 4))
    status = np.zeros(n, dtype=np.int32)
    rc = nat.lib().icp_surface_samples_many(n, int(device), _i(n_pts), _ptr_array(pts), _i(n_tri), _ptr_array(cells, nat.c_int_p, _i),
                                            _i(k_arr), s_arr.ctypes.data_as(nat.c_uint64_p), _ptr_array(spts),
                                            _ptr_array(scells, nat.c_int_p, _i), _ptr_array(bary), _ptr_array(vids, nat.c_int_p, _i),
                                            _ptr_array(list(info)), _i(status))
    if rc != 0 and (not status.any() or not np.all((status == 0) | (status == SAMPLES_NO_AREA))):
        nat.check(rc, "icp_surface_samples_many")  # a whole-call error, or an item the checks above should have refused
    return [SurfaceSamples(spts[b], scells[b], bary[b], vids[b],
                           {"triangles": int(info[b, 0]), "largest_area": float(info[b, 1]), "area": float(info[b, 2])}, int(status[b]))
            for b in range(n)]


def total_variance(points_list, kernels, point_weights=None, device=0) -> np.ndarray:
    """The mean trace of a kernel at given points, many in one call (icp_kernel_total_variance_many; apps/femur/CreateGPModel.scala:38-46,
    approxTotalVariance): item b is the mean over points_list[b] [n, 3] of trace k(x, x) for kernels[b], a kernel as gp_models takes it
    (`kernels`: one list of terms for every item, or one list per item).  A term's own `weights` belong to a mesh's vertices and are not
    read: a weighted term needs its region weights AT THESE POINTS, point_weights[b][t] ([n]; None for a term without weights; see
    region_weights).  One bare [n, 3] array is one item, and point_weights then that item's list.  The sum has a fixed shape that depends on n alone, so an item's bits depend on the item alone.  -> [n_items]."""
    single = isinstance(points_list, np.ndarray)
    ps = [points_list] if single else list(points_list)
    n = len(ps)
    if n == 0 or n > 65535:
        raise ValueError("at least one item, at most 65,535 a call")
    ks = list(kernels)
    if len(ks) > 0 and isinstance(ks[0], _KERNEL_TERMS):
        ks = [ks] * n
    if len(ks) != n:
        raise ValueError("kernels: one list of terms, or one list per item")
    pws = [None] * n if point_weights is None else [point_weights] if single else list(point_weights)
    if len(pws) != n:
        raise ValueError("point_weights: None, or one list (an entry per term) per item")
    keep, pts, terms, c_pws = [], [], [], []
    for b in range(n):
        p = _f64(ps[b])
        if p.ndim != 2 or p.shape[1] != 3 or not (1 <= p.shape[0] <= _SAMPLES_MAX_COUNT) or not np.all(np.isfinite(p)):
            raise ValueError(f"item {b}: points are [1 .. 2^24, 3] and finite")
        kb = list(ks[b])
        pw = [None] * len(kb) if pws[b] is None else list(pws[b])
        if len(pw) != len(kb):
            raise ValueError(f"item {b}: point_weights has one entry (None or [n]) per term")
        bare = [dataclasses.replace(k, weights=None) if isinstance(k, _KERNEL_TERMS) else k for k in kb]
        arr = _kernel_terms(b, bare, p, True, keep)
        c_pw = (nat.c_double_p * len(arr))()
        for t in range(len(arr)):
            if (kb[t].weights is not None) != (pw[t] is not None):
                raise ValueError(f"item {b}, term {t}: a term with weights needs them at these points (point_weights), a term without has none")
            if pw[t] is None:
                continue
            w = _f64(pw[t])
            if w.shape != (p.shape[0],) or not np.all(np.isfinite(w)) or not np.all(w >= 0.0) or not np.any(w > 0.0):
                raise ValueError(f"item {b}, term {t}: point weights are [n], finite, >= 0 and not all zero")
            keep.append(w)
            c_pw[t] = _d(w)
        pts.append(p); terms.append(arr); c_pws.append(c_pw)
    term_t = nat.KernelTermGeneral
    c_terms = (C.POINTER(term_t) * n)(*[C.cast(a, C.POINTER(term_t)) for a in terms])
    c_w = (C.POINTER(nat.c_double_p) * n)(*[C.cast(a, C.POINTER(nat.c_double_p)) for a in c_pws])
    n_pts = np.array([p.shape[0] for p in pts], dtype=np.int32)
    n_terms = np.array([len(a) for a in terms], dtype=np.int32)
    out = np.zeros(n)
    status = np.zeros(n, dtype=np.int32)
    rc = nat.lib().icp_kernel_total_variance_many(n, int(device), _i(n_pts), _ptr_array(pts), _i(n_terms), c_terms, c_w, _d(out), _i(status))
    nat.check(rc, "icp_kernel_total_variance_many")
    return out
