/*
 * icp_proposal.h — C ABI of the MI355X-native closest-point-proposal path (libicp_proposal_amd.so).
 *
 * This is the drop-in boundary for ONE hot path of unibas-gravis/icp-proposal: the three Scalismo plug-in
 * methods the Metropolis–Hastings chain calls per step,
 *
 *     ProposalGenerator[ModelFittingParameters].propose(current)
 *     TransitionProbability[ModelFittingParameters].logTransitionProbability(from, to)
 *     DistributionEvaluator[ModelFittingParameters].logValue(sample)
 *
 * as implemented by the reference classes cited at each entry point below (paths relative to the reference's
 * src/main/scala/).  The reference has no FFI of its own (pure Scala on Scalismo); INTEGRATION.md shows the
 * JNI stub + Scala adapters a maintainer would add to bind these symbols.
 *
 * Conventions
 *   - plain pointers and sizes only; all floating point is IEEE double, all ids int32; arrays are row-major.
 *   - theta = ModelFittingParameters.allParameters (ModelFittingParameters.scala:64):
 *       [ s | tx ty tz | phi theta psi | cx cy cz | c_0 .. c_{r-1} ]      (10 + rank doubles)
 *     pose = translation ∘ rotation(phi,theta,psi about c) with R = Rz(phi)·Ry(theta)·Rx(psi)
 *     (ModelFittingParameters.scala:79-86), scale applied last (:88-106).
 *   - every function returns an icp_status (0 = ok, < 0 = error); outputs are written into caller-owned buffers;
 *     the library copies model/target to the GPU once at icp_ctx_create and keeps no pointer to caller memory.
 *   - -inf is a VALID value of icp_proposal_log_transition (NonRigidIcpProposal.scala:72-74).
 *   - entry points are thread-safe (calls on one context are serialised internally); the random numbers of
 *     posterior.sample() (NonRigidIcpProposal.scala:55) are drawn by the CALLER and passed in as z.
 *   - there is no CPU fallback: if no HIP device is usable, icp_ctx_create fails with ICP_ERR_DEVICE.
 */
#ifndef ICP_PROPOSAL_H
#define ICP_PROPOSAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICP_API __attribute__((visibility("default")))

typedef struct icp_ctx icp_ctx;             /* one statistical mesh model + one target mesh, resident on one GPU */
typedef struct icp_proposal icp_proposal;   /* api/sampling/proposals/NonRigidIcpProposal.scala:30-41 */
typedef struct icp_evaluator icp_evaluator; /* the classes under api/sampling/evaluators/ */

typedef enum {
  ICP_OK = 0,
  ICP_ERR_INVALID_ARG = -1, /* null pointer, negative size, id out of range, unknown enum */
  ICP_ERR_DEVICE = -2,      /* HIP runtime / no device / out of memory (icp_last_error() has the HIP string) */
  ICP_ERR_NOT_FINITE = -3,  /* a result is NaN (the Scalismo chain throws on NaN transition probabilities) */
  ICP_ERR_NOT_SPD = -4,     /* a normal-equation matrix failed to factor */
  ICP_ERR_EMPTY = -5,       /* boundary-aware evaluator dropped every point (reference: empty .max throws) */
  ICP_ERR_BUSY = -6,        /* the context is part of a batch between icp_chain_step_batched_issue and _collect / _abandon */
  ICP_ERR_NOT_CONVERGED = -7 /* icp_nystrom_models_many: an item's iteration hit its cap on sweeps (its outputs are written all the same) */
} icp_status;

/* api/other/IcpProjectionDirection.scala:19-25.  ModelAndTargetSampling is not a proposal direction: the
 * reference builds TWO proposals and mixes them (api/sampling/MixedProposalDistributions.scala:52-65). */
typedef enum { ICP_MODEL_SAMPLING = 0, ICP_TARGET_SAMPLING = 1 } icp_direction;

/* api/sampling/evaluators/EvaluationModeType.scala:20-26 */
typedef enum { ICP_MODEL_TO_TARGET = 0, ICP_TARGET_TO_MODEL = 1, ICP_SYMMETRIC = 2 } icp_eval_mode;

typedef enum {
  ICP_EVAL_INDEPENDENT_POINT_DISTANCE = 0, /* evaluators/IndependentPointDistanceEvaluator.scala:27-67 */
  ICP_EVAL_HAUSDORFF = 1,                  /* evaluators/HausdorffDistanceEvaluator.scala:25-36 */
  ICP_EVAL_COLLECTIVE_AVG_HAUSDORFF_BOUNDARY_AWARE = 2 /* evaluators/CollectiveAverageHausdorffDistanceBoundaryAwareEvaluator.scala:27-79 */
} icp_eval_kind;

/* What crosses the boundary of a Scalismo StatisticalMeshModel (Statismo layout). */
typedef struct {
  int32_t n_points;               /* N */
  int32_t n_triangles;            /* T */
  int32_t rank;                   /* r */
  const double *ref_points;       /* [N*3]  reference mesh vertices */
  const double *mean_deformation; /* [N*3]  GP mean at the reference vertices (NULL = zero) */
  const double *basis;            /* [3N*r] UNSCALED eigenfunctions, row 3i+d = vertex i axis d */
  const double *variance;         /* [r]    eigenvalues */
  const int32_t *triangles;       /* [T*3] */
} icp_model_desc;

typedef struct {
  int32_t n_points;
  int32_t n_triangles;
  const double *points;     /* [M*3] */
  const int32_t *triangles; /* [Tt*3] */
} icp_mesh_desc;

/* Constructor arguments of NonRigidIcpProposal (NonRigidIcpProposal.scala:30-41).  The two decimations at
 * :45-46 stay with the caller (Scalismo): only their outcome crosses the boundary — the COUNT of points of the
 * decimated model (the reference uses ids 0 until K of the full mesh, :94-96) and the POINTS of the decimated
 * target (:117). */
typedef struct {
  double step_length;        /* :33 */
  double tangential_noise;   /* :34 stddev in the tangent plane */
  double noise_along_normal; /* :35 stddev along the vertex normal */
  int32_t direction;         /* :37 icp_direction */
  int32_t boundary_aware;    /* :38 */
  int32_t n_model_ids;       /* ModelSampling: number of points of model.decimate(numOfSamplePoints) */
  int32_t n_target_points;   /* TargetSampling: number of points of target.operations.decimate(numOfSamplePoints) */
  const double *target_points; /* [n_target_points*3] */
} icp_proposal_params;

/* Constructor arguments of the three likelihood evaluators; the likelihood distributions are the Breeze
 * objects built in api/sampling/ProductEvaluators.scala:39,58,77-78. */
typedef struct {
  int32_t kind;            /* icp_eval_kind */
  int32_t mode;            /* icp_eval_mode (ignored by ICP_EVAL_HAUSDORFF) */
  int32_t n_model_ids;     /* number of points of model.decimate(numberOfPointsForComparison); ids 0 until K */
  int32_t n_target_points; /* points of targetMesh.operations.decimate(numberOfPointsForComparison) */
  const double *target_points;
  double gauss_mean;       /* Gaussian(mean, sigma): kind 0 (per-point distance) and kind 2 (average distance) */
  double gauss_sigma;
  double exp_rate;         /* Exponential(rate): kind 1 (Hausdorff distance) and kind 2 (max distance) */
} icp_evaluator_params;

/* Diagnostic view of one ICP posterior (NonRigidIcpProposal.scala:88-153); any pointer may be NULL. */
typedef struct {
  int32_t n_candidates;   /* out: K (before the boundary filter) */
  int32_t *corr_id;       /* [K]   model vertex id of each correspondence — THE correspondence index (:118 / :94) */
  int32_t *corr_aux;      /* [K]   ModelSampling: target vertex nearest to the surface point (:98), else -1 */
  double *corr_point;     /* [K*3] target-side point (:97 / :117) */
  uint8_t *keep;          /* [K]   1 = survives the boundary filter (:104 / :124) */
  double *alpha;          /* [r]   posterior mean coefficients */
  double *M;              /* [r*r] I + sum_i Q_i^T Sigma_i^-1 Q_i */
  double *V;              /* [r*r] eigenvectors (columns) of D M^-1 D — the posterior KL basis is Phi·V */
  double *S;              /* [r]   its eigenvalues, descending */
} icp_posterior_view;

/* ---------------------------------------------------------------- context */

/* device: HIP ordinal, or -1 = use LOCAL_RANK from the environment (0 if unset). */
ICP_API int icp_ctx_create(const icp_model_desc *model, const icp_mesh_desc *target, int device, icp_ctx **out);
/* The same for a caller that makes MANY contexts from one model (one per chain of a batch registration: SURVEY.md §8e).  Contexts of a
 * device made from the same model share its device data; icp_ctx_create recognises the model by hashing its arrays — 137 MB of basis at
 * the face model's size, 6.6 ms per context.  model_key != 0: the caller vouches that equal keys mean equal model arrays (an object
 * id, a hash taken once); the library then hashes the key, the small arrays and a sample of the basis only (0.3 ms), and while the FIRST
 * context of a keyed model does its one-off host work, the streams of the contexts to come can be made by a helper thread
 * (icp_ctx_expect; hipStreamCreateWithPriority: 2.4 ms each; ICP_NO_STREAM_PREWARM=1: not).  0 = icp_ctx_create. */
ICP_API int icp_ctx_create_keyed(const icp_model_desc *model, const icp_mesh_desc *target, int device, uint64_t model_key, icp_ctx **out);
/* Optional hint of a host that is about to make n_contexts contexts on `device` (one per chain of a batch registration, one per chain
 * thread of a `.par` experiment): their streams — three quarters of what a further context costs — are made ahead by a helper thread
 * while the caller's first icp_ctx_create_keyed does the model's one-off host work.  Never changes results; at most 64 are made; a
 * host with one chain per GPU simply does not call it (until round 6 every first keyed context made two dozen unasked). */
ICP_API int icp_ctx_expect(int device, int32_t n_contexts);
ICP_API void icp_ctx_destroy(icp_ctx *ctx);
/* Gives the context ANOTHER target mesh and keeps everything that does not depend on the target — the model's device data, the
 * per-chain scratch, streams, pinned buffers: a batch registration (one statistical model against many targets:
 * apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:106-163) makes its contexts once.  The context must have no proposal and no
 * evaluator at the time (they are made for one target: destroy them first, create new ones afterwards); what it had cached against the
 * old target is dropped.  Creating a context costs 20+ ms at the face model's size, this call a fraction of a millisecond once the
 * target's own device data exists. */
ICP_API int icp_ctx_set_target(icp_ctx *ctx, const icp_mesh_desc *target);
ICP_API const char *icp_status_string(int status);
ICP_API const char *icp_last_error(void); /* thread-local detail of the last failing call */
ICP_API int icp_ctx_rank(const icp_ctx *ctx);
ICP_API int icp_ctx_device(const icp_ctx *ctx);

/* Pose across the boundary.  theta carries the three Euler angles; the reference turns them into a rotation with
 * Scalismo's Rotation(phi, theta, psi, centre) (ModelFittingParameters.scala:79-86).  A caller that wants Scalismo's OWN matrix
 * used — whatever its convention — registers it for the triple before passing a theta with these angles: R = row-major 3x3 rotation
 * (checked: orthonormal, determinant +1); R == NULL withdraws the entry.  Up to 32 triples are remembered (least recently used
 * out); a theta whose angles have no entry is posed with the library's Rz(phi)·Ry(theta)·Rx(psi).  Whenever the matrix in force
 * for a triple changes — first registration, replacement by a different matrix, withdrawal, eviction — everything the context has
 * cached under thetas with these angles (instances, posteriors of every proposal, memoised likelihood values) is dropped, so a
 * later call recomputes it with the new matrix; registering before the first use of a triple costs nothing. */
ICP_API int icp_ctx_set_rotation(icp_ctx *ctx, const double angles[3], const double R[9]);
/* The convention check behind it: every matrix handed to icp_ctx_set_rotation is compared with the library's own
 * Rz(phi)·Ry(theta)·Rx(psi) for the same angles (include/icp_sincos.h).  *verified counts the matrices that agreed to rounding
 * (2e-15 per entry), *mismatched the ones that did not (either may be NULL).  A host with mismatched == 0 — the Scala adapter, if
 * Scalismo's Rotation(phi, theta, psi, centre) is Rz·Ry·Rx as SURVEY App. B8 assumes — may run mixtures WITH pose walks through
 * icp_chains_run_on_device, where the proposed pose's matrix is made on the device; one mismatch closes that path for the context
 * (ICP_ERR_INVALID_ARG there; every host-stepped entry point keeps using the caller's matrices as before). */
ICP_API int icp_ctx_rotation_convention(icp_ctx *ctx, int64_t *verified, int64_t *mismatched);

/* ModelFittingParameters.transformedMesh (ModelFittingParameters.scala:108-110): points_out [N*3]. */
ICP_API int icp_transformed_mesh(icp_ctx *ctx, const double *theta, double *points_out);
/* vertex normals of that mesh (Scalismo vertexNormals, used at NonRigidIcpProposal.scala:100,120): [N*3]. */
ICP_API int icp_vertex_normals(icp_ctx *ctx, const double *theta, double *normals_out);

/* The two brute-force searches, exposed for parity tests and micro-benchmarks.
 * icp_closest_point_on_target : target.operations.closestPointOnSurface(p).point (NonRigidIcpProposal.scala:97);
 * icp_closest_target_vertex   : target.pointSet.findClosestPoint(p).id            (:98);
 * icp_closest_model_vertex    : currentMesh.pointSet.findClosestPoint(p).id for the mesh of theta (:118);
 * icp_closest_point_on_model  : modelSample.operations.closestPointOnSurface(p) (IndependentPointDistanceEvaluator.scala:51).
 * Ties: lowest squared distance, then lowest index.  Any output pointer may be NULL. */
ICP_API int icp_closest_point_on_target(icp_ctx *ctx, int32_t n, const double *queries, double *points_out,
                                        int32_t *triangle_out, double *dist2_out);
ICP_API int icp_closest_target_vertex(icp_ctx *ctx, int32_t n, const double *queries, int32_t *id_out, double *dist2_out);
ICP_API int icp_closest_model_vertex(icp_ctx *ctx, const double *theta, int32_t n, const double *queries,
                                     int32_t *id_out, double *dist2_out);
ICP_API int icp_closest_point_on_model(icp_ctx *ctx, const double *theta, int32_t n, const double *queries,
                                       double *points_out, int32_t *triangle_out, double *dist2_out);

/* ---------------------------------------------------------------- NonRigidIcpProposal */

ICP_API int icp_proposal_create(icp_ctx *ctx, const icp_proposal_params *params, icp_proposal **out);
ICP_API void icp_proposal_destroy(icp_proposal *p);

/* propose (NonRigidIcpProposal.scala:53-68).  z[r] = the standard normals posterior.sample() draws (:55);
 * theta_out[10+r] = theta with the shape coefficients replaced (:61-66).  corr_id_out (optional, [K]) receives
 * the correspondence indices of the posterior that was used, -1 where the boundary filter dropped one. */
ICP_API int icp_proposal_propose(icp_proposal *p, const double *theta, const double *z, double *theta_out,
                                 int32_t *corr_id_out);

/* logTransitionProbability(from, to) (NonRigidIcpProposal.scala:71-85). */
ICP_API int icp_proposal_log_transition(icp_proposal *p, const double *theta_from, const double *theta_to, double *out);

/* Opt-in, NOT the reference's arithmetic: how propose() turns the caller's standard normals z into a sample of the posterior.
 *   ICP_SAMPLER_EIGEN (default)   z multiplies the posterior's KL basis, D M^-1 D = V S V^T (what Scalismo's posterior.sample() does,
 *                                 NonRigidIcpProposal.scala:55): parity with the reference for a given z; needs the eigen-decomposition
 *                                 of every accepted state's posterior, the longest link of an accepted step.
 *   ICP_SAMPLER_CHOLESKY_ROOT     z multiplies W = D L^-T (M = L L^T): W W^T = D M^-1 D as well, so the sample has the SAME distribution
 *                                 and logTransitionProbability (which does not depend on the root) is unchanged — the chain
 *                                 is a different realisation of the same Markov kernel.  No eigen-decomposition at all: D^-1 W z = L^-T z
 *                                 is one back substitution per proposal.  The diagnostic view then returns V = L (row-major lower
 *                                 triangle) and S = 1 / diag(L).  Ranks <= 256 (up to 64: a kernel of its own where the decomposition
 *                                 would run; above: the posterior's factorisation hands its factor out).
 * Call before the proposal's first use, or any time: posteriors already decomposed the other way are decomposed again. */
typedef enum { ICP_SAMPLER_EIGEN = 0, ICP_SAMPLER_CHOLESKY_ROOT = 1 } icp_sampler;
ICP_API int icp_proposal_set_sampler(icp_proposal *p, int32_t sampler);

/* icpPosterior(theta) (NonRigidIcpProposal.scala:88-153), diagnostic. */
ICP_API int icp_proposal_posterior(icp_proposal *p, const double *theta, icp_posterior_view *view);
ICP_API int icp_proposal_num_candidates(const icp_proposal *p);

/* ---------------------------------------------------------------- evaluators */

ICP_API int icp_evaluator_create(icp_ctx *ctx, const icp_evaluator_params *params, icp_evaluator **out);
ICP_API void icp_evaluator_destroy(icp_evaluator *e);

/* logValue(sample) of the likelihood evaluator (computeLogValue of the three evaluator classes).
 * aux (optional, [4]): kind 0 -> {modelToTarget sum, targetToModel sum, 0, 0}; kind 1 -> {hausdorff, m2t max, t2m max, 0};
 * kind 2 -> {avg, max, n kept model->target, n kept target->model}. */
ICP_API int icp_evaluator_log_value(icp_evaluator *e, const double *theta, double *out, double *aux);

/* ModelPriorEvaluator.logValue (evaluators/ModelPriorEvaluator.scala:24-31): O(r) host arithmetic. */
ICP_API int icp_prior_log_value(int32_t rank, const double *theta, double *out);

/* ---------------------------------------------------------------- deterministic non-rigid ICP
 * IcpBasedSurfaceFitting.runfitting (api/other/IcpBasedSurfaceFitting.scala:46-126), the paper's comparison baseline: for every
 * sigma2 of the sequence (:36-40: 1, 0.1, 0.01) the recursion (:55-104) runs numIterations + 1 times: instance, correspondences
 * in one direction (:71-79), GP regression with ISOTROPIC noise sigma2 (:81), posterior MEAN (:82), its coefficients (:84), step
 * (:85).  The sample ids / sample points are drawn by Scalismo's UniformMeshSampler3D in the reference (:51-53) and are inputs
 * here (icp_surface_samples_many draws such ids and points); so is the per-iteration direction draw of ModelAndTargetSampling (:66-69: icp_fit_deterministic_many takes a schedule
 * of directions).  All iterations run on the device without host round trips.  theta_out = theta_init with the fitted shape
 * coefficients. */
typedef struct {
  int32_t direction;             /* icp_direction */
  int32_t n_model_ids;           /* ModelSampling: pointIds (:53), any ids, repeats allowed */
  const int32_t *model_ids;
  int32_t n_target_points;       /* TargetSampling: targetPointSamples (:51) */
  const double *target_points;
  double step_length;            /* :32 (default 1.0) */
} icp_fit_params;
ICP_API int icp_fit_deterministic(icp_ctx *ctx, const icp_fit_params *params, const double *theta_init, int32_t n_iterations,
                                  int32_t n_sigma, const double *sigma2_seq, double *theta_out);

/* Many deterministic fits in lockstep on one stream, one synchronisation per call (the study's 100 inits per target).
 * ctxs[b]: fit b's context; repeats allowed (the inits of one target share its context).  All contexts share one device and one
 * model.  directions: NULL (every recursion of fit b takes params[b]->direction) or [n_fits][n_sigma*(n_iterations+1)] bytes of
 * ICP_MODEL_SAMPLING / ICP_TARGET_SAMPLING, recursion si*(n_iterations+1)+it — ModelAndTargetSampling's per-recursion draw (:63-69).
 * A fit that uses a side needs a non-empty sample list for it.  Fit b's result is what icp_fit_deterministic gives when called once
 * per recursion (n_iterations = 0, one sigma2, that recursion's direction), each theta_out chained into the next theta_init; its
 * bits do not depend on the other fits of the call or their order.  The pose is left as it is.
 * ICP_ERR_INVALID_ARG (null pointers, mixed models or devices, unknown direction byte, non-finite theta_init, id out of range, bad
 * sigma2, missing samples): nothing has run, no theta_out is written.  Otherwise status[b] = ICP_OK / ICP_ERR_NOT_SPD /
 * ICP_ERR_NOT_FINITE per fit (a failed fit's theta_out is left untouched) and the return value is ICP_OK or the first failing fit's. */
ICP_API int icp_fit_deterministic_many(int32_t n_fits, icp_ctx *const *ctxs, const icp_fit_params *const *params,
                                       const double *const *theta_init, const uint8_t *directions, int32_t n_iterations,
                                       int32_t n_sigma, const double *sigma2_seq, double *const *theta_out, int32_t *status);

/* ---------------------------------------------------------------- posterior variability maps
 * apps/util/PosteriorVariability.scala:30-73 over n_samples logged chain states (thetas [n_samples*(10+r)]):
 *   mode 0: trace of the per-vertex sample covariance (computeDistanceMapFromMeshesTotal :30-49);
 *   mode 1: variance along the unit vertex normals of the mesh of theta_ref (computeDistanceMapFromMeshesNormal, sumNormals = false);
 *   mode 2: variance along the mean (not renormalised) of the samples' unit vertex normals (sumNormals = true, :63-65).
 * out [N].  n_samples >= 2. */
ICP_API int icp_posterior_variability(icp_ctx *ctx, int32_t n_samples, const double *thetas, int32_t mode, const double *theta_ref,
                                      double *out);

/* ---------------------------------------------------------------- registration metrics
 * api/other/RegistrationComparison.scala:24-49 between the mesh of theta (reconstruction) and the target (ground truth):
 *   out[0] = MeshMetrics.avgDistance(reconstruction, target)       mean vertex-to-surface distance              (:25)
 *   out[1] = MeshMetrics.hausdorffDistance(reconstruction, target) max over both directions                     (:27)
 *   out[2], out[3] = boundary-aware average and maximum: reconstruction vertices whose closest target point's nearest target
 *                    vertex lies on the target's boundary are dropped                                           (:31-42)
 *   out[4] = number of vertices kept by that filter. */
ICP_API int icp_mesh_metrics(icp_ctx *ctx, const double *theta, double *out /* [5] */);

/* Registration metrics of many meshes in one call, one synchronisation (the experiment summary of
 * apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:43-64: avg / hausdorff / dice of every scored mesh against its target).
 * Item b scores the mesh of thetas[b], pose included, against ctxs[b]'s target.  Contexts may repeat; all share one device and one
 * model, targets may differ.  out[9b+0..4] = the bits of icp_mesh_metrics(ctxs[b], thetas[b]); out[9b+5] = Dice; out[9b+6..8] =
 * nA, nB, nAB.  With dice_samples == 0 Dice is skipped and out[9b+5..8] are NaN.
 * Dice, MeshMetrics.diceCoefficient of Scalismo 0.90 as recalled [SCALISMO-UNVERIFIED]: S = dice_samples points uniform in the union
 * of the two meshes' axis-aligned boxes, p_k = lo_k + u(s,k)·(hi_k − lo_k) (subtract, multiply, add, each rounded) with
 * u(s,k) = orc_rng_uniform(dice_seed, s, k) — the same points whatever the item's place in the batch.  p is inside a mesh iff, with v
 * its nearest vertex (ties: lowest index) and n v's vertex normal, (n.x(v.x−p.x) + n.y(v.y−p.y)) + n.z(v.z−p.z) > 0.  nA / nB =
 * samples inside the reconstruction / the target, nAB = inside both, dice = 2·nAB / (nA + nB) (NaN when nA + nB == 0).  The rule is
 * evaluated for any mesh but means something for closed meshes only; its parity with Scalismo's own sampler and inside test is not
 * pinned (no Scalismo source here).
 * ICP_ERR_INVALID_ARG (null pointers, n_items outside [1, 65535], dice_samples outside [0, 2^24], a non-finite theta, mixed devices
 * or models): nothing has run, nothing is written.  ICP_ERR_BUSY: a context belongs to a batch in flight.  Otherwise status[b] =
 * ICP_OK, or ICP_ERR_NOT_FINITE for an item whose mesh is not finite (its out row is NaN), and the return value is ICP_OK or the
 * first failing item's.  An item's bits depend neither on the other items nor on their order. */
ICP_API int icp_mesh_metrics_many(int32_t n_items, icp_ctx *const *ctxs, const double *const *thetas, int32_t dice_samples,
                                  uint64_t dice_seed, double *out /* [n_items*9] */, int32_t *status /* [n_items] */);

/* Per-vertex registration maps of many meshes in one call, one synchronisation: what icp_mesh_metrics_many computes for every item
 * and reduces to five numbers, handed out row by row (the colour-coded distance map of a fit; a dense correspondence set).  Item b
 * is the mesh x = icp_transformed_mesh(ctxs[b], thetas[b]), N model vertices, against ctxs[b]'s target of M_b vertices.  Contexts
 * may repeat; all share one device and one model, targets may differ.  Every output is an array of n_items pointers, one array per
 * item, or NULL for "not wanted":
 *   m2t_point[b]       [N*3]   the bits of icp_closest_point_on_target(ctxs[b], N, x, ...)'s points
 *   m2t_triangle[b]    [N]     ... its triangle indices
 *   m2t_distance[b]    [N]     sqrt of its squared distances, the expression icp_mesh_metrics reduces
 *   m2t_on_boundary[b] [N]     1 iff the nearest target vertex of m2t_point (icp_closest_target_vertex) is a boundary vertex of the
 *                              target — the filter of api/other/RegistrationComparison.scala:31-42; all 0 for a target without
 *                              boundary, whose nearest vertices are then not searched
 *   t2m_point[b]       [M_b*3] the bits of icp_closest_point_on_model(ctxs[b], thetas[b], M_b, target vertices, ...)'s points
 *   t2m_triangle[b]    [M_b]   ... its triangle indices
 *   t2m_distance[b]    [M_b]   sqrt of its squared distances
 * A direction none of whose outputs is wanted is not searched.  Device memory does not grow with n_items: the rows stream to the
 * caller through a fixed staging buffer.
 * ICP_ERR_INVALID_ARG (null pointers or entries, n_items outside [1, 65535], every output NULL, a non-finite theta, mixed devices or
 * models) and ICP_ERR_BUSY (a context belongs to a batch in flight): nothing has run, nothing is written.  Otherwise status[b] =
 * ICP_OK, or ICP_ERR_NOT_FINITE for an item whose mesh is not finite (its rows are NaN, its triangles -1, its flags 0), and the
 * return value is ICP_OK or the first failing item's.  An item's bits depend neither on the other items nor on their order. */
ICP_API int icp_registration_maps_many(int32_t n_items, icp_ctx *const *ctxs, const double *const *thetas, double *const *m2t_point,
                                       int32_t *const *m2t_triangle, double *const *m2t_distance, uint8_t *const *m2t_on_boundary,
                                       double *const *t2m_point, int32_t *const *t2m_triangle, double *const *t2m_distance,
                                       int32_t *status /* [n_items] */);

/* The distance maps a chain's samples imply, for many chains in one call, one synchronisation.  Set m holds the n_samples[m] >= 1
 * states theta_sets[m] ([n_samples[m] * (10 + rank)]) on ctxs[m]; with d_s the distances icp_registration_maps_many gives for state
 * s, per vertex
 *   mean = (((d_0 + d_1) + d_2) + ...) / n_samples[m]   (added left to right in sample order, then ONE division)
 *   max  = the maximum of the same distances.
 * m2t_mean[m], m2t_max[m] [N]; t2m_mean[m], t2m_max[m] [M_m].  An output array may be NULL; a direction neither of whose outputs
 * is wanted is not searched.  The per-state maps never leave the device.  At most 2^24 samples a call.
 * Errors as icp_registration_maps_many (n_sets outside [1, 65535], a set without samples: ICP_ERR_INVALID_ARG, nothing written);
 * status[m] = ICP_ERR_NOT_FINITE for a set one of whose samples has a non-finite mesh (its rows are NaN).  A set's bits depend
 * neither on the other sets nor on their order. */
ICP_API int icp_distance_summaries_many(int32_t n_sets, icp_ctx *const *ctxs, const int32_t *n_samples, const double *const *theta_sets,
                                        double *const *m2t_mean, double *const *m2t_max, double *const *t2m_mean,
                                        double *const *t2m_max, int32_t *status /* [n_sets] */);

/* Log values of many states under many evaluators in one call, one synchronisation (the reference's logger scores every named
 * evaluator on every logged sample: JSONAcceptRejectLogger.scala:84-106; re-scoring a chain's log under another likelihood).
 * Item b delivers in values[b], aux[4b..4b+3] and status[b] the bits of icp_evaluator_log_value(evaluators[b], thetas[b], ...) on a
 * fresh evaluator, for every kind and mode, closed or open targets, ICP_ERR_EMPTY included.  Evaluators may repeat, differ in kind,
 * mode and parameters and belong to different contexts (targets); all contexts share one device and one model.  The call leaves the
 * evaluators and their contexts as they were: no memo, bind state, state slot or hint is read or written, and a chain stepped
 * around the call produces the records it would have produced without it.
 * ICP_ERR_INVALID_ARG (null pointers or entries, n_items outside [1, 65535], a non-finite theta, mixed devices or models) and
 * ICP_ERR_BUSY (a context belongs to a batch in flight): nothing has run, nothing is written.  Otherwise status[b] = ICP_OK,
 * ICP_ERR_EMPTY or ICP_ERR_NOT_FINITE as the one-item call reports it, and the return value is ICP_OK or the first status that is
 * neither ICP_OK nor ICP_ERR_EMPTY.  An item's bits depend neither on the other items nor on their order. */
ICP_API int icp_evaluator_log_values_many(int32_t n_items, icp_evaluator *const *evaluators, const double *const *thetas,
                                          double *values /* [n_items] */, double *aux /* [4 * n_items], may be NULL */,
                                          int32_t *status /* [n_items] */);

/* Posterior variability maps of many chains in one call, one synchronisation (PosteriorVariabilityToMeshColor's maps for every chain
 * of apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala).  Map m is computed from the n_samples[m] states thetas[m]
 * ([n_samples[m] * (10 + rank of ctxs[m])], poses included, registered rotation matrices honoured) in modes[m] (0, 1, 2 as in
 * icp_posterior_variability); theta_refs[m] is read where modes[m] == 1 and may be NULL elsewhere (theta_refs itself may be NULL when
 * no map has mode 1).  Contexts may repeat and may differ in model and rank; all are on one device.
 *   - Same bits as the one-map call: out[m] ([N_m]) equals, bit for bit, what icp_posterior_variability(ctxs[m], n_samples[m],
 *     thetas[m], modes[m], theta_refs[m], .) returns, whatever else the batch holds and however the samples fall into chunks.
 *   - mean_out: NULL, or per map NULL or [3 * N_m]: the per-vertex mean (sum_s x_s) * (1/S) the map is centred on, i.e. the posterior
 *     mean mesh, with the sum taken in sample order.
 *   - Working memory does not grow with the number of sample meshes: they pass through one chunk buffer of 64 MiB (meshes and, in
 *     mode 2, their vertex normals).  A map larger than the buffer is instanced twice, once for the sums and once for the centred
 *     moments.  Besides the buffer the call holds 10 * N_m doubles per map and the samples' coefficients and poses
 *     (rank + 18 doubles per sample).
 *   - Launches: at most four per chunk, however many maps, contexts and models the chunk holds.
 * ICP_ERR_INVALID_ARG (a null entry, n_maps < 0 or > 65535, fewer than two samples, an unknown mode, mode 1 without a reference,
 * contexts on two devices, a non-finite theta): nothing has run, nothing is written.  ICP_ERR_BUSY: a context belongs to a batch
 * in flight.  n_maps == 0 is accepted and does nothing. */
ICP_API int icp_posterior_variability_many(int32_t n_maps, icp_ctx *const *ctxs, const int32_t *n_samples,
                                           const double *const *thetas, const int32_t *modes, const double *const *theta_refs,
                                           double *const *out, double *const *mean_out);

/* ---------------------------------------------------------------- model projection of many meshes
 * Scalismo's model.instance / model.coefficients / model.project for many items in one call, one synchronisation
 * (apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:53-55 logs model.coefficients(best mesh) of 300 meshes per target;
 * RunMHRandomInitComparison.scala:72 starts every chain from model.coefficients(initShape)).
 *
 * icp_model_instances_many: points_out[b] ([3 * N_b]) = the bits of icp_transformed_mesh(ctxs[b], thetas[b], .), pose and registered
 * rotation matrices included.  Contexts may repeat and may differ in model and rank; all are on one device. */
ICP_API int icp_model_instances_many(int32_t n_items, icp_ctx *const *ctxs, const double *const *thetas,
                                     double *const *points_out /* [3*N] each */);

/* icp_model_coefficients_many, per item b (all contexts share one device and ONE model; they may repeat):
 *   - the mesh: exactly one of points[b] ([3 * N] vertices in the model's vertex order) and thetas[b] (the state whose
 *     transformedMesh is meant, instanced on the device with its pose: only 10 + rank doubles go up) is non-NULL; either array
 *     pointer may itself be NULL when no item uses it.
 *   - poses (NULL, or per item NULL or 10 doubles [s | t | angles | centre], s exactly 1): the inverse rigid pose
 *     R^T((p - t) - ctr) + ctr is applied to the vertices first, with the context's registered rotation matrix where the angles have
 *     one.  Without a pose the mesh is taken to be in model space, as model.coefficients takes it.
 *   - coeffs_out[b * rank ..] = c = P * Q^T (x - ref - mean) with Q = basis * sqrt(variance) and the context's resident
 *     P = (Q^T Q + sigma2 I)^-1, sigma2 = 1e-5: DiscreteLowRankGaussianProcess.coefficients as NonRigidIcpProposal.scala:59 and
 *     IcpBasedSurfaceFitting.scala:84 call it.  Of a model instance with coefficients c0 this is c0 - sigma2 * P * c0, not c0.
 *   - project_out (NULL, or per item NULL or [3 * N]) = model.project(mesh): the instance of c, under the item's pose where one was
 *     taken off; its bits equal icp_transformed_mesh of [pose or (1, 0, ..., 0) | c].
 * The meshes pass through a chunk buffer of 32 MiB, with as much again (rounded up to 16 meshes) for the residuals and at most as much
 * for partial sums: no mesh outlives its chunk.  Besides these the call holds rank doubles and a 144-byte record per item (and an
 * instance record of 144 bytes per item given as a state or projected).
 * An item's bits depend neither on the other items, nor on their order, nor on how the items fall into chunks.
 * Limits: no scale in the pose to take off; one model per call; meshes need the model's vertex count and order (no correspondence
 * is built here).
 * ICP_ERR_INVALID_ARG (a null entry, n_items outside [1, 65535], both or neither of points / theta for an item, a non-finite theta
 * or pose, s != 1 in a pose, mixed devices — or, for the coefficients, mixed models): nothing has run, nothing is written.
 * ICP_ERR_BUSY: a context belongs to a batch in flight.  Otherwise status[b] = ICP_OK, or ICP_ERR_NOT_FINITE for an item whose mesh
 * has a non-finite vertex (its coefficient row and projection are NaN; the other items are untouched), and the return value is
 * ICP_OK or the first failing item's. */
ICP_API int icp_model_coefficients_many(int32_t n_items, icp_ctx *const *ctxs, const double *const *points,
                                        const double *const *thetas, const double *const *poses,
                                        double *coeffs_out /* [n_items*rank] */, double *const *project_out,
                                        int32_t *status /* [n_items] */);

/* ---------------------------------------------------------------- fused chain step (measurement harness)
 * One call = all device work one Metropolis–Hastings step needs for a NEW state theta_prop proposed from
 * theta_cur, submitted as one stream sequence with a single synchronisation: the likelihood of theta_prop and,
 * for each of the n_props proposals, logT(cur -> prop) and logT(prop -> cur).  Results are identical to the
 * per-method entry points above (same kernels, same caches); only the number of host round trips differs.
 * fwd/bwd: [n_props]. */
ICP_API int icp_chain_eval_step(icp_evaluator *e, int32_t n_props, icp_proposal *const *props, const double *theta_cur,
                                const double *theta_prop, double *log_value_prop, double *fwd, double *bwd);

/* One call = propose (if generator >= 0) + icp_chain_eval_step, i.e. ALL device work of one Metropolis–Hastings step
 *  in one submission of five merged launches with a single synchronisation.
 *   generator >= 0 : theta_prop (out) = props[generator].propose(theta_cur) with the caller's standard normals z[r]
 *                    (NonRigidIcpProposal.scala:53-68);
 *   generator <  0 : theta_prop (in)  = a sample generated on the host (random-walk / pose proposals,
 *                    RandomShapeUpdateProposal.scala:31-35, PoseProposals.scala:31-90); z is ignored.
 * Then, as icp_chain_eval_step: log_value_prop = likelihood of theta_prop; fwd[i] / bwd[i] = logT(cur -> prop) /
 * logT(prop -> cur) of props[i].  Values are identical to the per-method entry points (same device code, same caches);
 * configurations the merged launches do not cover are routed through the per-stage kernels transparently. */
ICP_API int icp_chain_step(icp_evaluator *e, int32_t n_props, icp_proposal *const *props, int32_t generator,
                           const double *theta_cur, const double *z, double *theta_prop, double *log_value_prop, double *fwd,
                           double *bwd);

/* Optional companion of icp_chain_step: issue the first launches (proposal, instance, searches, correspondences) of the
 * step  theta_cur --generator, z--> proposal  (generator < 0: z_or_theta_prop is the proposed state itself) ahead of the
 * call that asks for it.  Meant to be called from the idle hook (below) with the NEXT step's arguments under the
 * assumption that the step in flight is rejected: an icp_chain_step with exactly these arguments then finds its first
 * half already on the device; any other call drops it.  Never changes results.  Does nothing when the posteriors of
 * theta_cur are not on record or the configuration is not covered by the merged launches.  n_props == 0 drops a
 * pending half step (a caller that stops stepping for a while should: the speculative work attached to it would
 * otherwise wait for its time-out). */
ICP_API int icp_chain_step_prelaunch(icp_evaluator *e, int32_t n_props, icp_proposal *const *props, int32_t generator,
                                     const double *theta_cur, const double *z_or_theta_prop);

/* The same with the step AFTER the next one beside it (the twin pass): while the chain stays where it is — two steps out of three
 * are rejected — its next two proposals both start from theta_cur, so both go through ONE set of launches as two lanes
 * (generator2 / z_or_theta_prop2: the second step's; NULL: icp_chain_step_prelaunch).  The icp_chain_step that asks for the first
 * step finishes both lanes in one launch and returns the first one's results; if its proposal is rejected, the call for the second
 * step finds that step's results in pinned memory and launches nothing; any other call drops the second lane.  Results are those
 * of one step at a time, bit for bit (the same device code per lane; the decompositions keep their order).  One lane is issued
 * where two are not possible: a second step the merged launches do not cover, ranks above 64, posteriors with 32 or more split-K
 * partials, ICP_NO_TWIN=1 in the environment.  *lanes_issued (optional): 0, 1 or 2 — a caller keeps ONE such front ahead of
 * the step being finished and uses the count to know which step the next front starts at. */
ICP_API int icp_chain_step_prelaunch2(icp_evaluator *e, int32_t n_props, icp_proposal *const *props, int32_t generator,
                                      const double *theta_cur, const double *z_or_theta_prop, int32_t generator2,
                                      const double *z_or_theta_prop2, int32_t *lanes_issued);
/* out: twin passes issued, second-lane results used, second-lane results dropped (icp_chain_step_prelaunch2) */
ICP_API int icp_ctx_twin_stats(icp_ctx *ctx, int64_t out[3]);
/* Diagnostic: the searches' hints as they stand on the device — the last winning target triangle of model ids 0..n_surface-1 (-1: none
 * yet), and, for a TargetSampling proposal of the context, the last nearest model vertex of its first n_vertex target points (prop may be
 * NULL with n_vertex == 0).  Waits for the device. */
ICP_API int icp_ctx_search_hints(icp_ctx *ctx, icp_proposal *prop, int32_t n_surface, int32_t *surface_out, int32_t n_vertex,
                                 int32_t *vertex_out);
/* The speculative decompositions of a twin pass's second lane go out with the first lane's, in one launch (ranks <= 64, the eigen
 * sampler; ICP_TWIN_LATE_EIGEN=1 in the environment — any value but empty or 0 —: at the second lane's own call, as before).  out: second-lane decompositions
 * started early, kept (the second lane's proposal was accepted), cancelled because the first lane's was accepted, started cold. */
ICP_API int icp_ctx_twin_eigen_stats(icp_ctx *ctx, int64_t out[4]);

/* B chains per launch (SURVEY.md §8b "*_batched variants", §8e "within a GPU, batch B chains per launch"; the
 * reference runs its chains from a ForkJoin pool, apps/femur/RunMHRandomInitComparison.scala:66): icp_chain_step for
 * n_chains independent chains in ONE sequence of five launches (chain = second grid dimension), the decompositions of
 * the chains that moved beside it.  Chain b = evaluators[b] with props[b*n_props .. b*n_props + n_props), generator[b],
 * theta_cur[b], z[b] (may be NULL where generator[b] < 0), theta_prop[b] (in or out as in icp_chain_step);
 * log_value_prop[b], fwd/bwd[b*n_props + i] and status[b] (ICP_OK / ICP_ERR_EMPTY / error of that chain) are written
 * per chain.  Every chain needs a context of its own (contexts hold the per-chain scratch; model and target are simply
 * given to each); chains on another device or of another rank than chain 0, a second chain on one context, and
 * configurations the merged launches do not cover take icp_chain_step one after the other.  Values are
 * bit-identical to icp_chain_step chain by chain.  Returns ICP_OK or the first failing chain's code.  Calls from
 * several threads must use disjoint sets of contexts. */
ICP_API int icp_chain_step_batched(int32_t n_chains, icp_evaluator *const *evaluators, int32_t n_props,
                                   icp_proposal *const *props, const int32_t *generator, const double *const *theta_cur,
                                   const double *const *z, double *const *theta_prop, double *log_value_prop, double *fwd,
                                   double *bwd, int32_t *status);

/* The same in two halves, for a caller that keeps two batches in flight (the decompositions of one run beside the
 * launches of the other; the C++ harness does): _issue returns when the batch's work is on the device, _collect waits for
 * it and writes the outputs named at _issue.  Everything passed to _issue by pointer (states, z, outputs) must stay valid
 * until _collect; the pointer ARRAYS themselves are copied.  A ticket is consumed by _collect or by _abandon (either may
 * come from any thread; no lock is held in between); until then every other entry point on a member context fails with
 * ICP_ERR_BUSY.  _abandon waits for the batch's launches and drops the step (nothing of it is recorded).  launch_ctx (may be NULL: the
 * first chain's context) names the context whose stream carries the launches: two batches given the SAME launch_ctx run
 * their launches one behind the other while the decompositions of the second run beside the launches of the first — at
 * most ICP_MAX_BATCHES_IN_FLIGHT tickets per launch_ctx at a time (one more: ICP_ERR_BUSY, nothing issued), collected in the
 * order they were issued. */
#define ICP_MAX_BATCHES_IN_FLIGHT 8
typedef struct icp_step_ticket icp_step_ticket;
ICP_API int icp_chain_step_batched_issue(int32_t n_chains, icp_evaluator *const *evaluators, int32_t n_props,
                                         icp_proposal *const *props, const int32_t *generator,
                                         const double *const *theta_cur, const double *const *z, double *const *theta_prop,
                                         double *log_value_prop, double *fwd, double *bwd, int32_t *status,
                                         icp_ctx *launch_ctx, icp_step_ticket **ticket);
ICP_API int icp_chain_step_batched_collect(icp_step_ticket *ticket);
ICP_API int icp_chain_step_batched_abandon(icp_step_ticket *ticket);

/* ---------------------------------------------------------------- posterior shape models from given correspondences, many in one call
 * Scalismo's model.posterior(correspondences, noise) and its discretisation as a model (api/other/IcpBasedSurfaceFitting.scala:81 with
 * isotropic noise, NonRigidIcpProposal.scala:152 with a 3 x 3 covariance per point, NonRigidIcpProposal.scala:77 for the model), for
 * correspondences the CALLER hands in: landmark pairs, a dense correspondence of an earlier fit.  SURVEY App. A.4, as the chain's own
 * posterior implements it:  M = I + sum Q_i^T Sigma_i^-1 Q_i,  b = sum Q_i^T Sigma_i^-1 (y_i - xbar_i - mu_i),  alpha = M^-1 b,
 * D M^-1 D = V S V^T  (Q = Phi D the scaled basis, D = diag(sqrt(variance))).  V has the canonical signs and the ordering of
 * icp_posterior_view.V for the same M.
 * Per item b (all contexts on ONE device; they may repeat, and they may differ in model and rank):
 *   ctxs[b]; n_obs[b] >= 1; vertex_ids[b] [n_obs]: model vertices in [0, N), repeats allowed (as Scalismo's regression allows them);
 *   points[b] [3 * n_obs]: the observed positions in MODEL space (the displacement is y_i - xbar_id - mu_id; take a pose off first);
 *   the noise in exactly one of two forms: sigma2[b] -> ONE finite positive double (isotropic, sigma2 * I), or covariances[b]
 *   [9 * n_obs]: a symmetric positive-definite 3 x 3 per observation, row-major (its symmetric part is used), inverted in closed form
 *   in plain f64.  `sigma2` and `covariances` may each be NULL as a whole where no item uses that form.
 * Outputs (each array may be NULL as a whole, and each entry of it may be NULL):
 *   alpha_out[b] [r];  mean_out[b] [3N] = mu + Q alpha (the posterior model's mean_deformation);  basis_out[b] [3N * r] = Phi V,
 *   row-major and unscaled like icp_model_desc.basis;  variance_out[b] [r] = S, descending;  point_variance_out[b] [N]: entry i =
 *   sum_d sum_j S_j (Phi V)[3i+d][j]^2, the trace of vertex i's 3 x 3 block of Q M^-1 Q^T;  status[b].
 * (ref_points, triangles, mean_out[b], basis_out[b], variance_out[b]) with the model's own reference and triangles IS a valid
 * icp_model_desc: icp_ctx_create accepts it, and a context made from it registers with the conditioned model.
 * One submission and one synchronisation per call: the regression sums of a group of items are ONE launch, their factorisations and
 * decompositions run side by side rank by rank (the chain's own many-problem kernels), and Phi [V | D alpha] - the mean is the extra
 * column - is a gfx950 kernel on the f64 matrix cores (v_mfma_f64_16x16x4_f64); point_variance is a pass over the rows that kernel has
 * just written, in a fixed order, without floating-point atomics.  (Only an item whose spectrum the side-by-side decomposition cannot
 * separate - equal eigenvalues - is decomposed again on its own behind a second synchronisation, as the chain does.)
 * Fixed working memory, whatever n_items and N:
 *   - ONE chunk buffer of ICP_POSTERIOR_MODELS_CHUNK_BYTES through which every output row streams back (a face-sized basis_out is
 *     137 MB; no item's basis is resident as a whole beyond this buffer);
 *   - r-space scratch for at most ICP_POSTERIOR_MODELS_GROUP items at a time, each at most ICP_POSTERIOR_MODELS_SLOT_BYTES(r, s) with
 *     r the largest rank of the call and s = min(64, ceil(largest n_obs / 8)) the split count of its regression;
 *   - the call's inputs (n_obs * (4 + 24 + 48) bytes per item) and 16 * r + 16 bytes of results per item.
 * An item's bits depend neither on the other items of the call, nor on their order, nor on how its rows fall into the chunk buffer.
 * Ranks: every rank the resident decompositions serve, i.e. r <= 256.  An item of a larger rank gets status[b] = ICP_ERR_INVALID_ARG
 * and nothing is written for it; the other items are computed.
 * Whole-call errors - nothing has run, nothing is written, status included: ICP_ERR_INVALID_ARG (a null entry, n_items outside
 * [1, 65535], n_obs < 1, an id out of range, both noise forms given for an item or neither, a non-finite input, sigma2 <= 0, contexts
 * on two devices); ICP_ERR_BUSY (a context belongs to a batch in flight).  Otherwise status[b] = ICP_OK, or ICP_ERR_NOT_FINITE for an
 * item with a covariance that is not positive definite or whose M failed to factor: that item's outputs are NaN, the other items are
 * untouched by it; the return value is ICP_OK or the first failing item's status. */
#define ICP_POSTERIOR_MODELS_CHUNK_BYTES (32u << 20)
#define ICP_POSTERIOR_MODELS_GROUP 16
#define ICP_POSTERIOR_MODELS_SLOT_BYTES(r, s) (8ull * ((unsigned long long)(s) * ((r) + 1) * ((r) + 1) + 50ull * ((r) + 17) * ((r) + 17) + 4096))
ICP_API int icp_posterior_models_many(int32_t n_items, icp_ctx *const *ctxs, const int32_t *n_obs, const int32_t *const *vertex_ids,
                                      const double *const *points, const double *const *sigma2, const double *const *covariances,
                                      double *const *alpha_out, double *const *mean_out, double *const *basis_out,
                                      double *const *variance_out, double *const *point_variance_out, int32_t *status);

/* ---------------------------------------------------------------- Gaussian-process shape models from analytic kernels, many in one call
 * What apps/femur/CreateGPModel.scala and apps/bfm/CreateGPModel.scala do before anything is registered: a low-rank model of a
 * matrix-valued kernel on a reference mesh's own points (the femur kernel through this entry point; the face kernel of apps/bfm, whose
 * terms are B-splines with weights and a mirror, through icp_gp_models_general_many below).  The approximation is Scalismo's pivoted Cholesky factorisation
 * (approximateGPCholesky) followed by the eigen-decomposition of an m x m Gram matrix; deterministic, no sampler.
 *   k(x, y) = sum_t scale_t * exp(-|x - y|^2 / sigma_t^2) * A_t      (Scalismo's GaussianKernel(sigma): no factor 1/2)
 * with 1 .. ICP_GP_MODELS_MAX_TERMS terms per item; A_t (row-major 3 x 3) exactly symmetric, positive semi-definite (checked on the host
 * in closed form) and not zero, scale_t > 0, sigma_t > 0, all finite.  CreateGPModel.scala:68-78 is 10 B G(90) + 5 I G(40) + 3 I G(10).
 * K is the 3N x 3N kernel matrix on the points (row 3 * vertex + coordinate), d its diagonal, summed over the terms in order.
 *   step j = 0, 1, ...: p = the row of the largest d (ties: the lowest row).  Stop BEFORE the step when j = n_pivots, when
 *     max d <= n_pivots * 2^-52 * (max d at the start), or when sum d <= rel_tolerance * trace(K).  Otherwise
 *     col = K[:, p] - L[:, :j] L[p, :j]^T (products summed in column order),  L[:, j] = col / sqrt(d[p]),  d -= L[:, j]^2 (not clamped).
 *   then, with m_eff columns: (theta_j, u_j) the eigenpairs of L L^T (through the m_eff x m_eff matrix L^T L, decomposed by the
 *     resident routes of the chain - ranks up to 64 Jacobi, up to 256 tridiagonal - and one step of iterative refinement of their
 *     eigenvectors, which the chain needs to 1e-11 only and a basis to rounding), descending;
 *     variance_j = theta_j / N,  basis column j = sqrt(N) u_j  (squared norm N, as Scalismo's discretised models have them).
 * Per item b: n_points[b] = N >= 1; points[b] [3N] finite; n_terms[b], terms[b]; 1 <= rank[b] <= n_pivots[b] <= min(256, 3N);
 * 0 <= rel_tolerance[b] < 1 (rel_tolerance == NULL: 0 for every item).  The effective rank is min(rank, m_eff).
 * Outputs (each array may be NULL as a whole, and each entry of it may be NULL):
 *   variance_out[b] [rank] descending, 0 behind the effective rank;  basis_out[b] [3N * rank] row-major like icp_model_desc.basis, zero
 *   columns behind the effective rank;  pivots_out[b] [n_pivots] rows 3 * vertex + coordinate in the order chosen, -1 behind m_eff;
 *   residual_out[b] [3N] = d when the loop stopped;  info_out[b] [4] = m_eff, effective rank, trace(K) / N, sum of variance_out[b].
 * With effective rank == rank, (points, triangles, NULL, basis_out[b], variance_out[b]) IS a valid icp_model_desc (mean deformation 0).
 * The call takes no context: `device` as icp_ctx_create takes it; streams and buffers come from the library's pools.  One launch per
 * pivot step carries every item of the call; ONE synchronisation behind the loop (the effective pivot counts), then one per round of
 * output rows: L^T L and L (W Theta^-1/2 sqrt N) run on the f64 matrix cores (v_mfma_f64_16x16x4_f64), the rows of the bases pass through
 * ONE chunk buffer of ICP_GP_MODELS_CHUNK_BYTES.  Device memory: 8 * 3N * (n_pivots + 2) bytes per item for L, d and the points, all items
 * of the call at once.  No floating-point atomics; every sum of an item is a function of the item alone: its bits depend neither on
 * the other items of the call, nor on their order, nor on how its rows fall into the chunk buffer.
 * Whole-call errors (nothing has run, nothing is written): ICP_ERR_INVALID_ARG for n_items outside [1, 65535] or a null required
 * argument; ICP_ERR_DEVICE.  An item outside the limits above gets status[b] = ICP_ERR_INVALID_ARG - decided for every item before
 * the device is touched - and nothing is written for it; the other items are computed.  status[b] = ICP_ERR_NOT_FINITE (outputs NaN)
 * if the decomposition of an item did not converge.  The return value is ICP_OK or the first failing item's status. */
typedef struct {
  double scale;
  double sigma;
  double A[9];
} icp_kernel_term;
#define ICP_GP_MODELS_MAX_TERMS 8
#define ICP_GP_MODELS_MAX_PIVOTS 256
#define ICP_GP_MODELS_CHUNK_BYTES (32u << 20)
ICP_API int icp_gp_models_many(int32_t n_items, int device, const int32_t *n_points, const double *const *points,
                               const int32_t *n_terms, const icp_kernel_term *const *terms, const int32_t *n_pivots,
                               const int32_t *rank, const double *rel_tolerance, double *const *variance_out,
                               double *const *basis_out, int32_t *const *pivots_out, double *const *residual_out,
                               double *const *info_out, int32_t *status);

/* ---------------------------------------------------------------- general kernel terms: B-spline, weighted and mirrored
 * What apps/bfm/CreateGPModel.scala needs of icp_gp_models_many (FaceKernel.scala:26-108, FaceMask.scala:41-54): the project's own
 * restatement; parity with Scalismo is unpinned.  For x, y on the mesh's own points, v(x) the vertex of x, term t, components c, c':
 *   k_t(x, y)[c][c'] = scale_t * w_t(v(x)) * w_t(v(y)) * A_t[c][c'] * ( b_t(x, y) + gain_t * s_c * b_t(x, ym) )
 * b_t, the scalar base kernel:
 *   ICP_KERNEL_GAUSSIAN  exp(-|x - y|^2 / sigma^2), the squared distance as (dx*dx + dy*dy) + dz*dz: icp_gp_models_many's expression;
 *   ICP_KERNEL_BSPLINE3  with c = 2^level:  b(x, y) = S(x0 c, y0 c) * S(x1 c, y1 c) * S(x2 c, y2 c),
 *     S(u, v) = sum over k = ceil(max(u, v) - 2) .. floor(min(u, v) + 2), ascending, of beta(u - k) * beta(v - k)  (at most five k; an
 *     empty range gives 0),  beta(t), a = |t|:  (2/3 - a*a) + ((0.5*a)*a)*a for a < 1;  ((1/6*(2 - a))*(2 - a))*(2 - a) for 1 <= a < 2;
 *     0 otherwise.  (Scalismo's BSplineKernel(order 3, scale level); its triple loop agrees with the product of the three sums to
 *     rounding.)  Lattice indices are exact doubles: the host requires |x_d| * 2^level < 2^31 for every coordinate of the item.
 * w_t: per-vertex weights [N], >= 0, finite, at least one positive; NULL: 1.
 * Mirror: ym = y with coordinate mirror_axis negated; gain_t = mirror_gain in [0, 1]; s_c = -1 for c == mirror_axis, else +1.  With
 *   mirror_gain > 0, A_t must not couple the mirror axis to the others (A[a][b] == 0 for b != a).  DEVIATION from the reference, which
 *   evaluates the weight of the mirrored argument AT the mirrored point (an unsymmetric kernel matrix unless the mask is mirror-
 *   symmetric): here the weight of ym is the weight of y - exact for a mirror-symmetric mask, and K is symmetric positive semi-definite
 *   for every 0 <= mirror_gain <= 1.  FaceKernel = k(x, y) + 0.7 * Im * k(x, ym): five ICP_KERNEL_BSPLINE3 terms (level, scale) =
 *   (-6, 128), (-5, 64), (-4, 32), (-3, 10), (-2, 4), A = I, the level's weights, mirror_gain 0.7, mirror_axis 0.
 * A term's value is ((scale * (w(v(x)) * w(v(y)))) * (b(x, y) + (gain * s_c) * b(x, ym))) * A[c][c'], the terms summed in order; the
 * diagonal d[3v + c] is the same expression at y = x (no longer constant over the mesh).  A term with kind 0, no weights and gain 0
 * (a plain term) has icp_gp_models_many's bits, and an item whose every term is plain runs icp_gp_models_many's code: the two entry
 * points reach one implementation.  The pivot rule, the stopping rules, the decomposition, the outputs and the limits are
 * icp_gp_models_many's.  Per item, checked before the device is touched (status[b] = ICP_ERR_INVALID_ARG, nothing written): all of
 * icp_gp_models_many's checks; struct_size; kind; for the B-spline -32 <= level <= 32 and the lattice range; 0 <= mirror_gain <= 1;
 * mirror_axis in {0, 1, 2}; the decoupling of A when mirror_gain > 0; the weights.
 * Decided on the device: with mirror_gain = 1, or where the weights vanish, rows of K are zero and trace(K) may be 0: an item whose
 * pivot loop leaves NO column gets status[b] = ICP_ERR_NOT_FINITE, NaN in variance_out, basis_out and residual_out, pivots -1 and
 * info_out = {0, 0, 0, 0}; the other items complete (icp_gp_models_many cannot meet the case: its diagonal is positive).
 *
 * icp_region_weights_many: FaceMask.computeSmoothedRegions, many in one call.  Item b: weights_out[b][i] = exp(-(d2 / (stddev *
 * stddev))), d2 the smallest (dx*dx + dy*dy) + dz*dz from point i of points[b] [3 * n_points] to the n_region[b] >= 1 points of
 * region_points[b]; 1.0 exactly at a region point.  stddev[b] > 0 (40 in the reference); everything finite.  One launch for the
 * whole call (a thread per point, the region tiled through LDS, f64); an item's bits depend on the item alone.  Statuses as above. */
#define ICP_KERNEL_GAUSSIAN 0
#define ICP_KERNEL_BSPLINE3 1
typedef struct {
  int32_t struct_size;      /* sizeof(icp_kernel_term_general) */
  int32_t kind;             /* ICP_KERNEL_GAUSSIAN 0, ICP_KERNEL_BSPLINE3 1 */
  double scale;             /* > 0, finite */
  double sigma;             /* Gaussian: > 0, finite; else ignored */
  int32_t level;            /* B-spline: 2^level cells per unit, [-32, 32]; else ignored */
  int32_t mirror_axis;      /* 0, 1 or 2 */
  double mirror_gain;       /* [0, 1] */
  double A[9];
  const double *weights;    /* [N] or NULL */
} icp_kernel_term_general;
ICP_API int icp_gp_models_general_many(int32_t n_items, int device, const int32_t *n_points, const double *const *points,
                                       const int32_t *n_terms, const icp_kernel_term_general *const *terms, const int32_t *n_pivots,
                                       const int32_t *rank, const double *rel_tolerance, double *const *variance_out,
                                       double *const *basis_out, int32_t *const *pivots_out, double *const *residual_out,
                                       double *const *info_out, int32_t *status);
ICP_API int icp_region_weights_many(int32_t n_items, int device, const int32_t *n_points, const double *const *points,
                                    const int32_t *n_region, const double *const *region_points, const double *stddev,
                                    double *const *weights_out, int32_t *status);

/* ---- Gaussian-process shape models by the Nystrom approximation on sample points, many in one call.
 * What apps/femur/CreateGPModel.scala:93 and apps/bfm/CreateGPModel.scala:56 call: LowRankGaussianProcess.approximateGPNystrom(gp,
 * sampler, numBasisFunctions).  The formulas are this project's restatement [SCALISMO-UNVERIFIED].  Item b: mesh points X
 * (points[b], [3 * n_points]), sample points S given by the caller (samples[b], [3 * n_samples], n = n_samples; icp_surface_samples_many
 * draws them as UniformMeshSampler3D does), the kernel of terms[b] (n_terms[b] general terms: icp_gp_models_general_many's, a plain term
 * running icp_gp_models_many's expression), rank[b] = k basis functions, min_variance[b] (NULL: 1e-8 for every item):
 *   1. K = k(S, S), R x R with R = 3n, the terms summed in order; both triangles come from one evaluation
 *   2. K = U L U^T, eigenvalues descending; all R are handed out (sample_eigenvalues_out[b], [R])
 *   3. k_eff = the number of i < k with lambda_i / n >= min_variance
 *   4. variance_out[b][i] = lambda_i / n for every i < k
 *   5. basis column i = k(X, S) u_i sqrt(n) / lambda_i for i < k_eff: basis_out[b] is [3 * n_points][k] row by row, the columns from
 *      k_eff on are zero
 *   6. the mean deformation is zero
 * sample_eigenvectors_out[b] [R][k]: the device's own u_i, row by row.  info_out[b] [4] = {k_eff, sweeps used, trace K, the
 * off-diagonal mass (sum of squares) the last sweep met in front of its rotations}.  Every output pointer, and every array of them,
 * may be NULL.
 * A term with weights (its `weights` are the region weights at the MESH points, [n_points]) needs the same region weights at the
 * sample points: sample_weights[b][t], [n_samples], finite, >= 0, at least one positive.  sample_weights, or sample_weights[b], may be
 * NULL when no term of the call, or of item b, has weights.
 * Limits, checked for every item before the device is touched (status[b] = ICP_ERR_INVALID_ARG for that item alone, nothing of it
 * written, its neighbours computed): 1 <= rank <= min(ICP_NYSTROM_MAX_RANK, R); R <= ICP_NYSTROM_MAX_ROWS; min_variance >= 0; finite
 * points and samples; the terms' checks of icp_gp_models_general_many, the lattice range over points and samples.
 * The eigenproblem is a two-sided block Jacobi iteration on the device (blocks of 32 columns, R padded with zero rows to an even
 * number of blocks; the pairs of a round side by side, every pair's rotation the one nearest the identity; row and column panels on
 * the f64 matrix cores).  An item stops behind the first sweep whose off-diagonal mass is <= (R 2^-52 |K|_F)^2; the host reads one
 * word per sweep.  After ICP_NYSTROM_MAX_SWEEPS sweeps an item gets ICP_ERR_NOT_CONVERGED, and its outputs are written from the
 * iteration as it stands.  k(X, S) is never stored: the basis product evaluates it tile by tile and streams its rows through ONE chunk
 * buffer of ICP_GP_MODELS_CHUNK_BYTES.  An item's bits depend on the item alone.  Returns the first bad item's code, or ICP_OK. */
#define ICP_NYSTROM_MAX_ROWS 2400
#define ICP_NYSTROM_MAX_RANK 256
#define ICP_NYSTROM_MAX_SWEEPS 40
ICP_API int icp_nystrom_models_many(int32_t n_items, int device, const int32_t *n_points, const double *const *points,
                                    const int32_t *n_samples, const double *const *samples, const int32_t *n_terms,
                                    const icp_kernel_term_general *const *terms, const double *const *const *sample_weights,
                                    const int32_t *rank, const double *min_variance, double *const *variance_out,
                                    double *const *basis_out, double *const *sample_eigenvalues_out,
                                    double *const *sample_eigenvectors_out, double *const *info_out, int32_t *status);

/* ---- PCA shape models from registered meshes, with generalised Procrustes alignment, many in one call.
 * What a registration study is made for: meshes in correspondence (all in the model's vertex order) become a statistical shape model,
 * Scalismo's DataCollection.gpa followed by StatisticalMeshModel.createUsingPCA.  The alignment rules are this project's restatement
 * [SCALISMO-UNVERIFIED].  The meshes live in a pool that is uploaded once: pool mesh k is pool[k] [pool_points[k]][3]; item b uses
 * pool[mesh_ids[b][0 .. n_meshes[b]-1]], all of one N, copied into working copies of its own.  A leave-one-out call on n meshes uploads n.
 *   alignment   at most gpa_iterations[b] rounds (0: the meshes are taken as given).  The first mean shape is the mean of the copies,
 *               summed in the order j = 0, 1, ....  A round aligns every mesh to the SAME current mean shape by the least-squares rigid
 *               transform over all N vertex pairs (proper rotation, no scale), then the aligned meshes' mean is the new mean shape.
 *               The transform in two passes: the centroids c_x, c_y first, then S = sum (x - c_x)(y - c_y)^T of the centred points
 *               (not sum x y^T - N c_x c_y^T, which cancels at coordinates of 200 mm); the rotation is Horn's unit quaternion, the
 *               eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix of S, by cyclic Jacobi sweeps in f64;
 *               x <- R (x - c_x) + c_y.  An item stops behind the round in which sqrt(mean_i |new mean_i - mean_i|^2) < halt_distance[b]:
 *               the RMS displacement of the mean shape, NOT Scalismo's procrustesDistance, which aligns the two means once more.
 *               transforms_out[b] [n][12]: every mesh's composite transform (R <- R_k R, t <- R_k t + t_k with t_k = c_y - R_k c_x,
 *               accumulated on the device), rotation by rows, then the translation: aligned = R x + t up to rounding.
 *   centring    mean_out[b] [3N] is the final mean shape (the model's mean deformation is mean_out - reference, a subtraction the caller
 *               makes; without a reference the mean shape is the reference mesh and the mean deformation 0); column j of the data
 *               matrix L is (x_j - mean) / sqrt(n - 1).
 *   model       the covariance is L L^T over ALL n columns; its eigenpairs through the n x n matrix G = L^T L exactly as
 *               icp_gp_models_many makes them (the same launches): variance_j = theta_j / N, basis column j = sqrt(N) L w_j / sqrt(theta_j).
 *               G is singular by construction (the centred columns sum to rounding): rank[b] <= n - 1, and the effective rank is
 *               min(rank, #{j : theta_j > tau}), tau = max(3N n 2^-52 trace(G), tau_0): the first is the worst-case rounding of the
 *               Gram sum (3N products per entry, n x n entries in spectral norm); tau_0 = 2^-80 sum_j |x_j|^2 / (n - 1) is a direction
 *               in which the aligned meshes differ by less than 2^-40 of their size, which is what up to 32 rounds of rotating the
 *               copies in f64 leave of rounding.  Decided on the device.  Columns and variances behind the effective rank are zero.
 *               An item that keeps no component (all meshes equal) fails alone: status[b] = ICP_ERR_NOT_FINITE, every output NaN.
 *   info_out[b] [8] = meshes, effective rank, trace(G) / N (the total variance), sum of variance_out[b], rounds run, the last round's
 *               RMS displacement (0 without a round), 0, 0.
 * reference: NULL, or per item NULL or [3N]; checked for finiteness and otherwise the caller's.  Every output array may be NULL as a
 * whole, and so may each entry.  Limits, checked for every item before the device is touched (status[b] = ICP_ERR_INVALID_ARG, nothing
 * written for it, the other items computed): 2 <= n_meshes <= 256; N >= 1, 3N <= INT32_MAX; 1 <= rank <= n_meshes - 1;
 * 0 <= gpa_iterations <= ICP_PCA_MODELS_MAX_ROUNDS; halt_distance >= 0 and finite; ids in [0, n_pool); one N per item; finite points.
 * Whole-call errors (nothing has run): n_items outside [1, 65535], n_pool < 1, a null required argument; ICP_ERR_DEVICE.
 * The call takes no context.  1 + 4 * (the call's largest gpa_iterations) + 1 launches carry every item and every mesh, without a
 * synchronisation between them (a stopped item returns from every later launch); ONE synchronisation; then icp_gp_models_many's
 * m-space half, one synchronisation per round of output rows.  Device memory: the pool once, and 8 * 3N * (n + 1) bytes per item and a
 * few partials, all items at once.  No floating-point atomics; an item's bits depend neither on the other items, nor on their order,
 * nor on how its rows fall into the chunk buffer.  Not covered: more than 256 meshes per item; parity of the halt rule with Scalismo;
 * degenerate (collinear) vertex sets, whose rotation is not unique. */
#define ICP_PCA_MODELS_MAX_ROUNDS 32
ICP_API int icp_pca_models_many(int32_t n_items, int device, int32_t n_pool, const int32_t *pool_points, const double *const *pool,
                                const int32_t *n_meshes, const int32_t *const *mesh_ids, const double *const *reference,
                                const int32_t *rank, const int32_t *gpa_iterations, const double *halt_distance,
                                double *const *variance_out, double *const *basis_out, double *const *mean_out,
                                double *const *transforms_out, double *const *info_out, int32_t *status);

/* ---- aligned and partial targets from raw scans, many in one call.
 * The step both studies of the reference start with (apps/femur/AlignShapes.scala:30-55, apps/bfm/AlignShapes.scala:33-101): a raw
 * scan is scaled, landmark-aligned, cut around landmarks and by an id list, and what is left is compacted.  Kabsch on a handful of
 * landmark pairs stays with the caller; the device gets the transform.  Per item b, all floating point f64 with every operation
 * rounded separately, all ids int32:
 *   transform   A(x): q = s*x per coordinate, u = q - c, y_i = ((R_i0*u_0 + R_i1*u_1) + R_i2*u_2) + o_i with o = c + t rounded once on
 *               the host: Scalismo's translation o rotation-about-c behind Scaling(s) (AlignmentTransforms.scala:25-30,
 *               apps/bfm/AlignShapes.scala:66,77-83).  aligned_out[b] [3 * M] = A(points[b]), landmarks_out[b] [3 * L] = A(landmarks[b]):
 *               vertices and landmarks go through one device function, so a cut's centre has the bits the caller gets back.
 *   cut j       (findNClosestPoints, :90) z = landmarks_out[cut_landmark[b][j]], d2(v) = (dx*dx + dy*dy) + dz*dz with dx = aligned[v].x -
 *               z.x ...; the cut set is the min(cut_count[b][j], M) vertices smallest in (d2, v), ordered lexicographically: EQUAL
 *               DISTANCES GO TO THE LOWEST IDS (a rule of this library; the reference's KD-tree leaves it open).
 *   flags       cut_flags_out[b][v] [M] has bit j if v is in cut set j and bit 7 if v occurs in mask_ids[b] (duplicates allowed, ids
 *               >= M match nothing); a vertex is dropped iff its flags are not zero.
 *   compaction  (operations.maskPoints(...).transformedMesh, :92 [SCALISMO-UNVERIFIED]) a triangle is kept iff none of its vertices
 *               is dropped, kept triangles stay in their order; a vertex is kept iff a kept triangle uses it, kept vertices stay in
 *               ascending old id order — a vertex no triangle references leaves the partial mesh even when it is not cut.
 *               partial_points_out[b] (caller: [3 * M]), partial_triangles_out[b] (caller: [3 * T], renumbered), kept_ids_out[b]
 *               (caller: [M], kept_ids[new] = old): the rows counts_out[2b] = n_kept / counts_out[2b + 1] = t_kept are written, the
 *               rows behind them are left untouched.  An empty result (everything cut, T = 0) is ICP_OK with counts (0, 0).
 * Any output array, or any entry of one, may be NULL, and so may counts_out; status may not.  Limits, checked for every item before
 * the device is touched (status[b] = ICP_ERR_INVALID_ARG, nothing written for that item): 1 <= M <= 2^26, 0 <= T <= 2^26, triangle
 * ids in [0, M), struct_size, pre_scale > 0, every double finite and |s*x|, |c|, |t|, |R_ij| <= 2^400 (no result is NaN),
 * 0 <= n_cuts <= ICP_SCAN_MAX_CUTS, 0 <= cut_landmark < L, cut_count >= 0, mask ids >= 0; n_items in [1, 65535].  The items go
 * through the device in rounds of at most ICP_SCAN_PREP_ROUND_BYTES (an item above that has a round of its own), one
 * synchronisation per round; an item's bits depend on the item alone. */
#define ICP_SCAN_MAX_CUTS 7
#define ICP_SCAN_PREP_ROUND_BYTES (64u << 20)
typedef struct {
  uint64_t struct_size;   /* sizeof(icp_scan_transform) */
  double pre_scale;       /* s > 0 */
  double rotation[9];     /* R, row-major */
  double centre[3];       /* c */
  double translation[3];  /* t */
} icp_scan_transform;
ICP_API int icp_scans_prepare_many(int32_t n_items, int device, const int32_t *n_points, const double *const *points,
                                   const int32_t *n_triangles, const int32_t *const *triangles, const icp_scan_transform *transforms,
                                   const int32_t *n_landmarks, const double *const *landmarks, const int32_t *n_cuts,
                                   const int32_t *const *cut_landmark, const int32_t *const *cut_count, const int32_t *n_mask_ids,
                                   const int32_t *const *mask_ids, double *const *aligned_out, double *const *landmarks_out,
                                   uint8_t *const *cut_flags_out, double *const *partial_points_out,
                                   int32_t *const *partial_triangles_out, int32_t *const *kept_ids_out,
                                   int32_t *counts_out /* [n_items * 2] */, int32_t *status);

/* ---- mesh decimation to a vertex subset, many in one call.
 * The step in front of every hot-path object of the reference (NonRigidIcpProposal.scala:45-46, the evaluators' constructors,
 * BfmFittingComplete.scala:45-47, apps/bfm/CreateGPModel.scala:43).  VTK's quadric decimation is a sequential priority queue and is NOT
 * reproduced: this is a decimation of this library's own kind — farthest-point samples, their graph-distance cells, the cells' dual
 * triangles — deterministic to the bit, whose vertices are a SUBSET of the input's, so that a model is decimated by a row gather.
 * Per item b, with M = n_points[b], T = n_triangles[b], k = n_samples[b], kk = min(k, M):
 *   selection   d2(u, v) = ((dx*dx + dy*dy) + dz*dz) in f64, every operation rounded separately.  ids[0] = starts[b] (starts == NULL:
 *               0); after j samples D_j(v) = min over i < j of d2(v, ids[i]), and ids[j] is the vertex with the largest D_j: EQUAL
 *               VALUES GO TO THE LOWEST ID.  If that largest value is 0 every vertex coincides with a sample and the selection stops:
 *               k_eff = j, otherwise k_eff = kk.  cover2[j] = max over v of D_{j+1}(v), the squared covering radius after j + 1
 *               samples: finite, not increasing, 0 at the last index when the selection stopped early.  ANY PREFIX OF ids IS THE
 *               DECIMATION TO THAT SMALLER COUNT: one call at the largest count serves a whole ladder of counts.
 *   labels      a half-edge (u -> v) for every ordered pair of distinct corners of every triangle, of length (float)sqrt(d2(u, v)):
 *               the f64 square root, then one rounding to f32.  A vertex's key is the unsigned 64-bit word (bits of its f32
 *               distance) << 32 | label; sample j starts with (0, j), every other vertex with all ones.  Sweep s:
 *               key'[v] = min(key[v], min over half-edges (u -> v) with key[u] not all ones of ((f32)(dist[u] + len), label[u])),
 *               every right-hand side read from sweep s (synchronous); the iteration ends at the first sweep that changes no key of
 *               the item.  labels[v] = the low word of the final key, -1 for a vertex no sample reaches; equal distances go to the
 *               lowest label.  sweeps = the number of sweeps that changed a key.
 *   triangles   triangle t with labels (a, b, c) is a candidate iff all three are >= 0 and pairwise distinct; its canonical form is
 *               the rotation that puts the smallest label first (the orientation is kept); a candidate is kept iff no candidate of a
 *               lower index has the same canonical form.  Kept triangles stay in the order of their index; their rows are the
 *               canonical label triples, ids into `ids`.  The other orientation of a kept triple is a different triple and is kept.
 *   outputs     counts_out [3 * n_items]: (k_eff, T_out, sweeps); ids_out[b] (caller: [k]), points_out[b] ([3 * k], the samples'
 *               coordinates bit for bit), cover2_out[b] ([k]): rows 0 .. k_eff - 1; labels_out[b] ([M]); cells_out[b] (caller:
 *               [3 * T]): rows 0 .. T_out - 1.  The rows behind k_eff and T_out are left untouched.  Every sample is a vertex of the
 *               result, whether a triangle uses it or not.
 * Any output array, or any entry of one, may be NULL, but not all six arguments; status may not.  Limits, checked for every item before
 * the device is touched (status[b] = ICP_ERR_INVALID_ARG, nothing written for that item): 1 <= M <= 2^24, 0 <= T <= 2^26, triangle
 * ids in [0, M), 1 <= k <= ICP_DECIMATE_MAX_POINTS (three labels fit one 64-bit triple key), 0 <= start < M, every coordinate finite
 * with |x| <= 2^60 (no length or path sum overflows f32); n_items in [1, 65535].  The items go through the device in rounds of at most
 * ICP_DECIMATE_ROUND_BYTES (an item above that has a round of its own); an item's bits depend on the item alone.  No floating-point
 * atomics.  Not covered: lengths below 2^-126 (f32 subnormals) are untested; the result need not be a manifold (data.mesh_edge_census
 * of the Python layer counts the edges by their triangles). */
#define ICP_DECIMATE_MAX_POINTS 65535
#define ICP_DECIMATE_ROUND_BYTES (64u << 20)
ICP_API int icp_decimate_many(int32_t n_items, int device, const int32_t *n_points, const double *const *points,
                              const int32_t *n_triangles, const int32_t *const *cells, const int32_t *n_samples, const int32_t *starts,
                              int32_t *counts_out /* [n_items * 3] */, int32_t *const *ids_out, double *const *points_out,
                              double *const *cover2_out, int32_t *const *labels_out, int32_t *const *cells_out, int32_t *status);

/* ---- uniform surface samples of many meshes, with the nearest vertex of every sample, many in one call.
 * Scalismo's UniformMeshSampler3D as the reference draws from it: IcpBasedSurfaceFitting.scala:51-53 (target points, model points and
 * their nearest vertex ids), apps/femur/CreateGPModel.scala:92-93 and apps/bfm/CreateGPModel.scala:55-56 (the sample points of
 * approximateGPNystrom), apps/femur/CreateGPModel.scala:38-46 (approxTotalVariance).  The generator is this library's own, so the
 * points are not Scalismo's; the law is: a triangle in proportion to its area, a point uniform in it.  Deterministic to the bit.
 * Per item b, with M = n_points[b], T = n_triangles[b], n = n_samples[b], seed = seeds[b]; all floating point f64 with every operation
 * rounded separately:
 *   weights     triangle t with corners a, b, c: e1 = b - a, e2 = c - a, the normal (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z,
 *               e1x*e2y - e1y*e2x) - two products and one subtraction per component -, A2_t = sqrt((nx*nx + ny*ny) + nz*nz), twice
 *               the area (a value that is not finite counts as 0; within the limits below there is none).  Amax = the largest A2_t.
 *               q_t = (uint64) trunc((A2_t / Amax) * 2^32), AN INTEGER WEIGHT in [0, 2^32]; C_t = q_0 + ... + q_t in 64-bit integers,
 *               Q = C_{T-1} < 2^58.  Integers, because a floating-point prefix sum would tie an item's bits to the shape of the scan.
 *               DEVIATION from sampling by exact area: A TRIANGLE BELOW 2^-32 OF THE LARGEST IS NEVER DRAWN, and every other
 *               probability is off by at most 2^-32 relative to the largest triangle's.
 *   draws       h(seed, step, lane) = splitmix64(splitmix64(splitmix64(seed) ^ step * 0xD1342543DE82EF95) ^ lane * 0x2545F4914F6CDD1D)
 *               >> 11, a 53-bit integer (splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 *               x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31), and u(seed, step, lane) = (h + 0.5) * 2^-53: the generator of
 *               icp_mesh_metrics_many's Dice samples.  Sample k: x = (h(seed, 0, k) * Q) >> 53, the high word of the 64 x 64 bit
 *               product (h << 11) * Q, in [0, Q - 1]; its triangle is THE FIRST t WITH C_t > x (a triangle of weight 0 is never
 *               chosen); r = sqrt(u(seed, 1, k)), v = u(seed, 2, k); w0 = 1 - r, w1 = r * (1 - v), w2 = r * v;
 *               p = (w0 * a + w1 * b) + w2 * c per coordinate.
 *   nearest     vertex_ids_out[b][k] = the lexicographic minimum of (d2, id) over ALL M vertices, d2 = (dx*dx + dy*dy) + dz*dz from p:
 *               EQUAL DISTANCES GO TO THE LOWEST ID.  Not the nearest of the triangle's three corners: on a needle triangle some
 *               other vertex is nearer.  (Scalismo's findClosestPoint(p).id; its KD-tree leaves ties open.)
 *   outputs     points_out[b] [3 * n], cells_out[b] [n] (the triangle of every sample), bary_out[b] [3 * n] (w0, w1, w2),
 *               vertex_ids_out[b] [n], info_out[b] [4] = {triangles with q_t > 0, 0.5 * Amax, the surface area as
 *               (0.5 * Amax) * ((double)Q * 2^-32), 0}.  Every output array, and every entry of one, may be NULL, but not all five
 *               arguments; status may not.  The nearest-vertex launch is skipped for a round in which no item asks for ids.
 * Limits, checked for every item before the device is touched (status[b] = ICP_ERR_INVALID_ARG for that item alone, nothing of it
 * written, its neighbours computed): 1 <= M <= 2^24, 1 <= T <= 2^26, triangle ids in [0, M), 1 <= n <= 2^24, every coordinate finite
 * with |x| <= 2^60, non-null points[b] and cells[b].  Whole-call errors (nothing has run, nothing is written): n_items outside
 * [1, 65535], a null required argument, no output at all; ICP_ERR_DEVICE.
 * Decided on the device: an item whose every A2_t is 0 has nothing to draw from: status[b] = ICP_ERR_NOT_FINITE, NaN in its double
 * outputs, -1 in its int outputs, info = {0, 0, 0, 0}; the other items complete.
 * The call takes no context.  The items go through the device in rounds of at most ICP_SURFACE_SAMPLES_ROUND_BYTES (an item above
 * that has a round of its own), one upload, one copy back and one synchronisation per round; per round one grid per stage for all its
 * items: areas and tile maxima; Amax, q and tile totals; tile offsets; pick and point; nearest vertex.  No atomics.  An item's bits
 * depend neither on the other items, nor on their order, nor on the rounds, nor on which outputs are asked for.
 *
 * icp_kernel_total_variance_many: approxTotalVariance, many in one call.  Item b: the mean over its n = n_points[b] points (any points,
 * [3 * n]; the reference takes 50,000 surface samples) of the trace of k(x, x).  Per point and component c the diagonal entry is the
 * term expression of icp_gp_models_general_many at y = x, ((scale * (w(x) * w(x))) * (b(x, x) + (gain * s_c) * b(x, xm))) * A[c][c],
 * the terms summed in order; the trace is (entry 0 + entry 1) + entry 2.  A term's `weights` field is NOT read: the weights at these
 * points are point_weights[b][t] ([n], finite, >= 0, at least one positive), NULL where the term has none; point_weights, or
 * point_weights[b], may be NULL.  The sum has a shape that depends on n alone: blocks of 256 consecutive points, inside a block
 * tr[i] += tr[i + s] for s = 128, 64, ..., 1 with +0.0 for the entries past n, the block sums added in block order, the result
 * divided by n: total_variance_out[b].  Limits (status[b] = ICP_ERR_INVALID_ARG, total_variance_out[b] untouched): 1 <= n <= 2^24,
 * finite points, 1 <= n_terms <= 8, the terms' checks of icp_gp_models_general_many with the lattice range over these points, the
 * weights.  Whole-call errors as above. */
#define ICP_SURFACE_SAMPLES_ROUND_BYTES (64u << 20)
ICP_API int icp_surface_samples_many(int32_t n_items, int device, const int32_t *n_points, const double *const *points,
                                     const int32_t *n_triangles, const int32_t *const *cells, const int32_t *n_samples,
                                     const uint64_t *seeds, double *const *points_out, int32_t *const *cells_out,
                                     double *const *bary_out, int32_t *const *vertex_ids_out, double *const *info_out,
                                     int32_t *status);
ICP_API int icp_kernel_total_variance_many(int32_t n_items, int device, const int32_t *n_points, const double *const *points,
                                           const int32_t *n_terms, const icp_kernel_term_general *const *terms,
                                           const double *const *const *point_weights, double *total_variance_out, int32_t *status);

/* ---------------------------------------------------------------- the per-method entry points as ONE submission per step (round 6)
 * The drop-in contract is "Scalismo's chain, unchanged": MetropolisHastings.next (constructed at
 * api/sampling/SamplingRegistration.scala:52-58) calls  logValue(current) [memoised] → propose(current) → logValue(proposal) →
 * logTransitionRatio(current, proposal), and the MixtureProposal of api/sampling/MixedProposalDistributions.scala:48-68 turns the last
 * into logTransitionProbability(current, proposal) and (proposal, current) of EVERY ICP proposal (App. B2): with two ICP proposals six
 * device round trips per step where icp_chain_step has one.  A caller that cannot change that loop binds the chain's likelihood
 * evaluator and its ICP proposals (in the mixture's order) ONCE.  From then on
 *   - icp_proposal_propose of a bound proposal submits the WHOLE step — what icp_chain_step submits: the proposal, the proposed state's
 *     instance, its searches, every bound proposal's posterior there, the likelihood, all transition densities both ways — and returns
 *     when it is complete;
 *   - icp_evaluator_log_value of the bound evaluator for a state it has no value for (a random-walk or pose proposal made on the host)
 *     submits the same with the state of the PREVIOUS icp_evaluator_log_value call as the current state (MetropolisHastings.next evaluates
 *     the current state before it proposes; the Scala adapter passes every logValue through);
 *   - the calls that follow — logValue(proposal), logTransitionProbability(current, proposal), (proposal, current) — find their values
 *     on the host: the likelihood in the evaluator's Memoize(3), the densities parked under the exact (from, to) vectors of the two
 *     latest such steps.  Any other argument computes as before.
 * Values are those of the unbound calls, bit for bit (same device code, same caches; tests/test_gpu_dropin.py).  A bound step that
 * fails leaves the per-method call to compute — and report — on its own.  A proposal belongs to one binding at a time (binding it
 * again moves it); destroying a member dissolves the binding.  n_props == 0 unbinds.  Not for a caller that evaluates unrelated states
 * through the bound evaluator: every unseen state costs a whole step from the previous one. */
ICP_API int icp_chain_bind(icp_evaluator *e, int32_t n_props, icp_proposal *const *props);
/* out[0] whole steps submitted by icp_proposal_propose, out[1] by icp_evaluator_log_value, out[2] transition densities answered from
 * a parked step, since the binding was made. */
ICP_API int icp_chain_bind_stats(const icp_evaluator *e, int64_t out[3]);

/* ---------------------------------------------------------------- the whole Metropolis–Hastings loop on the device
 * n_steps steps of n_chains independent chains WITHOUT a host round trip per step: beside the five merged launches of
 * icp_chain_step_batched, a small kernel at the head of every step draws the mixture component and makes the step's proposal input
 * (Scalismo MixtureProposal.propose; api/sampling/proposals/RandomShapeUpdateProposal.scala:31-35), and one behind launch 5 is
 * MetropolisHastings.next (api/sampling/SamplingRegistration.scala:52-58): ModelPriorEvaluator × likelihood, the mixture's transition
 * ratio by log-sum-exp over all leaves, accept/reject, the step's record; the KL bases of accepted states follow in the same stream.
 * The host only enqueues launches and streams the standard normals in ahead.
 *   Mixture: (w_icp: the n_props ICP proposals with icp_weight) + (w_rw: shape random walk of rw_sigma) in the reference's order
 *   (apps/femur/IcpProposalRegistration.scala:70-72), optionally behind the six pose walks (w_pose > 0: apps/bfm/BfmFittingPartial.scala:70;
 *   the proposed pose's rotation matrix is made on the device with include/icp_sincos.h, the sines and cosines the host side and the
 *   oracle use — a context whose caller-supplied rotation matrices, icp_ctx_set_rotation, have all agreed with that convention is
 *   covered, one that ever supplied a different matrix is not: icp_ctx_rotation_convention); product evaluator = shape
 *   prior × `evaluator`.
 *   Random numbers: the counter-based generator of the C++ harness (host/icp_host.hpp StepRandom, shared bit for bit with the oracle):
 *   stream (seeds[b], step, lane), steps first_step[b] .. first_step[b] + n_steps − 1.
 *   theta[b] (in/out): the chain's current state; log_value[b] (in/out): its product log value (as MetropolisHastings carries it).
 *   records[b] (may be NULL): n_steps rows [index, accepted, leaf id (0/1 ICP proposal, 2 shape walk, 3..8 pose walks), log value, theta].
 * Covered (one context per chain, one device, one rank and sampler per run; otherwise ICP_ERR_INVALID_ARG and nothing has run):
 *   - what the five merged launches cover at ranks <= 64 (closed target or no boundary-aware branch): their launches, from
 *     device-resident records that change roles when a state is accepted;
 *   - (round 5) everything the WIDE step covers — targets with a boundary, the full-mesh Hausdorff evaluator, ranks up to 256 (round 6;
 *     200 until then: the reference's femur_gp_model_200-components.h5 has 201 components), the femur
 *     mixture at ranks 65..116 (apps/bfm/BfmFittingPartial.scala:62-96, apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala) — with
 *     the chains of a run sharing one model: the wide step's own launches replayed from device-resident records, an accepted state's
 *     posterior copied into the current state's entries; above rank 64 the proposed state is decomposed ahead of the decision, beside
 *     the factorisation and the evaluator's searches (KL-basis sampler; the Cholesky-root sampler up to rank 64).
 * Results are those of icp_chain_step_batched driven by the harness, chain by chain — bit for bit, except that the warm-started
 * Jacobi iteration of a wide step at ranks <= 64 starts from another basis than the host-stepped one's (states equal to 1e-11)
 * (tests/test_gpu_chain.py::test_device_loop_*, tests/test_gpu_wide_loop.py). */
typedef struct {
  /* = sizeof(icp_mh_mixture) of the header the caller was compiled against; anything else is refused with ICP_ERR_INVALID_ARG (the
   * structure grew in round 4: a caller built against the shorter one must not have its memory read past its end) */
  uint64_t struct_size;
  double icp_weight[2];
  double w_icp, w_rw;
  double rw_sigma;
  /* (round 4) the six pose walks of MixedProposalDistributions.mixedRandomPoseProposal (MixedProposalDistributions.scala:29-39;
   * PoseProposals.scala:31-90), first in the outer mixture as in apps/bfm/BfmFittingPartial.scala:70: w_pose = 0 -> none.
   * pose_rot_sigma = (yaw, pitch, roll), pose_trans_sigma = (x, y, z): the argument order of :29. */
  double w_pose;
  double pose_rot_sigma[3], pose_trans_sigma[3];
} icp_mh_mixture;
ICP_API int icp_chains_run_on_device(int32_t n_chains, icp_evaluator *const *evaluators, int32_t n_props, icp_proposal *const *props,
                                     const icp_mh_mixture *mixture, const uint64_t *seeds, const int64_t *first_step,
                                     double *const *theta, double *log_value, int32_t n_steps, double *const *records,
                                     int64_t *accepted);

/* ---------------------------------------------------------------- instrumentation (bench.py's roofline leg)
 * Between start and stop every kernel the context launches is bracketed by HIP events on the context stream;
 * stop returns one row per kernel name.  Off by default (adds nothing to the launch path). */
typedef struct {
  char name[40];
  int64_t calls;
  double total_ms, min_ms, max_ms;
} icp_kernel_stat;
ICP_API int icp_ctx_profile_start(icp_ctx *ctx, int32_t max_launches);
/* on != 0: the NEXT profile_start .. profile_stop interval also counts the tests the searches execute (per wave, with atomics on
 * a handful of device words — they slow the filter launches down, so this is for a short leg of its own, not for timing);
 * profile_stop then returns extra rows "count.surface_ball_tests", "count.surface_sphere_tests", "count.surface_exact_tests",
 * "count.vertex_filter_tests", "count.vertex_exact_tests" with the number in `calls`. */
ICP_API int icp_ctx_profile_search_counters(icp_ctx *ctx, int32_t on);
ICP_API int icp_ctx_profile_stop(icp_ctx *ctx, icp_kernel_stat *stats, int32_t capacity /* >= 32 */, int32_t *n_out);

/* ---- fall-back counters.  The step schedules above take their cross-stream order on the device (a launch waits for a word another
 * stream's launch raises) with time-outs behind them; every time-out ends in a slower but equivalent schedule, so a normal run must
 * show ZERO everywhere — anything else is a performance bug (or a tool that lets one kernel run at a time: rocprofv3 --pmc).
 * ctx == NULL: totals of the process since it started. */
typedef struct {
  int64_t wait_timeouts;        /* a step's first launch gave up waiting for its word (50 ms on the device) */
  int64_t speculation_giveups;  /* a KL basis started ahead never saw its input (5 ms) and the step that drew from it was repeated */
  int64_t pipeline_fallbacks;   /* contexts switched to the one-stream schedule for good after a time-out */
  int64_t step_redos;           /* steps computed twice because of any of the above */
  int64_t gate_timeouts;        /* batched steps: the launch sequence was not released because the batch's decompositions did not
                                   become resident in time (2 s) */
  int64_t reserved[3];
} icp_runtime_stats;
ICP_API int icp_ctx_runtime_stats(const icp_ctx *ctx, icp_runtime_stats *out);

/* ---- which path the chain steps took (diagnostic: the results do not depend on it).  Counts since the context was created or, with
 * ctx == NULL, of the process: out[0] the five merged launches (icp_chain_step[_batched]), out[1] the wide step (targets with a
 * boundary, the Hausdorff evaluator, ranks up to 256, pose moves: DESIGN.md), out[2] per-stage kernels, out[3] steps taken inside
 * icp_chains_run_on_device. */
ICP_API int icp_ctx_step_paths(const icp_ctx *ctx, int64_t out[4]);

/* Is the KL basis the proposal would draw from at `theta` ready?  2: the posterior of theta is on record and decomposed (or needs no
 * decomposition); 1: its decomposition is still on the device (started ahead by the step that proposed theta) — an ICP proposal from
 * theta would wait for it; 0: nothing on record (a step from theta computes it).  Never blocks.  A caller that steps many independent
 * chains uses it to let a chain whose basis is still under way sit out a round instead of holding the others back. */
ICP_API int icp_proposal_basis_state(icp_proposal *p, const double *theta);

/* Which path icp_chain_step[_batched] takes for this proposal set and evaluator (a property of the configuration, not of a state):
 * 0 the five merged launches, 1 the wide step, 2 per-stage kernels.  A caller that steps many chains uses it to size its batches:
 * the merged launches are short and want several groups of chains in flight, a wide step is long and wants one. */
ICP_API int icp_chain_step_path(icp_evaluator *e, int32_t n_props, icp_proposal *const *props);

/* ---- model cache.  Contexts made from the same model arrays share its derived device data (the scaled basis in two layouts, the
 * Gram matrix and its inverses: 0.35 s of host work and 2 x 137 MB of uploads at N = 28,561, rank 200).  The library keeps the two
 * most recently used models alive after their last context is destroyed, so that a job which builds one context per target over one
 * model (BASELINE.json configs[4]) pays for the model once; this call drops them (their device memory is freed as soon as no context
 * uses them).
 * Likewise the streams, pinned host blocks and device buffers of destroyed contexts, proposals and evaluators are kept for the next
 * ones (a job that makes its chains anew for every target spent a third of its time creating and destroying them): up to 96 streams
 * per device and priority class, 64 MiB of pinned memory, 6 GiB of device memory in blocks of at most 64 MiB.  This call gives all
 * of that back as well; the environment variable ICP_NO_POOL=1 (read when the library is loaded) switches the pools off. */
ICP_API void icp_release_cached_models(void);

/* ---- idle hook (optional).  icp_chain_step spends most of a step waiting for the device.  A caller that has host
 * work which does not depend on the step's outcome — drawing the random numbers of the NEXT step, say — registers it
 * here: `fn(arg)` is called once per icp_chain_step, on the calling thread, after the step's launches have been issued
 * and before the wait.  It may call icp_chain_step_prelaunch and nothing else of this library.  fn == NULL removes the hook.  Nothing in the
 * reference corresponds to it (its Breeze RNG is sequential); the C++ harness uses it with its counter-based RNG. */
typedef void (*icp_idle_fn)(void *arg);
ICP_API int icp_ctx_set_idle_hook(icp_ctx *ctx, icp_idle_fn fn, void *arg);

#ifdef __cplusplus
}
#endif
#endif /* ICP_PROPOSAL_H */
