// icp_abi.hip — host side of libicp_proposal_amd.so: the C ABI of include/icp_proposal.h.
//
// Owns device memory, the per-context HIP stream, the state / posterior / likelihood caches that stand in
// for the reference's Memoize wrappers (NonRigidIcpProposal.scala:49, evaluators/EvaluationCaching.scala:32),
// and the order in which kernels are enqueued.  Every entry point enqueues its whole kernel sequence on the
// context stream and synchronises ONCE, when results are copied back.  No CPU fallback exists: without a HIP
// device icp_ctx_create fails.
//
// ONE translation unit, split by concern (round 5; it was a single 5,200-line file): the parts below are included in this order.
#include "abi_types.inl"  // common types: errors, device buffers, shared model / target data, state slots, icp_ctx
#include "abi_state.inl"  // icp_ctx: state slots (instances) and the search prefixes shared by proposals and evaluators
#include "abi_pools.inl"  // pools and caches: streams, pinned blocks, device buffers of destroyed objects; live-context and eigen-stream registries
#include "abi_posterior.inl"  // posterior memo entries, icp_proposal / icp_evaluator and their methods (NonRigidIcpProposal.scala:88-153, the evaluators)
#include "abi_hints.inl"  // search hints handed from the first evaluation of a (model, target) pair to the contexts and evaluators that follow
#include "abi_context.inl"  // C ABI: contexts — create / destroy / set_target / set_rotation, counters, profiling, geometry entry points
#include "abi_methods.inl"  // C ABI: per-method entry points — proposals, evaluators, deterministic fit, variability maps, metrics, icp_chain_eval_step
#include "abi_many.inl"  // what the batched entry points below share: context locks, argument checks, instance plan, status epilogue
#include "abi_pool_many.inl"  // what the context-free entry points below share: device choice, pooled stream, live items, argument loops, a kernel term's record; the round and piece plans of icp_round_plan.hpp
#include "abi_fit_many.inl"  // C ABI: icp_fit_deterministic_many (many deterministic fits in lockstep, kernels_fit.hip)
#include "abi_metrics_many.inl"  // C ABI: icp_mesh_metrics_many (registration metrics and Dice of many meshes, kernels_metrics.hip)
#include "abi_variability_many.inl"  // C ABI: icp_posterior_variability_many (variability maps of many chains, kernels_variability.hip)
#include "abi_projection_many.inl"  // C ABI: icp_model_instances_many / icp_model_coefficients_many (model projection of many meshes, kernels_projection.hip)
#include "abi_log_values_many.inl"  // C ABI: icp_evaluator_log_values_many (log values of many states under many evaluators, kernels_evaluate.hip)
#include "abi_registration_maps.inl"  // C ABI: icp_registration_maps_many / icp_distance_summaries_many (per-vertex registration maps and chain summaries, kernels_maps.hip)
#include "abi_posterior_models.inl"  // C ABI: icp_posterior_models_many (posterior shape models of given correspondences, kernels_posterior_model.hip)
#include "abi_gp_models.inl"  // C ABI: icp_gp_models_many (Gaussian-process shape models from analytic kernels by pivoted Cholesky, kernels_gp_model.hip)
#include "abi_pca_models.inl"  // C ABI: icp_pca_models_many (PCA shape models of registered meshes with Procrustes alignment, kernels_pca_model.hip; the m-space half of abi_gp_models.inl)
#include "abi_nystrom_models.inl"  // C ABI: icp_nystrom_models_many (GP shape models by the Nyström approximation on sample points, kernels_nystrom_model.hip)
#include "abi_scan_prep.inl"  // C ABI: icp_scans_prepare_many (aligned and partial targets of many raw scans, kernels_scan_prep.hip)
#include "abi_decimate.inl"  // C ABI: icp_decimate_many (decimation of many meshes to vertex subsets, kernels_decimate.hip)
#include "abi_samples.inl"  // C ABI: icp_surface_samples_many / icp_kernel_total_variance_many (uniform surface samples with nearest vertices; a kernel's mean trace, kernels_samples.hip)
#include "abi_step.inl"  // the merged step (five launches): flag poll, argument checks and finish arguments its entry points share; fronts, speculative decompositions, icp_chain_step_prelaunch; icp_chain_step in phases
#include "abi_wide.inl"  // the wide step's host side (kernels_wide.hip)
#include "abi_batched.inl"  // C ABI: icp_chain_step_batched (_issue / _collect / _abandon), icp_chain_step_path, icp_proposal_basis_state
#include "abi_loop_common.inl"  // what the two on-device MH loops below share: arguments and checks, the MhChain fill, a group's buffers, the harness' normals and their feed, drain and hand-out
#include "abi_wide_loop.inl"  // the whole MH loop on the device for chains whose step is the wide one
#include "abi_device_loop.inl"  // C ABI: icp_chains_run_on_device (the whole MH loop on the device: the merged step's loop, dispatch to the wide one)
