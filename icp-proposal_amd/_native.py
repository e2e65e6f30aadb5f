"""ctypes binding of libicp_proposal_amd.so — the C ABI declared in include/icp_proposal.h.

There is deliberately no fallback: if the HIP library is missing or no GPU is usable, loading / context
creation raises.  Nothing under oracle/ is ever imported from here.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ICP_LIBRARY_PATH: a test process may ask for the build with the test hooks compiled in (libicp_proposal_amd_testhooks.so)
LIB_PATH = os.environ.get("ICP_LIBRARY_PATH") or os.path.join(_HERE, "libicp_proposal_amd.so")

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int32)
c_ubyte_p = C.POINTER(C.c_uint8)
c_uint64_p = C.POINTER(C.c_uint64)


class ModelDesc(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_triangles", C.c_int32), ("rank", C.c_int32),
                ("ref_points", c_double_p), ("mean_deformation", c_double_p), ("basis", c_double_p),
                ("variance", c_double_p), ("triangles", c_int_p)]


class MeshDesc(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_triangles", C.c_int32), ("points", c_double_p), ("triangles", c_int_p)]


class ProposalParams(C.Structure):
    _fields_ = [("step_length", C.c_double), ("tangential_noise", C.c_double), ("noise_along_normal", C.c_double),
                ("direction", C.c_int32), ("boundary_aware", C.c_int32), ("n_model_ids", C.c_int32),
                ("n_target_points", C.c_int32), ("target_points", c_double_p)]


class EvaluatorParams(C.Structure):
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("n_model_ids", C.c_int32), ("n_target_points", C.c_int32),
                ("target_points", c_double_p), ("gauss_mean", C.c_double), ("gauss_sigma", C.c_double),
                ("exp_rate", C.c_double)]


class PosteriorView(C.Structure):
    _fields_ = [("n_candidates", C.c_int32), ("corr_id", c_int_p), ("corr_aux", c_int_p), ("corr_point", c_double_p),
                ("keep", c_ubyte_p), ("alpha", c_double_p), ("M", c_double_p), ("V", c_double_p), ("S", c_double_p)]


class FitParams(C.Structure):
    _fields_ = [("direction", C.c_int32), ("n_model_ids", C.c_int32), ("model_ids", c_int_p), ("n_target_points", C.c_int32),
                ("target_points", c_double_p), ("step_length", C.c_double)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 40), ("calls", C.c_int64), ("total_ms", C.c_double), ("min_ms", C.c_double),
                ("max_ms", C.c_double)]


class MhMixture(C.Structure):
    _fields_ = [("struct_size", C.c_uint64), ("icp_weight", C.c_double * 2), ("w_icp", C.c_double), ("w_rw", C.c_double), ("rw_sigma", C.c_double),
                ("w_pose", C.c_double), ("pose_rot_sigma", C.c_double * 3), ("pose_trans_sigma", C.c_double * 3)]


class RuntimeStats(C.Structure):
    _fields_ = [("wait_timeouts", C.c_int64), ("speculation_giveups", C.c_int64), ("pipeline_fallbacks", C.c_int64),
                ("step_redos", C.c_int64), ("gate_timeouts", C.c_int64), ("reserved", C.c_int64 * 3)]


class KernelTerm(C.Structure):
    _fields_ = [("scale", C.c_double), ("sigma", C.c_double), ("A", C.c_double * 9)]


KERNEL_GAUSSIAN, KERNEL_BSPLINE3 = 0, 1


class KernelTermGeneral(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("scale", C.c_double), ("sigma", C.c_double), ("level", C.c_int32),
                ("mirror_axis", C.c_int32), ("mirror_gain", C.c_double), ("A", C.c_double * 9), ("weights", c_double_p)]


class ScanTransform(C.Structure):
    _fields_ = [("struct_size", C.c_uint64), ("pre_scale", C.c_double), ("rotation", C.c_double * 9), ("centre", C.c_double * 3),
                ("translation", C.c_double * 3)]


# every symbol include/icp_proposal.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "icp_ctx_create": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(MeshDesc), C.c_int, C.POINTER(C.c_void_p)]),
    "icp_ctx_create_keyed": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(MeshDesc), C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "icp_ctx_destroy": (None, [C.c_void_p]),
    "icp_ctx_expect": (C.c_int, [C.c_int, C.c_int32]),
    "icp_ctx_set_target": (C.c_int, [C.c_void_p, C.POINTER(MeshDesc)]),
    "icp_status_string": (C.c_char_p, [C.c_int]),
    "icp_last_error": (C.c_char_p, []),
    "icp_ctx_rank": (C.c_int, [C.c_void_p]),
    "icp_ctx_device": (C.c_int, [C.c_void_p]),
    "icp_transformed_mesh": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "icp_vertex_normals": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "icp_closest_point_on_target": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, c_double_p, c_int_p, c_double_p]),
    "icp_closest_target_vertex": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, c_int_p, c_double_p]),
    "icp_closest_model_vertex": (C.c_int, [C.c_void_p, c_double_p, C.c_int32, c_double_p, c_int_p, c_double_p]),
    "icp_closest_point_on_model": (C.c_int, [C.c_void_p, c_double_p, C.c_int32, c_double_p, c_double_p, c_int_p, c_double_p]),
    "icp_proposal_create": (C.c_int, [C.c_void_p, C.POINTER(ProposalParams), C.POINTER(C.c_void_p)]),
    "icp_proposal_destroy": (None, [C.c_void_p]),
    "icp_proposal_num_candidates": (C.c_int, [C.c_void_p]),
    "icp_proposal_set_sampler": (C.c_int, [C.c_void_p, C.c_int32]),
    "icp_proposal_propose": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_int_p]),
    "icp_proposal_log_transition": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "icp_proposal_posterior": (C.c_int, [C.c_void_p, c_double_p, C.POINTER(PosteriorView)]),
    "icp_evaluator_create": (C.c_int, [C.c_void_p, C.POINTER(EvaluatorParams), C.POINTER(C.c_void_p)]),
    "icp_evaluator_destroy": (None, [C.c_void_p]),
    "icp_evaluator_log_value": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "icp_prior_log_value": (C.c_int, [C.c_int32, c_double_p, c_double_p]),
    "icp_ctx_profile_start": (C.c_int, [C.c_void_p, C.c_int32]),
    "icp_ctx_profile_search_counters": (C.c_int, [C.c_void_p, C.c_int32]),
    "icp_ctx_set_idle_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "icp_chain_step_prelaunch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "icp_chain_step_prelaunch2": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.POINTER(C.c_int32)]),
    "icp_ctx_twin_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "icp_ctx_search_hints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]),
    "icp_ctx_twin_eigen_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "icp_ctx_profile_stop": (C.c_int, [C.c_void_p, C.POINTER(KernelStat), C.c_int32, C.POINTER(C.c_int32)]),
    "icp_chain_eval_step": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), c_double_p, c_double_p, c_double_p,
                                      c_double_p, c_double_p]),
    "icp_fit_deterministic": (C.c_int, [C.c_void_p, C.POINTER(FitParams), c_double_p, C.c_int32, C.c_int32, c_double_p, c_double_p]),
    "icp_fit_deterministic_many": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.POINTER(FitParams)), C.POINTER(c_double_p),
                                             c_ubyte_p, C.c_int32, C.c_int32, c_double_p, C.POINTER(c_double_p), c_int_p]),
    "icp_posterior_variability": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, C.c_int32, c_double_p, c_double_p]),
    "icp_posterior_variability_many": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), c_int_p, C.POINTER(c_double_p), c_int_p,
                                                 C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p)]),
    "icp_mesh_metrics": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "icp_mesh_metrics_many": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(c_double_p), C.c_int32, C.c_uint64, c_double_p,
                                        c_int_p]),
    "icp_registration_maps_many": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(c_double_p), C.POINTER(c_double_p),
                                             C.POINTER(c_int_p), C.POINTER(c_double_p), C.POINTER(c_ubyte_p), C.POINTER(c_double_p),
                                             C.POINTER(c_int_p), C.POINTER(c_double_p), c_int_p]),
    "icp_distance_summaries_many": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), c_int_p, C.POINTER(c_double_p), C.POINTER(c_double_p),
                                              C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p), c_int_p]),
    "icp_evaluator_log_values_many": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(c_double_p), c_double_p, c_double_p,
                                                c_int_p]),
    "icp_model_instances_many": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(c_double_p), C.POINTER(c_double_p)]),
    "icp_model_coefficients_many": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(c_double_p), C.POINTER(c_double_p),
                                              C.POINTER(c_double_p), c_double_p, C.POINTER(c_double_p), c_int_p]),
    "icp_posterior_models_many": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), c_int_p, C.POINTER(c_int_p), C.POINTER(c_double_p),
                                            C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p),
                                            C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p), c_int_p]),
    "icp_gp_models_many": (C.c_int, [C.c_int32, C.c_int, c_int_p, C.POINTER(c_double_p), c_int_p, C.POINTER(C.POINTER(KernelTerm)), c_int_p,
                                     c_int_p, c_double_p, C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_int_p),
                                     C.POINTER(c_double_p), C.POINTER(c_double_p), c_int_p]),
    "icp_gp_models_general_many": (C.c_int, [C.c_int32, C.c_int, c_int_p, C.POINTER(c_double_p), c_int_p,
                                             C.POINTER(C.POINTER(KernelTermGeneral)), c_int_p, c_int_p, c_double_p, C.POINTER(c_double_p),
                                             C.POINTER(c_double_p), C.POINTER(c_int_p), C.POINTER(c_double_p), C.POINTER(c_double_p), c_int_p]),
    "icp_region_weights_many": (C.c_int, [C.c_int32, C.c_int, c_int_p, C.POINTER(c_double_p), c_int_p, C.POINTER(c_double_p), c_double_p,
                                          C.POINTER(c_double_p), c_int_p]),
    "icp_nystrom_models_many": (C.c_int, [C.c_int32, C.c_int, c_int_p, C.POINTER(c_double_p), c_int_p, C.POINTER(c_double_p), c_int_p,
                                          C.POINTER(C.POINTER(KernelTermGeneral)), C.POINTER(C.POINTER(c_double_p)), c_int_p, c_double_p,
                                          C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p),
                                          C.POINTER(c_double_p), c_int_p]),
    "icp_pca_models_many": (C.c_int, [C.c_int32, C.c_int, C.c_int32, c_int_p, C.POINTER(c_double_p), c_int_p, C.POINTER(c_int_p),
                                      C.POINTER(c_double_p), c_int_p, c_int_p, c_double_p, C.POINTER(c_double_p), C.POINTER(c_double_p),
                                      C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p), c_int_p]),
    "icp_scans_prepare_many": (C.c_int, [C.c_int32, C.c_int, c_int_p, C.POINTER(c_double_p), c_int_p, C.POINTER(c_int_p),
                                         C.POINTER(ScanTransform), c_int_p, C.POINTER(c_double_p), c_int_p, C.POINTER(c_int_p),
                                         C.POINTER(c_int_p), c_int_p, C.POINTER(c_int_p), C.POINTER(c_double_p), C.POINTER(c_double_p),
                                         C.POINTER(c_ubyte_p), C.POINTER(c_double_p), C.POINTER(c_int_p), C.POINTER(c_int_p), c_int_p,
                                         c_int_p]),
    "icp_decimate_many": (C.c_int, [C.c_int32, C.c_int, c_int_p, C.POINTER(c_double_p), c_int_p, C.POINTER(c_int_p), c_int_p, c_int_p, c_int_p,
                                    C.POINTER(c_int_p), C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_int_p), C.POINTER(c_int_p),
                                    c_int_p]),
    "icp_surface_samples_many": (C.c_int, [C.c_int32, C.c_int, c_int_p, C.POINTER(c_double_p), c_int_p, C.POINTER(c_int_p), c_int_p, c_uint64_p,
                                           C.POINTER(c_double_p), C.POINTER(c_int_p), C.POINTER(c_double_p), C.POINTER(c_int_p),
                                           C.POINTER(c_double_p), c_int_p]),
    "icp_kernel_total_variance_many": (C.c_int, [C.c_int32, C.c_int, c_int_p, C.POINTER(c_double_p), c_int_p,
                                                 C.POINTER(C.POINTER(KernelTermGeneral)), C.POINTER(C.POINTER(c_double_p)), c_double_p,
                                                 c_int_p]),
    "icp_chain_step":(C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, c_double_p, c_double_p, c_double_p,
                                 c_double_p, c_double_p, c_double_p]),
    "icp_chain_step_batched_issue": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                               C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p), c_double_p,
                                               c_double_p, c_double_p, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_void_p)]),
    "icp_chain_step_batched_collect": (C.c_int, [C.c_void_p]),
    "icp_chain_step_batched_abandon": (C.c_int, [C.c_void_p]),
    "icp_ctx_set_rotation": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "icp_ctx_rotation_convention": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "icp_ctx_runtime_stats": (C.c_int, [C.c_void_p, C.POINTER(RuntimeStats)]),
    "icp_ctx_step_paths": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "icp_chain_step_path": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "icp_proposal_basis_state": (C.c_int, [C.c_void_p, c_double_p]),
    "icp_chain_bind": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "icp_chain_bind_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "icp_release_cached_models": (None, []),
    "icp_chains_run_on_device": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(MhMixture),
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(c_double_p), c_double_p, C.c_int32,
                                           C.POINTER(c_double_p), C.POINTER(C.c_int64)]),
    "icp_chain_step_batched": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                         C.POINTER(c_double_p), C.POINTER(c_double_p), C.POINTER(c_double_p), c_double_p, c_double_p,
                                         c_double_p, C.POINTER(C.c_int32)]),
}

_LIB = None


class IcpNativeError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__(f"{where}: status {status} ({detail})")


def lib():
    """Load libicp_proposal_amd.so (built by __graft_entry__.build() / csrc/Makefile).  Raises if absent."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise IcpNativeError(-2, "load", f"{LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'`; "
                                             "there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(status, where):
    if status != 0:
        L = lib()
        detail = (L.icp_last_error() or b"").decode() or (L.icp_status_string(status) or b"").decode()
        raise IcpNativeError(status, where, detail)


def step_paths(ctx_handle=None) -> dict:
    """icp_ctx_step_paths: how many chain steps took which path (of one context, or of the process)."""
    out = (C.c_int64 * 4)()
    check(lib().icp_ctx_step_paths(ctx_handle, out), "icp_ctx_step_paths")
    return {"merged": int(out[0]), "wide": int(out[1]), "per_stage": int(out[2]), "device_loop": int(out[3])}


def twin_stats(ctx_handle) -> dict:
    """icp_ctx_twin_stats: twin passes issued, second-lane results used, second-lane results dropped (icp_chain_step_prelaunch2)."""
    out = (C.c_int64 * 3)()
    check(lib().icp_ctx_twin_stats(ctx_handle, out), "icp_ctx_twin_stats")
    return {"passes": int(out[0]), "lane1_used": int(out[1]), "lane1_dropped": int(out[2])}


def twin_eigen_stats(ctx_handle) -> dict:
    """icp_ctx_twin_eigen_stats: second-lane decompositions started with the first lane's, kept, cancelled because the first lane
    was accepted, started cold."""
    out = (C.c_int64 * 4)()
    check(lib().icp_ctx_twin_eigen_stats(ctx_handle, out), "icp_ctx_twin_eigen_stats")
    return {"started_early": int(out[0]), "kept": int(out[1]), "cancelled_by_lane0": int(out[2]), "started_cold": int(out[3])}


def runtime_stats(ctx_handle=None) -> dict:
    """icp_ctx_runtime_stats: fall-back counters of one context (its handle) or, with None, of the whole process.  A normal run
    shows zero everywhere."""
    st = RuntimeStats()
    check(lib().icp_ctx_runtime_stats(ctx_handle, C.byref(st)), "icp_ctx_runtime_stats")
    return {k: int(getattr(st, k)) for k, _ in RuntimeStats._fields_ if k != "reserved"}
