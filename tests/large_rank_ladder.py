"""The ranks 65..501 at which the library takes another path, and the models of those ranks: the inputs of
tests/test_gpu_large_ranks.py, pinned without a GPU by tests/test_large_rank_ladder_cpu.py.  The sibling of tests/small_rank_ladder.py,
whose closed forms, truncated models and oracle parameters it uses.

DISPATCH restates, in Python, every decision of the native code that depends on a rank in 65..501 and SELECTS code — a template
instance, a kernel, a path, a refusal — with the file and function it comes from.  An edge is a rank r in 65..500 at which one of them
gives another answer for r + 1; LADDER must hold both sides of every edge, and 65, 256, 257 and 500 besides.  PERIODIC holds the
decisions that above 64 only change a trip count (the instance sum's loops, regression_tiles, the 16-padding of k_proj_* / k_pm_*):
the ladder has to hold at least one rank in each of their distinct states, not both sides of every period.

Readings of the code that differ from the obvious one:
 * with the tridiagonal route on (ranks 65..256, the default) launch_eigen_big is never the primary route: it is the status-2
   fall-back up to rank 200, cold (Vwarm = nullptr).  Warm states at 65..256 go through the tridiagonal route again, which takes no
   warm start.  The generic kernel k_posterior_eigen is the fall-back at 201..256 and the primary route from 257 on, where
   r·(r|1) doubles fit no LDS budget: a_in_lds = v_in_lds = 0 at every rank above 128, so Vwarm is dropped at every rank this
   module reaches it.
 * launch_transition_tails keeps both matrices of the iteration in LDS up to rank 89, one up to 125, and takes k_transition_tails<1024>
   from 126 on (r·(r|1) against kLdsDoubles − 2560) — not from 135 on, as its comment and launch_propose's say.
 * launch_transition_tail_direct (whether [M; bᵀ] is in LDS: 130 | 131) runs only where the fixed-point form of a transition density
   does not contract, which none of these models brings about; the edge is in the ladder, the kernel is not reached (DESIGN.md §9.3,
   "Not covered")."""
from conftest import make_theta
from small_rank_ladder import (DIRECTIONS, closed_form_log_transition, closed_form_propose, factor_tile_count, gram, instance_split,  # noqa: F401
                               matvec_tpr_log2, n_prime, oracle_params, smallest_relative_gap, truncated)
from test_gpu_eigen_spectra import factor_kernel  # launch_posterior_factor's ladder (kernels_factor.hip): one restatement per decision

MIN_RANK, MAX_RANK = 65, 500   # kMaxRank (abi_types.inl); 501 is the first rank a context refuses
LDS = 18432                    # kLdsDoubles (icp_dense.hpp)
CHOL_MAX = 256                 # kCholMaxRank (kernels_factor.hip) = kCholMaxRankAbi (abi_types.inl)
TRI_MAX = 256                  # kTriMaxRank (kernels_eigen.hip)
BIG_MAX = 200                  # kBigMaxRank (kernels_eigen.hip)
PM_MAX = 256                   # kPmMaxRank (abi_posterior_models.inl)
GPM_MAX_PIVOTS = 256           # kGpmMaxPivots (abi_gp_models.inl): rank <= n_pivots <= 256


# ---------------------------------------------------------------- the dispatch, restated

def context(r):
    """abi_context.inl, icp_ctx_create: rank <= kMaxRank"""
    return "accepted" if r <= MAX_RANK else "refused"


def finish_plan(r):
    """kernels_step.hip, finish_plan -> (tiles per thread, threads, n_lds, the backward tail's matrices behind the factor's region) of
    k_step_finish<E, NT>, or None: no merged step at this rank"""
    ld = r | 1
    tiles, w, one, budget = factor_tile_count(r), (r + 1) * ld, r * ld, LDS - 4700
    if w > budget:
        return None
    if tiles <= 256:
        e, nt = 1, 256
    elif tiles <= 1024:
        e, nt = 2, 512
    elif tiles <= 2048:
        e, nt = 2, 1024
    else:
        return None
    n_lds = 2 if 2 * one <= budget else (1 if one <= budget else 0)
    return e, nt, n_lds, n_lds == 2 and w + one * n_lds <= budget


def finish_tails_tpr(r):
    """kernels_step.hip, launch_step_finish: above 64 the finish launch's tails take the threads per row of the launch's own size"""
    p = finish_plan(r)
    return None if p is None else matvec_tpr_log2(r, p[1])


def eigen_speculation_supported(r):
    """kernels_eigen.hip"""
    return 3 <= r <= 64


def tridiag_route(r):
    """kernels_eigen.hip, tridiag_route = eigen_tridiag_many_supported"""
    return 64 < r <= TRI_MAX


def wide_rank_covered(r, root=False):
    """abi_wide.inl"""
    if r < 3 or r > 256:
        return False
    return r <= CHOL_MAX if root else (eigen_speculation_supported(r) or tridiag_route(r))


def step_path(r, closed):
    """abi_batched.inl, icp_chain_step_path, for the chain configurations of this module: step_pipeline_covers (abi_methods.inl)
    holds on a closed target where step_finish_supported(r) does — on a target with a boundary a boundary-aware ModelSampling proposal
    needs the nearest-vertex pass, which the merged step has not —, then wide_pipeline_covers (abi_wide.inl: wide_rank_covered), then the
    per-stage kernels"""
    if closed and finish_plan(r) is not None:
        return "merged"
    return "wide" if wide_rank_covered(r) else "per_stage"


def factor_launch(r):
    """kernels_factor.hip, launch_posterior_factor -> (the kernel, k_sum_partials ahead of it, the generic kernel's matrix in LDS)"""
    kernel = factor_kernel(r)
    ld = r | 1
    w_fits = (r + 1) * ld <= LDS - 2000
    generic = kernel == "k_posterior_factor_generic"
    return kernel, (not w_fits) and r <= CHOL_MAX, generic and (r + 1) * ld <= LDS


def root_sampler(r):
    """abi_posterior.inl, icp_proposal::posterior (root_here) and abi_methods.inl, icp_proposal_set_sampler: above 64 the posterior's
    own factorisation hands the factor out (Lout, Sout), whichever kernel that is; refused above kCholMaxRankAbi"""
    return ("Lout of " + factor_kernel(r)) if r <= CHOL_MAX else "refused"


def propose_launch(r, root=False):
    """kernels_posterior.hip, launch_propose; kernels_wide.hip, launch_wide_propose and launch_wide_propose_resident take the same
    block size and threads per row, rank by rank -> (threads, log2 of the threads that share a row)"""
    if root:
        return (1024, matvec_tpr_log2(r, 1024)) if r <= CHOL_MAX else None
    if r > 134:
        return 1024, 4
    return 256, matvec_tpr_log2(r, 256)


def tails_launch(r):
    """kernels_posterior.hip, launch_transition_tails -> (threads, matrices in LDS, log2 of the threads that share a row)"""
    one = r * (r | 1)
    n_lds = 2 if 2 * one <= LDS - 2560 else (1 if one <= LDS - 2560 else 0)
    return (1024, 0, 4) if n_lds == 0 else (256, n_lds, matvec_tpr_log2(r, 256))


def tail_direct_in_lds(r):
    """kernels_posterior.hip, launch_transition_tail_direct (the fall-back of a tail whose fixed point does not contract)"""
    return (r + 1) * (r | 1) <= LDS - 1200


def mhw_decide(r):
    """kernels_step.hip, launch_mhw_decide, inside the on-device loop, which above 64 needs the tridiagonal route (abi_wide_loop.inl)"""
    if not tridiag_route(r):
        return None
    return "k_mhw_decide<2>" if r <= 128 else "k_mhw_decide<4>"


def tri_shapes(r):
    """kernels_eigen.hip, tri_reduction_shape and tri_row_slots -> (<waves, row slots, column slots a wave, empty column slots> of
    k_tridiag, row slots of k_tri_solve / k_tri_back)"""
    if not tridiag_route(r):
        return None
    red = (4, 2, 32, 0) if r <= 128 else (8, 3, 24, 0) if r <= 192 else (8, 4, 25, 7) if r <= 200 else (8, 4, 26, 6) if r <= 208 else (8, 4, 32, 0)
    return red, 2 if r <= 128 else 3 if r <= 192 else 4


def generic_eigen_lds(r):
    """kernels_eigen.hip, launch_posterior_eigen -> (a_in_lds, v_in_lds) of the generic launch; without a_in_lds the warm start is dropped"""
    budget = LDS - 1800
    return r * (r | 1) <= budget, 2 * r * (r | 1) <= budget


def eigen_route(r):
    """kernels_eigen.hip, launch_posterior_eigen: the primary route of one posterior's decomposition"""
    if tridiag_route(r):
        return "tridiagonal"
    return ("k_posterior_eigen",) + generic_eigen_lds(r)


def eigen_fallback(r):
    """kernels_eigen.hip, launch_posterior_eigen / launch_eigen_big: what decomposes a spectrum the multisection could not separate
    (status 2) — k_eigen_big<square> with the full image in LDS, k_eigen_big on the packed triangle, the generic kernel behind L2"""
    if not tridiag_route(r):
        return None
    if r <= BIG_MAX:
        return "k_eigen_big<true>" if r <= 140 else "k_eigen_big<false>"
    return "k_posterior_eigen(0, 0)"


def batched_limits(r):
    """abi_posterior_models.inl (kPmMaxRank: an item of a larger rank gets ICP_ERR_INVALID_ARG), abi_gp_models.inl (rank <= n_pivots <=
    kGpmMaxPivots), abi_projection_many.inl (no limit of its own: every rank a context has) -> (posterior models, gp models, projection)"""
    return r <= PM_MAX, r <= GPM_MAX_PIVOTS, r <= MAX_RANK


DISPATCH = {
    "context": (context, "abi_context.inl: icp_ctx_create"),
    "finish_plan": (finish_plan, "kernels_step.hip: finish_plan"),
    "finish tails' threads per row": (finish_tails_tpr, "kernels_step.hip: launch_step_finish"),
    "step path, closed target": (lambda r: step_path(r, True), "abi_batched.inl: icp_chain_step_path"),
    "step path, open target": (lambda r: step_path(r, False), "abi_batched.inl: icp_chain_step_path"),
    "factor launch": (factor_launch, "kernels_factor.hip: launch_posterior_factor"),
    "root sampler": (root_sampler, "abi_posterior.inl: root_here; abi_methods.inl: icp_proposal_set_sampler"),
    "propose, eigen sampler": (propose_launch, "kernels_posterior.hip: launch_propose; kernels_wide.hip: launch_wide_propose(_resident)"),
    "propose, root sampler": (lambda r: propose_launch(r, True), "kernels_posterior.hip: launch_propose; kernels_wide.hip: launch_wide_propose"),
    "transition tails": (tails_launch, "kernels_posterior.hip: launch_transition_tails"),
    "direct tail in LDS": (tail_direct_in_lds, "kernels_posterior.hip: launch_transition_tail_direct"),
    "k_mhw_decide": (mhw_decide, "kernels_step.hip: launch_mhw_decide"),
    "tridiagonal shapes": (tri_shapes, "kernels_eigen.hip: tri_reduction_shape, tri_row_slots"),
    "eigen route": (eigen_route, "kernels_eigen.hip: launch_posterior_eigen"),
    "eigen fall-back": (eigen_fallback, "kernels_eigen.hip: launch_posterior_eigen, launch_eigen_big"),
    "wide step covered": (wide_rank_covered, "abi_wide.inl: wide_rank_covered"),
    "batched entry points": (batched_limits, "abi_posterior_models.inl, abi_gp_models.inl, abi_projection_many.inl"),
}


def instance_state(r):
    """icp_search.hpp, instance_point: above 64 a batch of 25 always runs -> (batches of 10 present, a remainder present)"""
    _, n10, rem = instance_split(r)
    return n10 > 0, rem > 0


def pad_state(r):
    """abi_projection_many.inl / kernels_posterior_model.hip: r ≡ 0, r ≡ 15 (r + 1 fills its last tile: regression_tiles,
    posterior_model_pads) or neither, mod 16"""
    return {0: "0", 15: "15"}.get(r % 16, "neither")


PERIODIC = {
    "instance loops": (instance_state, ((False, False), (False, True), (True, False), (True, True))),
    "16-padding and regression_tiles": (pad_state, ("0", "15", "neither")),
}


def edges(decision):
    """the ranks r in 65..500 with decision(r) != decision(r + 1)"""
    return [r for r in range(MIN_RANK, MAX_RANK + 1) if decision(r) != decision(r + 1)]


def derived_ladder():
    out = {MIN_RANK, 256, 257, MAX_RANK}
    for fn, _ in DISPATCH.values():
        for r in edges(fn):
            out.update((r, r + 1))
    out.discard(MAX_RANK + 1)   # 501: no context, tested on its own
    return tuple(sorted(out))


def stands_for(r):
    """the edges rank r is a side of -> ["name e | e + 1", ...] (DESIGN.md §9.3 is written from this)"""
    return [f"{name} {e} | {e + 1}" for name, (fn, _) in DISPATCH.items() for e in edges(fn) if r in (e, e + 1)]


# both sides of every edge of DISPATCH, and 65, 256, 257, 500 (tests/test_large_rank_ladder_cpu.py: equal to derived_ladder()); the
# states of PERIODIC are all among them
LADDER = (65, 67, 68, 82, 83, 89, 90, 116, 117, 125, 126, 127, 128, 129, 130, 131, 134, 135, 140, 141, 192, 193, 200, 201, 208, 209, 217,
          218, 253, 254, 256, 257, 500)
REFUSED_RANK = MAX_RANK + 1
CHAIN_RANKS = (65, 116, 117, 129, 135, 218, 254, 257)   # short chains against the oracle
# steps of those chains, from the oracle chain's time on a CPU (tests/test_large_rank_ladder_cpu.py prints it)
CHAIN_STEPS = {65: 12, 116: 6, 117: 6, 129: 6, 135: 6, 218: 5, 254: 4, 257: 4}


# ---------------------------------------------------------------- the models

FACE_GRID, FACE_REMOVE = 41, 60   # data.synthetic_face_model(grid=41): 1,681 vertices, 1,023 modes available


def source(r):
    """femur-100 (rank 101) up to 101, femur-200 (rank 201) up to 201 — the merged | wide edge at 116 | 117 needs the closed femur
    target —, above the synthetic face model with its open target (tests/test_gpu_rank201.py)"""
    return "femur-100" if r <= 101 else "femur-200" if r <= 201 else "face"


def closed_target(r):
    return source(r) != "face"


def chain_setup(pkg, model, target):
    """-> (setup, initial state, seed) of the short chains: the femur study's registration (tests/test_gpu_chain.py) on the closed
    femur target, BfmFittingPartial with the collective evaluator (tests/test_gpu_rank201.py) on the face model's open one"""
    if closed_target(model.rank):
        return pkg.femur_icp_proposal_registration(model, target, fused=2), pkg.initial_parameters(model), 1024
    return pkg.bfm_fitting_partial(model, target, evaluator="collective", fused=2), pkg.random_initial_parameters(model, 3), 55


def ladder_model(pkg, r):
    """-> (model, target) on arrays of their own"""
    s = source(r)
    if s == "face":
        model = pkg.data.synthetic_face_model(grid=FACE_GRID, rank=r)
        return model, pkg.data.synthetic_partial_target(model, n_remove=FACE_REMOVE)
    return truncated(pkg, 100 if s == "femur-100" else 200, r)


# (make_theta seed, shape_scale, K / r) of the parity state per rank: (100, 0.5, 2) — the parity test's — unless that state misses the
# gap condition of tests/test_large_rank_ladder_cpu.py (smallest gap of N' at least 1e-5·μ_max, in both directions); entries are chosen
# with 1.1e-5 so that the condition does not hang on a digit.
#  * 83: (100, 0.5) gives less than 1e-5; the first seed from 100 on that gives 1.1e-5 is 102.
#  * 116..141, cut from femur-200, ModelSampling: ONE pair (eigenvalues 15 and 16 from below) sits 3.5e-6..4.4e-6 apart at K = 2r; no
#    seed in 100..139 at scale 0.5 or 1.0 moves it and K = 3r fails at 116 and 117.  K = 4r with the default state gives 1.6e-5 and more
#    at every one of these ranks, every correspondence kept.  K changes the number of split-K partials, not a rank route.
# The figures per rank are printed by the CPU test.
PARITY_STATE = {83: (102, 0.5, 2), **{r: (100, 0.5, 4) for r in (116, 117, 125, 126, 127, 128, 129, 130, 131, 134, 135, 140, 141)}}


def parity_state(r):
    return PARITY_STATE.get(r, (100, 0.5, 2))


def parity_K(r):
    return parity_state(r)[2] * r


def parity_theta(model):
    seed, scale, _ = parity_state(model.rank)
    return make_theta(model, seed, shape_scale=scale)
