"""The counts at which the batched entry points (icp_model_instances_many, icp_model_coefficients_many, icp_posterior_models_many,
icp_posterior_variability_many, icp_mesh_metrics_many, icp_evaluator_log_values_many, icp_registration_maps_many,
icp_distance_summaries_many) take another path — N model vertices, n items of a call, K observations of a posterior-model item, S
samples of a variability map, S_d Dice samples, D distances of a reduction, T and V searched elements, S_sum samples of a summary set —
and the models, states, observation sets and sample sets of those counts: the inputs of tests/test_gpu_batched_counts.py, pinned
without a GPU by tests/test_batched_count_ladder_cpu.py.  tests/count_ladder.py does the same for the searches, the regression and
the merged step, and this module takes its meshes and its `edges` / `derived_ladder` from there.

DISPATCH restates every decision that the family's kernels and host planners take on one of those counts, the file and function
beside it.  A decision is what selects code — one slab or several, a loop that runs or does not, a dead step, a second group —, not a
trip count.  PERIODIC holds the decisions that repeat with a period: they are taken over one period at the smallest counts.  PAIRS
holds the decisions on two counts at their smallest shape.

Readings of the code that differ from the obvious one:
 * a mode-1 variability map of S = 32,768 samples runs in TWO segments (32,767 + 1), not one: its reference mesh holds a place of the
   round (`held` = 1 when the first segment is cut); modes 0 and 2 run one segment at 32,768 and two at 32,769.
 * k_pm_regression has no loop of four: one matrix instruction per observation.  Its K edges are regression_splits' alone (kchunk,
   empty leaves); regression_tile's 3 | 4 and 4 | 5 do not exist here.  REGRESSION_KS holds both sides of every edge it does have.
 * eval_gauss (the Gaussian log-pdf sum) runs at 256 threads whatever K; only eval_stats switches at 4,096.
 * the log values' model-side queries of the items that share a target are ONE packed query list: the searches see n·K_m queries.
 * Dice has no edge at 255 | 256: k_met_samples and k_met_dice_count launch cdiv(n, 256) workgroups (256 | 257) and a thread past n
   contributes false to a ballot.  The third range starts at 65,536 | 65,537; both sides are in the ladder.
 * the Dice rounds close after 2·kMetMaxChunk = 128 ranges: a chunk of 64 items reaches that with S_d > 65,536 (192 ranges).  Not
   covered on the device (64 × 65,537 samples); the restatement holds the edge.
 * a summary set that spans three chunks of kMapMaxChunk = 64 samples has a middle segment (neither first nor last) and takes its
   carry from the other half of the ping-pong buffer: S_sum = 128 | 129.
 * eval_max folds 1,024 distances at a time: the second fold at 1,024 | 1,025, the third at 2,048 | 2,049.
"""
import math

import numpy as np

import count_ladder as CL
from count_ladder import cdiv, edges

# ---------------------------------------------------------------- constants of the native code (name -> (value, file, pattern))

CONSTANTS = {
    "kInstGroup": (8, "icp_kernels.hpp", r"constexpr int kInstGroup = (\d+);"),
    "kInstManyBlock": (64, "kernels_geometry.hip", r"constexpr int kInstManyBlock = (\d+);"),
    "kInstManyU": (8, "kernels_geometry.hip", r"constexpr int kInstManyU = (\d+);"),
    "kProjGroup": (16, "icp_kernels.hpp", r"constexpr int kProjGroup = (\d+);"),
    "kProjMinSlabRows": (256, "icp_kernels.hpp", r"constexpr int kProjMinSlabRows = (\d+);"),
    "kProjMaxSlabs": (128, "icp_kernels.hpp", r"constexpr int kProjMaxSlabs = (\d+);"),
    "kProjResBlock": (128, "kernels_projection.hip", r"constexpr int kProjResBlock = (\d+);"),
    "kProjSteps": (4, "kernels_projection.hip", r"constexpr int kProjSteps = (\d+);"),
    "kProjMaxChunkItems": (32752, "abi_projection_many.inl", r"constexpr int kProjMaxChunkItems = (\d+);"),
    "ICP_POSTERIOR_MODELS_GROUP": (16, "../../include/icp_proposal.h", r"#define ICP_POSTERIOR_MODELS_GROUP (\d+)"),
    "kPmRowQuantum": (48, "abi_posterior_models.inl", r"constexpr int kPmRowQuantum = (\d+);"),
    "kPmRowTiles": (2, "kernels_posterior_model.hip", r"constexpr int kPmRowTiles = (\d+), kPmColTiles = \d+;"),
    "kPmColTiles": (4, "kernels_posterior_model.hip", r"constexpr int kPmRowTiles = \d+, kPmColTiles = (\d+);"),
    "kVarMaxRoundSamples": (32768, "abi_variability_many.inl", r"constexpr int kVarMaxRoundSamples = (\d+);"),
    "kVarBlock": (128, "kernels_variability.hip", r"constexpr int kVarBlock = (\d+);"),
    "kMetMaxChunk": (64, "abi_metrics_many.inl", r"constexpr int kMetMaxChunk = (\d+);"),
    "kMetDiceRange": (32768, "abi_metrics_many.inl", r"constexpr int kMetDiceRange = (\d+);"),
    "kMetHintElems": (1024, "abi_metrics_many.inl", r"constexpr int kMetHintElems = (\d+);"),
    "kDiceBlock": (256, "kernels_metrics.hip", r"constexpr int kDiceBlock = (\d+);"),
    "kEvalMaxChunk": (256, "abi_log_values_many.inl", r"constexpr int kEvalMaxChunk = (\d+);"),
    "kEvalHintElems": (1024, "abi_log_values_many.inl", r"constexpr int kEvalHintElems = (\d+);"),
    "kReduceBlock": (1024, "kernels_evaluate.hip", r"constexpr int kReduceBlock = (\d+);"),
    "kMapMaxChunk": (64, "abi_registration_maps.inl", r"constexpr int kMapMaxChunk = (\d+);"),
    "kMapBlock": (256, "kernels_maps.hip", r"constexpr int kMapBlock = (\d+);"),
    # the reductions' switch of block size, written as a literal in four places
    "stats switch, metrics plan (model side)": (4096, "abi_metrics_many.inl", r"if \(\(N > (\d+)\) == \(big == 1\)\)"),
    "stats switch, metrics plan (target side)": (4096, "abi_metrics_many.inl", r"if \(\(tg\.V > (\d+)\) == \(big == 1\)\)"),
    "stats switch, k_eval_reduce": (4096, "kernels_evaluate.hip", r"eval_stats\(j, j\.K > (\d+) \? 1024 : 256, s_red\)"),
    "stats switch, launch_dist_stats": (4096, "kernels_evaluate.hip", r"dim3\(K > (\d+) \? 1024 : kBlock\)"),
    "eval_gauss threads": (256, "kernels_evaluate.hip", r"eval_gauss\(j, (\d+), s_red\)"),
}
K_INST_GROUP, K_INST_BLOCK, K_INST_U = 8, 64, 8
K_PROJ_GROUP, K_PROJ_MIN_SLAB_ROWS, K_PROJ_MAX_SLABS, K_PROJ_RES_BLOCK, K_PROJ_STEPS, K_PROJ_MAX_CHUNK_ITEMS = 16, 256, 128, 128, 4, 32752
K_PM_GROUP, K_PM_ROW_QUANTUM, K_PM_ROW_TILES = 16, 48, 2
K_VAR_MAX_ROUND, K_VAR_BLOCK = 32768, 128
K_MET_MAX_CHUNK, K_MET_DICE_RANGE, K_HINT_ELEMS, K_DICE_BLOCK = 64, 32768, 1024, 256
K_EVAL_MAX_CHUNK, K_REDUCE_BLOCK, K_GAUSS_THREADS, K_STATS_SWITCH = 256, 1024, 256, 4096
K_MAP_MAX_CHUNK, K_MAP_BLOCK = 64, 256
K_SEARCH_BLOCK = CL.K_BLOCK   # kSearchBlock: k_met_spheres, k_met_normals, the small k_met_stats


# ---------------------------------------------------------------- the dispatch, restated

def proj_slab_rows(N):
    """kernels_projection.hip, proj_slab_rows"""
    rows = 3 * (N if N > 0 else 1)
    return cdiv(max(K_PROJ_MIN_SLAB_ROWS, cdiv(rows, K_PROJ_MAX_SLABS)), 16) * 16


def proj_slabs(N):
    """kernels_projection.hip, proj_slabs"""
    return cdiv(3 * (N if N > 0 else 1), proj_slab_rows(N))


def proj_last_trip(N):
    """kernels_projection.hip, k_proj_gemm: the last trip of the last slab's 16-row loop -> (steps with `k + 4u < k1`, quarter-waves
    with `ok[u]` in the last of them); the slab's rows are a multiple of 16, so both hang on 3N mod 16"""
    rem = (3 * N - 1) % (4 * K_PROJ_STEPS) + 1
    return cdiv(rem, 4), (rem - 1) % 4 + 1


def proj_trips(N):
    """k_proj_gemm: the 16-row loop of the first slab runs once / more than once"""
    return min(cdiv(min(3 * N, proj_slab_rows(N)), 4 * K_PROJ_STEPS), 2)


def pm_gemm_rows(N):
    """kernels_posterior_model.hip, k_pm_gemm on an item that is one piece: (32-row blocks, capped at 2; the second 16-row tile of the
    last block has a live row — `rok[1]`; the last tile is full)"""
    rows = 3 * N
    last = (rows - 1) % (16 * K_PM_ROW_TILES) + 1
    return min(cdiv(rows, 16 * K_PM_ROW_TILES), 2), last > 16, last % 16 == 0


def pm_point_variance_waves(N):
    """k_pm_point_variance: waves of the last workgroup of four vertices"""
    return (N - 1) % 4 + 1


def instance_rank_loops(r):
    """kernels_geometry.hip, k_instance_many: (the loop of kInstManyU columns runs, the loop of one runs)"""
    return r // K_INST_U > 0, r % K_INST_U > 0


def pm_mean_only_t0(r):
    """abi_posterior_models.inl, plan_group: the first column tile of a mean-only piece, and whether the mean's column r opens a
    tile of its own (r ≡ 0 mod 16) or closes the last tile of the basis (r ≡ 15)"""
    return r // 16, r % 16 == 0, r % 16 == 15


def inst_groups(n):
    """abi_many.inl, InstancePlan::add over n consecutive items of one model: (groups, capped at 2; the last group is full — no
    `g >= ng` padding lane)"""
    return min(cdiv(n, K_INST_GROUP), 2), n % K_INST_GROUP == 0


def proj_groups(n):
    """k_proj_residual / k_proj_gemm: (groups of 16 items, capped at 2; zero padding columns in the last)"""
    return min(cdiv(n, K_PROJ_GROUP), 2), n % K_PROJ_GROUP != 0


def pm_groups(n):
    """abi_posterior_models.inl: groups of kPmGroup items, capped at 3 — from the second on the r-space slots are taken over
    (`q % slots`) and `rec_used` has advanced; the third takes them over a second time"""
    return min(cdiv(n, K_PM_GROUP), 3)


def chunks_of(n, cap):
    return min(cdiv(n, cap), 2)


def var_plan(S, mode, N=3, cap=8 << 20, sweep=0):
    """abi_variability_many.inl: the segments of one map alone in a call -> (whole, [(s0, n, first, last)]) of the sums' sweep
    (sweep 0) or of the centred moments' (sweep 1).  A mode-1 map's reference mesh sits in the round of the FIRST segment of the
    sums' sweep only: the two sweeps of such a map may be cut differently."""
    n3 = 3 * N
    per, extra = (2 * n3 if mode == 2 else n3), (n3 if mode == 1 else 0)
    whole = extra + S * per <= cap and S + 1 <= K_VAR_MAX_ROUND
    if whole:
        return True, [(0, S, True, True)]
    used, held = (n3, 1) if mode == 1 and sweep == 0 else (0, 0)
    segs, s0 = [], 0
    while s0 < S:
        n = min(S - s0, (cap - used) // per, K_VAR_MAX_ROUND - held)
        if n > 0:
            segs.append((s0, n, s0 == 0, s0 + n == S))
            s0 += n
        used, held = 0, 0
    return False, segs


def var_shape(S, mode):
    """(whole, segments of the sums' sweep, of the centred sweep; capped at 2)"""
    whole, segs = var_plan(S, mode)
    return whole, min(len(segs), 2), min(len(var_plan(S, mode, sweep=1)[1]), 2)


def dice_ranges(S_d):
    """abi_metrics_many.inl: ranges of kMetDiceRange samples -> [(s0, n)]"""
    return [(s0, min(K_MET_DICE_RANGE, S_d - s0)) for s0 in range(0, S_d, K_MET_DICE_RANGE)]


def dice_round_ranges(n_items, S_d):
    """the Dice rounds of one chunk: ranges per round (the candidate budget aside) -> list of counts"""
    total = n_items * len(dice_ranges(S_d))
    return [min(2 * K_MET_MAX_CHUNK, total - k) for k in range(0, total, 2 * K_MET_MAX_CHUNK)]


def stats_shape(D):
    """k_met_stats / eval_stats / k_dist_stats: (threads, every thread has a distance, a thread has a second one)"""
    nt = 1024 if D > K_STATS_SWITCH else 256
    return nt, D >= nt, D > nt


def gauss_shape(D):
    """eval_gauss: 256 threads whatever D: (every thread has a term, a thread has a second one)"""
    return D >= K_GAUSS_THREADS, D > K_GAUSS_THREADS


def max_shape(D):
    """eval_max: (folds of 1,024, capped at 3; the last fold is full)"""
    return min(cdiv(D, K_REDUCE_BLOCK), 3), D % K_REDUCE_BLOCK == 0


def hint_step(n):
    """abi_metrics_many.inl / abi_log_values_many.inl / abi_registration_maps.inl: std::max(1, n / 1024)"""
    return max(1, n // K_HINT_ELEMS)


def summary_segments(S, chunk=K_MAP_MAX_CHUNK):
    """abi_registration_maps.inl, icp_distance_summaries_many: the segments of one set alone -> [(n, first, last)]"""
    return [(min(chunk, S - s0), s0 == 0, s0 + chunk >= S) for s0 in range(0, S, chunk)]


def summary_shape(S):
    segs = summary_segments(S)
    return min(len(segs), 3), any(not f and not l for _, f, l in segs)


N_DISPATCH = {  # name -> (decision(N), first N, last N looked at)
    "proj_slabs: one slab / several (kProjMinSlabRows)": (lambda N: min(proj_slabs(N), 2), 1, 600),
    "proj_slab_rows: 256 rows / more (kProjMaxSlabs)": (lambda N: proj_slab_rows(N) > K_PROJ_MIN_SLAB_ROWS, 10000, 11000),
    "k_proj_gemm: the 16-row loop runs once / again": (proj_trips, 1, 600),
    "k_pm_gemm: 32-row blocks, one / several": (lambda N: pm_gemm_rows(N)[0], 1, 600),
    "k_instance_many: cdiv(N, kInstManyBlock)": (lambda N: min(cdiv(N, K_INST_BLOCK), 2), 1, 600),
    "k_proj_residual, k_var_*: cdiv(N, 128)": (lambda N: min(cdiv(N, K_PROJ_RES_BLOCK), 2), 1, 600),
    "k_met_spheres / normals / box, k_map_rows, k_map_summaries: cdiv(N, 256)": (lambda N: min(cdiv(N, K_SEARCH_BLOCK), 2), 1, 600),
    "k_met_stats<256 | 1024> over the model's distances": (lambda N: stats_shape(N)[0], 4000, 4200),
}
N_PERIODIC = {  # name -> (decision(N), period)
    "k_proj_gemm: live steps and quarter-waves of the last trip (3N mod 16)": (proj_last_trip, 16),
    "k_pm_gemm: live rows of the last 32-row block (3N mod 32)": (lambda N: pm_gemm_rows(N)[1:], 32),
    "k_pm_point_variance: waves of the last workgroup (N mod 4)": (pm_point_variance_waves, 4),
}
ITEMS_DISPATCH = {
    "InstancePlan: groups of kInstGroup, a full last group": (inst_groups, 1, 9),
    "k_proj_gemm: groups of kProjGroup, padding columns": (proj_groups, 1, 17),
    "posterior models: groups of kPmGroup, slots taken over": (pm_groups, 1, 40),
    "metrics, maps: chunks of 64 items": (lambda n: chunks_of(n, K_MET_MAX_CHUNK), 1, 300),
    "log values: chunks of kEvalMaxChunk items": (lambda n: chunks_of(n, K_EVAL_MAX_CHUNK), 1, 300),
}
K_DISPATCH = {
    "k_pm_regression: regression_splits, kchunk, empty leaves": CL.K_DISPATCH["regression_splits, kchunk, empty leaves, kStepReduceSplits"],
}
S_DISPATCH = {
    "InstancePlan over a map's samples": (inst_groups, 2, 9),
    "variability, modes 0 and 2: whole / one segment twice / two segments": (lambda S: var_shape(S, 0), 32000, 33000),
    "variability, mode 2 (twice the doubles a sample)": (lambda S: var_shape(S, 2), 32000, 33000),
    "variability, mode 1: whole / two segments": (lambda S: var_shape(S, 1), 32000, 33000),
}
SD_DISPATCH = {
    "Dice skipped": (lambda S: S > 0, 0, 3),
    "k_met_samples, k_met_dice_count: cdiv(n, kDiceBlock)": (lambda S: min(cdiv(S, K_DICE_BLOCK), 2), 1, 600),
    "Dice ranges of kMetDiceRange, offset s0": (lambda S: min(len(dice_ranges(S)), 3), 1, 70000),
}
D_DISPATCH = {
    "k_met_stats, eval_stats, k_dist_stats": (stats_shape, 1, 4200),
    "eval_gauss at 256 threads": (gauss_shape, 1, 600),
    "eval_max: folds of 1,024": (max_shape, 1, 2100),
}
TV_DISPATCH = {
    "hint stride max(1, n / 1024)": (lambda n: min(hint_step(n), 2), 1, 2100),
}
SSUM_DISPATCH = {
    "summaries: segments of a set over chunks of kMapMaxChunk": (summary_shape, 1, 200),
}
DISPATCH = {"N": N_DISPATCH, "n": ITEMS_DISPATCH, "K": K_DISPATCH, "S": S_DISPATCH, "S_d": SD_DISPATCH, "D": D_DISPATCH, "TV": TV_DISPATCH,
            "S_sum": SSUM_DISPATCH}
BASE = {"N": (1, 2, 3), "n": (1, 2, 3), "K": (1,), "S": (2, 3), "S_d": (0, 1, 2, 3), "D": (1, 2, 3), "TV": (), "S_sum": (1, 2, 3)}


def derived_ladder(count):
    out = set(BASE[count])
    for fn, lo, hi in DISPATCH[count].values():
        for c in edges(fn, lo, hi):
            out.update((c, c + 1))
    if count == "N":
        out.update(range(1, 17))   # one period of the first periodic decision; the others' residues are shown covered by the CPU test
    return tuple(sorted(out))


def stands_for(count, c):
    return [f"{name} {e} | {e + 1}" for name, (fn, lo, hi) in DISPATCH[count].items() for e in edges(fn, lo, hi) if c in (e, e + 1)]


N_LADDER = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 64, 65, 85, 86, 128, 129, 256, 257, 4096, 4097, 10922, 10923)
ITEMS_LADDER = (1, 2, 3, 7, 8, 9, 15, 16, 17, 32, 33, 64, 65, 256, 257)
K_LADDER = CL.REGRESSION_KS
S_LADDER = (2, 3, 7, 8, 9, 32767, 32768, 32769)
SD_LADDER = (0, 1, 2, 3, 256, 257, 32768, 32769, 65536, 65537)
D_LADDER = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097)
TV_LADDER = (2047, 2048)
SSUM_LADDER = (1, 2, 3, 64, 65, 128, 129)
LADDERS = {"N": N_LADDER, "n": ITEMS_LADDER, "K": K_LADDER, "S": S_LADDER, "S_d": SD_LADDER, "D": D_LADDER, "TV": TV_LADDER, "S_sum": SSUM_LADDER}

# decisions on two counts: name -> (the fixed count N, decision(n), first n, last n), and the n on both sides of their edges
PAIR_DISPATCH = {
    "projection and instances: a chunk's item cap kProjMaxChunkItems (N = 1: 3 doubles a mesh)":
        (1, lambda n: min(cdiv(n, min(max(1, (4 << 20) // 3), K_PROJ_MAX_CHUNK_ITEMS)), 2), 32000, 33000),
}
PAIRS = ((1, 32752), (1, 32753))


def derived_pairs():
    return tuple((N, c) for N, fn, lo, hi in PAIR_DISPATCH.values() for e in edges(fn, lo, hi) for c in (e, e + 1))


RANKS = CL.RANKS                  # 12: one tile; 40: three tile rows
MEAN_ONLY_RANKS = (15, 16)        # r ≡ 15 and r ≡ 0 mod 16: pm_mean_only_t0
SMALL_N = tuple(N for N in N_LADDER if N <= 257)
PM_N = N_LADDER + (600,)   # posterior models: the whole N ladder; 600 carries the K ladder
# one N per decision at rank 40.  Posterior models: 40 observations of 65 vertices — at N = 17 (17 observations, 16 distinct vertices)
# no seed from 100 to 139 separates the 40 eigenvalues by 1.1e-5·μ_max, at N = 33 the first is 117
RANK40_N = {"instances": 65, "coefficients": 86, "posterior models": 65, "variability": 65}


# ---------------------------------------------------------------- meshes, models, states

def rank_of(N):
    return min(RANKS[0], 3 * N)


def ladder_mesh(N, closed=True):
    """N = 1, 2: count_ladder.tiny_mesh; 3: one triangle; 4..8: an open cut of the curved grid; from 9 on closed_mesh (closed=False:
    the open cut, whose rim is boundary)"""
    if N < 3:
        return CL.tiny_mesh(N)
    if N == 3:
        return CL.cut_mesh(T=1)
    if N < 9 or not closed:
        return CL.cut_mesh(V=N)
    return CL.closed_mesh(N)


def model_of(pkg, N, r=None, seed=41, closed=True):
    return CL.model_on(pkg, ladder_mesh(N, closed), rank_of(N) if r is None else r, seed)


def state(model, seed, pose=True, scale=0.5):
    """a chain state: coefficients of `scale`, and — pose — a translation of a few mm, a rotation of a few hundredths about the centroid"""
    rng = np.random.default_rng(seed)
    th = np.zeros(10 + model.rank)
    th[0] = 1.0
    th[7:10] = model.ref_points.sum(axis=0) / model.n_points
    th[10:] = np.clip(scale * rng.normal(size=model.rank), -2.0, 2.0)
    if pose:
        th[1:4] = 2.0 * rng.normal(size=3)
        th[4:7] = 0.03 * rng.normal(size=3)
    return th


def states(model, seed, n, pose=True, scale=0.5):
    return np.stack([state(model, seed + s, pose, scale) for s in range(n)])


def observation_set(model, K, seed, noise=0.5):
    """K observed vertices (with repeats once K exceeds N; one repeat otherwise, as test_gpu_posterior_models.observations) of a
    random instance plus noise, in model space"""
    rng = np.random.default_rng(seed)
    N = model.n_points
    ids = (rng.choice(N, size=K, replace=False) if K <= N else rng.integers(0, N, size=K)).astype(np.int32)
    if K > 1:
        ids[-1] = ids[0]
    inst = model.instance(0.7 * rng.normal(size=model.rank))
    return ids, inst[ids] + noise * rng.normal(size=(K, 3))


def spd_blocks(K, seed):
    """test_gpu_posterior_models.random_spd"""
    a = np.random.default_rng(seed).normal(size=(K, 3, 3))
    return np.einsum("kab,kcb->kac", a, a) + 0.05 * np.eye(3)


def pm_K(N):
    return min(N, 40)


# (N, rank) -> the seed of the posterior-model case's observation set: the first from 100 on whose decomposed matrix D⁻¹MD⁻¹ has a
# smallest gap of at least 1e-5·μ_max under both noise forms; derived and compared by the CPU test
PM_CASES = tuple((N, rank_of(N)) for N in PM_N) + ((RANK40_N["posterior models"], RANKS[1]), (33, 15), (33, 16), (600, RANKS[1]))


def pm_case_inputs(model, K, seed):
    ids, y = observation_set(model, K, seed)
    return ids, y, 0.1, spd_blocks(K, seed + 1000)


def pm_gap_and_cond(model, ids, y, sigma2, cov):
    """-> (smallest relative gap of D⁻¹MD⁻¹, cond(M)) of the long form, the worse of the two noise forms"""
    import posterior_long_form as LF
    import small_rank_ladder as SR
    gap, cond = 1.0, 0.0
    for kw in (dict(sigma2=sigma2), dict(covariances=cov)):
        M = LF.long_form(model, ids, y, **kw)["M"]
        gap, cond = min(gap, SR.smallest_relative_gap(SR.n_prime(model, M))), max(cond, float(np.linalg.cond(M)))
    return gap, cond


GAP = 1e-5                        # test_gpu_small_ranks.GAP
GAP_CHOSEN = 1.1e-5               # what a seed is chosen by, so that the condition does not hang on a last digit (small_rank_ladder)
COND_MAX = 1e-9 / 2.0 ** -52      # a solve loses cond(M)·2⁻⁵² of α: above this the 1e-9 of check_against_long_form cannot be asked


def derive_pm_seed(pkg, N, r, K=None):
    model = model_of(pkg, N, r)
    K = pm_K(N) if K is None else K
    for seed in range(100, 140):
        gap, cond = pm_gap_and_cond(model, *pm_case_inputs(model, K, seed))
        if gap >= GAP_CHOSEN and cond <= COND_MAX:
            return seed, gap, cond
    raise AssertionError((N, r))


PM_SEED = {**{case: 100 for case in PM_CASES}, (33, 16): 101}
PM_K_SEED = {(r, K): 100 for r in RANKS for K in K_LADDER}   # the K ladder at N = 600, both ranks


# ---------------------------------------------------------------- long forms that share no line with the library

def fsum_reference(d2, keep=None):
    """-> (Σ √d² by math.fsum, Σ |term|, the terms): the reductions' reference; keep: the flags of the boundary-aware sum"""
    t = np.sqrt(np.asarray(d2, dtype=np.float64))
    if keep is not None:
        t = t[np.asarray(keep, dtype=bool)]
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist()), t


def sum_bound(terms):
    """(D − 1)·2⁻⁵³·Σ|term|: what ANY order of D − 1 rounded additions of these terms may differ from the exact sum by, to first
    order (Higham, Accuracy and Stability of Numerical Algorithms, (4.4): |E| <= γ_{D−1}·Σ|x_i|, γ_k = k·u / (1 − k·u), u = 2⁻⁵³)"""
    t = np.asarray(terms, dtype=np.float64)
    return max(t.shape[0] - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(t).tolist())


def left_to_right(terms):
    s = 0.0
    for v in np.asarray(terms, dtype=np.float64).tolist():
        s = s + v
    return s


def gauss_logpdf_terms(d2, mean, sigma):
    """the terms −((√d² − mean) / σ)² / 2 − (log √(2π) + log σ) of eval_gauss, in numpy; σ >= 1: what gauss_bound rests on"""
    assert sigma >= 1.0
    d = (np.sqrt(np.asarray(d2, dtype=np.float64)) - mean) / sigma
    return -d * d / 2.0 - (math.log(math.sqrt(2.0 * math.pi)) + math.log(sigma))


GAUSS_TERM_ULPS = 4


def gauss_bound(terms):
    """sum_bound plus GAUSS_TERM_ULPS = 4 ulp of every term, for what the device's term and numpy's may differ by.  The term is
    −q − c with q = ((√d² − mean) / σ)² / 2 >= 0 and c = log √(2π) + log σ.  Given the same d², q has the same bits on both sides:
    the square root is correctly rounded on both, the subtraction, the division by σ, the square and the last subtraction are IEEE
    operations, the halving is exact.  Only c may differ: it is made of two calls of log, each within 1 ulp of the true logarithm on
    either side, so the two sides' values of each logarithm lie within 2 ulp of each other, and the two of them — both positive for
    σ > 1, so that an ulp of either is at most an ulp of their sum c — move c by at most 4 ulp of c; the addition that forms c and
    the subtraction that forms the term are rounded alike once their operands agree.  Since q >= 0 and c >= 0, |term| = q + c >= c,
    and 4 ulp of c are at most 4 ulp of the term.  This rests on c >= 0, i.e. σ >= 1 / √(2π) ≈ 0.399 (and on log σ >= 0, σ >= 1, for the
    step from the logarithms to their sum); the cases use σ = 2, and gauss_logpdf_terms refuses a σ below 1."""
    t = np.asarray(terms, dtype=np.float64)
    return sum_bound(t) + GAUSS_TERM_ULPS * 2.0 ** -52 * math.fsum(np.abs(t).tolist())


def variability_restatement(x, mode, normals=None):
    """k_variability's two loops in float64 numpy, in sample order with the kernel's expressions: x [S, N, 3] -> [N].  cumsum adds
    left to right from the first element (0.0 + x is x); every product and sum is rounded separately, as the library is built
    (-ffp-contract=off)."""
    S = x.shape[0]
    m = np.cumsum(x, axis=0)[-1] * (1.0 / S)
    inv_n1 = 1.0 / (S - 1)
    if mode == 0:
        v = x - m[None]
        c = np.cumsum(v * v, axis=0)[-1]
        return (c[:, 0] * inv_n1 + c[:, 1] * inv_n1) + c[:, 2] * inv_n1
    v = x - m[None]
    p = (normals[None, :, 0] * v[:, :, 0] + normals[None, :, 1] * v[:, :, 1]) + normals[None, :, 2] * v[:, :, 2]
    return np.cumsum(p * p, axis=0)[-1] * inv_n1


def _splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def dice_sample_points(lo, hi, s0, n, seed):
    """test_mesh_metrics_many_cpu.dice_samples for the samples s0 .. s0 + n − 1, vectorised in uint64 (the CPU test compares the two)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    step = np.arange(s0, s0 + n, dtype=np.uint64)[:, None]
    lane = np.arange(3, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        h = _splitmix64(_splitmix64(_splitmix64(np.uint64(seed)) ^ (step * np.uint64(0xD1342543DE82EF95))) ^ (lane * np.uint64(0x2545F4914F6CDD1D)))
    u = ((h >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    return lo + u * (hi - lo)


def dice_counts_by_range(oracle, x, nx, t_points, t_normals, S_d, seed):
    """Dice's counts (nA, nB, nAB) range by range, restated from oracle calls as test_gpu_mesh_metrics_many.cpu_dice_counts does
    for the whole set: x / nx the reconstruction's vertices and normals -> [(s0, n, nA, nB, nAB)]"""
    t_points = np.ascontiguousarray(t_points, dtype=np.float64)
    lo = np.minimum(x.min(axis=0), t_points.min(axis=0))
    hi = np.maximum(x.max(axis=0), t_points.max(axis=0))
    out = []
    for s0, n in dice_ranges(S_d):
        p = dice_sample_points(lo, hi, s0, n, seed)
        a, b = dice_inside_flags(oracle, p, x, nx), dice_inside_flags(oracle, p, t_points, t_normals)
        out.append((s0, n, int(a.sum()), int(b.sum()), int((a & b).sum())))
    return out


def dice_inside_flags(oracle, p, pts, nrm):
    """met_inside over the samples p: the nearest vertex, its normal, the stated dot product"""
    idx, _ = oracle.nearest_vertex(p, pts)
    v, nv = pts[idx], nrm[idx]
    return (nv[:, 0] * (v[:, 0] - p[:, 0]) + nv[:, 1] * (v[:, 1] - p[:, 1])) + nv[:, 2] * (v[:, 2] - p[:, 2]) > 0.0


# ---------------------------------------------------------------- the Dice scene

DICE_N, DICE_TARGET = 129, dict(N=257, R=41.0, r0=15.5)
# S_d -> the first seed from 1024 on with which every range of kMetDiceRange samples — the last one's single sample included — adds
# to nA, nB and nAB, and the set's FIRST sample is classified otherwise than that last one: a range that forgot its offset s0 would
# draw sample 0 again and must not count the same (derived and compared by the CPU test)
DICE_SEED = {32769: 1037, 65537: 1024}


def dice_seed_ok(case, S_d, seed):
    parts = case.by_range(S_d, seed)
    return all(min(p[2:]) >= 1 for p in parts) and case.by_range(1, seed)[0][2:] != parts[-1][2:]


class DiceCase:
    """a closed model of 129 vertices inside a closed target of 257 (both tori: count_ladder.closed_mesh), one state"""

    def __init__(self, pkg, oracle):
        from test_gpu_mesh_metrics_many import target_normals
        self.oracle = oracle
        self.model = model_of(pkg, DICE_N)
        self.target = CL.as_target(pkg, CL.closed_mesh(DICE_TARGET["N"], DICE_TARGET["R"], DICE_TARGET["r0"]))
        self.om = oracle.OracleModel.from_model(self.model)
        self.theta = state(self.model, 77)
        self.x = self.om.instance(self.theta)
        self.nx = self.om.vertex_normals(self.x)
        self.tn = target_normals(oracle, self.target.points, self.target.cells)
        self._memo = {}

    def by_range(self, S_d, seed):
        if (S_d, seed) not in self._memo:
            self._memo[(S_d, seed)] = dice_counts_by_range(self.oracle, self.x, self.nx, self.target.points, self.tn, S_d, seed)
        return self._memo[(S_d, seed)]


# ---------------------------------------------------------------- lists of posterior-model items over several models

def pm_item_list(models, n, seed, K_of=lambda m: min(m.n_points, 9), pick=None):
    """n items, item k on model pick[k] (k % len(models) without `pick`), the noise forms alternating
    -> [(model index, ids, y, sigma2 or None, covariances or None)]"""
    items = []
    for k in range(n):
        i = int(pick[k]) if pick is not None else k % len(models)
        ids, y = observation_set(models[i], K_of(models[i]), seed + k)
        iso = k % 2 == 0
        items.append((i, ids, y, 0.1 + 0.05 * (k % 5) if iso else None, None if iso else spd_blocks(ids.shape[0], seed + 500 + k)))
    return items


ITEMS_N, ITEMS_SEED, ITEMS_LONG_FORM = 7, 700, (15, 17, 31, 32)           # 33 items of one model: the items held to the long form
THREE_RANKS = ((16, None), (33, 15), (65, 40))                            # (N, rank) of the shuffled call's models
THREE_RANKS_SEED, THREE_RANKS_LONG_FORM = 800, (0, 15, 16)


def items_of_one_model(pkg):
    model = model_of(pkg, ITEMS_N)
    items = pm_item_list([model], 33, ITEMS_SEED)
    items[16], items[32] = items[0], items[0]
    return [model], items


def items_of_three_ranks(pkg):
    models = [model_of(pkg, N, r) for N, r in THREE_RANKS]
    pick = np.random.default_rng(5).permutation(17) % 3
    return models, pm_item_list(models, 17, THREE_RANKS_SEED, K_of=lambda m: min(m.n_points, 40), pick=pick)
