"""CPU: the ladders of tests/batched_count_ladder.py hold both sides of every edge of the restated dispatch of the batched entry
points, every restated constant is the number on the source line that defines it, and every designed input of
tests/test_gpu_batched_counts.py is sound before a GPU sees it — the posterior-model cases' condition and gap, the Dice restatement
range by range, the reductions' bound against a plain left-to-right sum — without a GPU."""
import math
import os
import re

import numpy as np
import pytest

import batched_count_ladder as BL
import count_ladder as CL
from conftest import ROOT
from test_mesh_metrics_many_cpu import dice_samples

CSRC = os.path.join(ROOT, "icp-proposal_amd", "csrc")


# ---------------------------------------------------------------- ladders

@pytest.mark.parametrize("count", list(BL.DISPATCH))
def test_ladder_holds_both_sides_of_every_edge(count):
    table, ladder = BL.DISPATCH[count], BL.LADDERS[count]
    assert ladder == tuple(sorted(set(ladder))) and set(BL.BASE[count]) <= set(ladder)
    for name, (fn, lo, hi) in table.items():
        es = CL.edges(fn, lo, hi)
        print(f"{count}: {name}: changes behind {es}")
        assert es, name  # (a decision without an edge does not belong in DISPATCH)
        for c in es:
            assert c in ladder and c + 1 in ladder, (name, c)
    if count == "K":   # REGRESSION_KS is count_ladder's: a superset of what k_pm_regression's edges ask for
        assert set(BL.derived_ladder("K")) <= set(ladder) and ladder == CL.REGRESSION_KS
    else:
        assert ladder == BL.derived_ladder(count)
        assert all(BL.stands_for(count, c) or c in BL.BASE[count] or (count == "N" and c <= 16) for c in ladder)


def test_periodic_decisions_take_every_value_on_the_ladder():
    for name, (fn, period) in BL.N_PERIODIC.items():
        every = {fn(N) for N in range(1, 20 * period)}
        assert {fn(N) for N in range(1, period + 1)} == every == {fn(N) for N in range(1 + period, 2 * period + 1)}, name
        on_ladder = {fn(N) for N in BL.SMALL_N}
        print(f"{name}: {len(every)} values, all on the ladder up to 257")
        assert on_ladder == every, name
    assert {BL.proj_last_trip(N) for N in range(1, 17)} == {(s, q) for s in (1, 2, 3, 4) for q in (1, 2, 3, 4)}
    # the ranks the cases run: both loops of k_instance_many, the mean-only pieces' first tile
    loops = {r: BL.instance_rank_loops(r) for r in (3, 6, 9, 12, 15, 16, 40)}
    assert loops[3] == (False, True) and loops[12] == (True, True) and loops[16] == loops[40] == (True, False)
    assert BL.pm_mean_only_t0(15) == (0, False, True) and BL.pm_mean_only_t0(16) == (1, True, False) and BL.pm_mean_only_t0(12)[0] == 0


def test_pairs_and_case_lists():
    assert BL.derived_pairs() == BL.PAIRS == ((1, 32752), (1, 32753))
    for name, (N, fn, lo, hi) in BL.PAIR_DISPATCH.items():
        assert CL.edges(fn, lo, hi), name
    assert 3 * 32753 < (4 << 20)          # the meshes of the pair fit the chunk buffer: the item cap alone closes the chunk
    assert BL.SMALL_N == tuple(N for N in BL.N_LADDER if N <= 257) and BL.PM_N[-1] == 600
    assert all(N in BL.N_LADDER for N in BL.RANK40_N.values()) and all(3 * N >= BL.RANKS[1] for N in BL.RANK40_N.values())


def test_restated_dispatch_gives_the_values_the_issue_and_the_code_document():
    assert [BL.proj_slabs(N) for N in (1, 85, 86, 1622, 10922, 10923, 28561)] == [1, 1, 2, 20, 128, 121, 128]
    assert [BL.proj_slab_rows(N) for N in (1, 10922, 10923, 28561)] == [256, 256, 272, 672]
    assert [BL.proj_last_trip(N) for N in (1, 5, 6, 16)] == [(1, 3), (4, 3), (1, 2), (4, 4)]
    assert [BL.inst_groups(n) for n in (7, 8, 9)] == [(1, False), (1, True), (2, False)]
    assert [BL.proj_groups(n) for n in (15, 16, 17)] == [(1, True), (1, False), (2, True)]
    assert [BL.pm_groups(n) for n in (12, 16, 17, 32, 33)] == [1, 1, 2, 2, 3]
    # variability: the issue's reading holds for modes 0 and 2; a mode-1 map of 32,768 samples is cut 32,767 + 1 in its sums' sweep
    assert BL.var_plan(32767, 0) == (True, [(0, 32767, True, True)])
    assert BL.var_plan(32768, 0) == BL.var_plan(32768, 2) == (False, [(0, 32768, True, True)])
    assert BL.var_plan(32769, 0) == (False, [(0, 32768, True, False), (32768, 1, False, True)])
    assert BL.var_plan(32768, 1) == (False, [(0, 32767, True, False), (32767, 1, False, True)])
    assert BL.var_plan(32768, 1, sweep=1) == (False, [(0, 32768, True, True)])
    assert 32769 * 18 < (8 << 20)          # at N = 3 the chunk buffer never cuts: kVarMaxRoundSamples alone does
    assert BL.dice_ranges(65537) == [(0, 32768), (32768, 32768), (65536, 1)] and BL.dice_ranges(0) == []
    assert BL.dice_round_ranges(64, 65537) == [128, 64] and BL.dice_round_ranges(64, 65536) == [128] and BL.dice_round_ranges(65, 32769)[0] == 128
    assert [BL.stats_shape(D) for D in (255, 256, 257, 4096, 4097)] == [(256, False, False), (256, True, False), (256, True, True),
                                                                       (256, True, True), (1024, True, True)]
    assert [BL.max_shape(D) for D in (1023, 1024, 1025, 2048, 2049)] == [(1, False), (1, True), (2, False), (2, True), (3, False)]
    assert [BL.hint_step(n) for n in (1, 2047, 2048, 58322)] == [1, 1, 2, 56]
    assert BL.summary_segments(65) == [(64, True, False), (1, False, True)]
    assert BL.summary_segments(129) == [(64, True, False), (64, False, False), (1, False, True)]
    assert BL.summary_shape(128) == (2, False) and BL.summary_shape(129) == (3, True)


def test_every_restated_constant_is_the_number_on_its_source_line():
    texts = {}
    for name, (value, path, pattern) in BL.CONSTANTS.items():
        full = os.path.normpath(os.path.join(CSRC, path))
        if full not in texts:
            with open(full) as f:
                texts[full] = f.read()
        found = re.findall(pattern, texts[full])
        assert len(found) == 1, (name, path, found)
        assert int(found[0]) == value, (name, found[0], value)
    c = {k: v[0] for k, v in BL.CONSTANTS.items()}
    assert (BL.K_INST_GROUP, BL.K_INST_BLOCK, BL.K_INST_U) == (c["kInstGroup"], c["kInstManyBlock"], c["kInstManyU"])
    assert (BL.K_PROJ_GROUP, BL.K_PROJ_MIN_SLAB_ROWS, BL.K_PROJ_MAX_SLABS) == (c["kProjGroup"], c["kProjMinSlabRows"], c["kProjMaxSlabs"])
    assert (BL.K_PROJ_RES_BLOCK, BL.K_PROJ_STEPS, BL.K_PROJ_MAX_CHUNK_ITEMS) == (c["kProjResBlock"], c["kProjSteps"], c["kProjMaxChunkItems"])
    assert (BL.K_PM_GROUP, BL.K_PM_ROW_QUANTUM, BL.K_PM_ROW_TILES) == (c["ICP_POSTERIOR_MODELS_GROUP"], c["kPmRowQuantum"], c["kPmRowTiles"])
    assert (BL.K_VAR_MAX_ROUND, BL.K_VAR_BLOCK) == (c["kVarMaxRoundSamples"], c["kVarBlock"])
    assert (BL.K_MET_MAX_CHUNK, BL.K_MET_DICE_RANGE, BL.K_DICE_BLOCK) == (c["kMetMaxChunk"], c["kMetDiceRange"], c["kDiceBlock"])
    assert BL.K_HINT_ELEMS == c["kMetHintElems"] == c["kEvalHintElems"]
    assert (BL.K_EVAL_MAX_CHUNK, BL.K_REDUCE_BLOCK, BL.K_GAUSS_THREADS) == (c["kEvalMaxChunk"], c["kReduceBlock"], c["eval_gauss threads"])
    assert (BL.K_MAP_MAX_CHUNK, BL.K_MAP_BLOCK) == (c["kMapMaxChunk"], c["kMapBlock"])
    assert all(c[k] == BL.K_STATS_SWITCH for k in c if k.startswith("stats switch"))
    assert BL.K_SEARCH_BLOCK == 256 and BL.K_VAR_BLOCK == BL.K_PROJ_RES_BLOCK == 128
    # the chunk buffers the plans above take as given
    assert re.search(r"kProjChunkDoubles = \(size_t\)4 << 20;", texts[os.path.join(CSRC, "abi_projection_many.inl")])
    assert re.search(r"kVarChunkDoubles = \(size_t\)8 << 20;", texts[os.path.join(CSRC, "abi_variability_many.inl")])
    assert re.search(r"k1 - k >= 2 \* \(size_t\)kMetMaxChunk", texts[os.path.join(CSRC, "abi_metrics_many.inl")])


# ---------------------------------------------------------------- meshes and models

def test_ladder_meshes_have_their_counts_and_models_their_ranks(pkg):
    for N in BL.SMALL_N + (600,):
        pts, cells = BL.ladder_mesh(N)
        assert pts.shape == (N, 3) and cells.min() >= 0 and cells.max() < N and cells.shape[0] >= 1, N
        if N >= 9:   # closed: every edge in exactly two triangles — mode 2 and Dice mean something
            e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]]), axis=1)
            assert (np.unique(e, axis=0, return_counts=True)[1] == 2).all(), N
        m = BL.model_of(pkg, N)
        assert m.rank == min(12, 3 * N) and m.n_points == N
    assert BL.ladder_mesh(3)[1].shape == (1, 3)
    for N in (129, 4096, 4097):
        pts, cells = BL.ladder_mesh(N, closed=False)
        e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]]), axis=1)
        assert pts.shape == (N, 3) and (np.unique(e, axis=0, return_counts=True)[1] == 1).any(), N   # a rim: boundary vertices


# ---------------------------------------------------------------- the posterior-model cases

def test_posterior_model_cases_are_well_conditioned_and_separated(pkg):
    """cond(M) of the long form within what a 1e-9 bar on α allows (1e-9 / 2⁻⁵²), the smallest gap of D⁻¹MD⁻¹ at least 1e-5·μ_max
    (§9.2), under both noise forms; the pinned seed is the first from 100 on that meets the gap with a tenth to spare"""
    worst = {"gap": 1.0, "cond": 0.0}
    for (N, r) in BL.PM_CASES:
        seed, gap, cond = BL.derive_pm_seed(pkg, N, r)
        print(f"N {N} rank {r} K {BL.pm_K(N)}: seed {seed} gap {gap:.2e} cond(M) {cond:.1e}")
        assert seed == BL.PM_SEED[(N, r)], (N, r, seed)
        assert gap >= BL.GAP and cond <= BL.COND_MAX
        worst["gap"], worst["cond"] = min(worst["gap"], gap), max(worst["cond"], cond)
    for r in BL.RANKS:
        for K in BL.K_LADDER:
            seed, gap, cond = BL.derive_pm_seed(pkg, 600, r, K)
            assert seed == BL.PM_K_SEED[(r, K)], (r, K, seed)
            assert gap >= BL.GAP and cond <= BL.COND_MAX
            worst["gap"], worst["cond"] = min(worst["gap"], gap), max(worst["cond"], cond)
    print(f"smallest gap {worst['gap']:.2e}, largest cond(M) {worst['cond']:.2e} (at most {BL.COND_MAX:.1e})")
    assert BL.COND_MAX == 1e-9 / 2.0 ** -52


def test_item_lists_are_well_conditioned_and_separated(pkg):
    """every item of the two lists that tests/test_gpu_batched_counts.py holds to the long form meets the same two conditions"""
    import posterior_long_form as LF
    import small_rank_ladder as SR
    for name, (models, items) in (("one model", BL.items_of_one_model(pkg)), ("three ranks", BL.items_of_three_ranks(pkg))):
        gaps, conds = [], []
        for i, ids, y, s2, cov in items:
            M = LF.long_form(models[i], ids, y, sigma2=s2, covariances=cov)["M"]
            gaps.append(SR.smallest_relative_gap(SR.n_prime(models[i], M)))
            conds.append(float(np.linalg.cond(M)))
        print(f"{name}: {len(items)} items, smallest gap {min(gaps):.2e}, largest cond(M) {max(conds):.1e}")
        assert min(gaps) >= BL.GAP and max(conds) <= BL.COND_MAX
    models, items = BL.items_of_one_model(pkg)
    assert all(np.array_equal(items[k][1], items[0][1]) and np.array_equal(items[k][2], items[0][2]) for k in (16, 32))
    models, items = BL.items_of_three_ranks(pkg)
    assert {models[it[0]].rank for it in items} == {12, 15, 40} and len(items) == 17


def test_observation_sets_repeat_a_vertex_and_stay_in_range(pkg):
    m = BL.model_of(pkg, 7)
    for K in (1, 7, 9):
        ids, y = BL.observation_set(m, K, 3)
        assert ids.shape == (K,) and y.shape == (K, 3) and ids.min() >= 0 and ids.max() < 7
        assert K == 1 or ids[-1] == ids[0]
    assert np.all(np.linalg.eigvalsh(BL.spd_blocks(9, 1)) > 0)


# ---------------------------------------------------------------- Dice

def test_dice_restatement_counts_in_every_range(pkg, oracle):
    """the vectorised sample points are test_mesh_metrics_many_cpu.dice_samples'; at S_d = 32,769 and 65,537 every range — the last
    one's single sample included, for these seeds — adds to nA, nB and nAB, and the ranges' counts add up to the whole set's"""
    lo, hi = np.array([-3.0, 1.0, 2.5]), np.array([4.0, 9.0, 2.75])
    assert np.array_equal(BL.dice_sample_points(lo, hi, 0, 300, 1024), dice_samples(lo, hi, 300, 1024))
    assert np.array_equal(BL.dice_sample_points(lo, hi, 32768, 2, 7), dice_samples(lo, hi, 32770, 7)[32768:])
    case = BL.DiceCase(pkg, oracle)
    for S_d in (32769, 65537):
        seed = BL.DICE_SEED[S_d]
        assert seed == next(s for s in range(1024, 1124) if BL.dice_seed_ok(case, S_d, s))   # the first that does
        parts = case.by_range(S_d, seed)
        print(S_d, seed, parts)
        assert [p[:2] for p in parts] == BL.dice_ranges(S_d) and len(parts) == (2 if S_d == 32769 else 3)
        assert all(min(p[2:]) >= 1 for p in parts)
        assert parts[-1][1:] == (1, 1, 1, 1)                    # the last range is one sample, inside both
        assert case.by_range(1, seed)[0][2:] != (1, 1, 1)       # … and sample 0 is not: a forgotten offset shows
    # the whole-set restatement of the existing module agrees where it is affordable
    from test_gpu_mesh_metrics_many import cpu_dice_counts
    parts = case.by_range(257, 1024)
    assert cpu_dice_counts(oracle, case.om, case.theta, case.target.points, case.tn, n=257, seed=1024) == tuple(sum(p[k] for p in parts) for k in (2, 3, 4))


# ---------------------------------------------------------------- the reductions' bound

@pytest.mark.parametrize("D", [4096, 4097])
def test_sum_bound_is_not_vacuous(D):
    """distances of the ladder's scale (a few mm): the fsum reference and a plain left-to-right sum differ, and by less than the
    bound — which is itself some 1e-13 of the sum: a wrong term of one part in 10¹² would show"""
    rng = np.random.default_rng(D)
    d2 = rng.uniform(0.0, 40.0, size=D) ** 2
    ref, mag, terms = BL.fsum_reference(d2)
    plain = BL.left_to_right(terms)
    bound = BL.sum_bound(terms)
    print(f"D {D}: |left to right - fsum| {abs(plain - ref):.3e}, bound {bound:.3e}, sum {ref:.6e}")
    assert 0.0 < abs(plain - ref) < bound
    assert bound == (D - 1) * 2.0 ** -53 * mag and bound < 1e-12 * ref
    assert abs(float(np.sum(terms)) - ref) < bound          # numpy's pairwise order too: the bound is the order-free one
    # dropped terms leave the bound of the kept ones
    keep = rng.random(D) > 0.25
    ref_k, _, kept = BL.fsum_reference(d2, keep)
    assert kept.shape[0] == keep.sum() and abs(BL.left_to_right(kept) - ref_k) < BL.sum_bound(kept)
    # the Gaussian terms: the bound grows by 4 ulp a term
    g = BL.gauss_logpdf_terms(d2, 0.0, 2.0)
    assert BL.gauss_bound(g) == BL.sum_bound(g) + 4 * 2.0 ** -52 * math.fsum(np.abs(g).tolist())
    assert abs(BL.left_to_right(g) - math.fsum(g.tolist())) < BL.sum_bound(g)


def test_variability_restatement_is_the_textbook_variance():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(9, 5, 3)) + 10.0
    v0 = BL.variability_restatement(x, 0)
    assert np.allclose(v0, x.var(axis=0, ddof=1).sum(axis=1), rtol=1e-13)
    n = rng.normal(size=(5, 3))
    v1 = BL.variability_restatement(x, 1, n)
    assert np.allclose(v1, (np.einsum("snd,nd->sn", x - x.mean(axis=0), n) ** 2).sum(axis=0) / 8.0, rtol=1e-12)
