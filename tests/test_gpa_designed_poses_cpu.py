"""CPU: the cases of tests/gpa_designed_poses.py are what they claim — what tests/test_gpu_gpa_poses.py feeds the alignment half of
icp_pca_models_many is pinned here, without a GPU.  Conditions on the INPUTS, met by the numpy long form alone; none is a tolerance
for the device.

1. Solver spread: every case whose transforms the GPU test compares with the long form's has a CPU spread of the two rigid solvers (Horn
   by eigh against Kabsch by SVD, over mean shape and transforms) of at most 1/8 of the conditioning bound 1e3·2⁻⁵²·max|coordinate|/gap.
   A case that misses goes to gpa_designed_poses.MISS_THE_SOLVER_SPREAD (invariants only), never to a looser bound.  None does: the
   largest shares are 1.8e-2 (tiny N = 5, n = 256), 6.1e-3 (the 32-round item) and 2.5e-3 (shifts of 1e5); the nearly collinear set,
   gap 1.8e-7, uses 1.8e-4 of its (large) bound.
2. Rank margins: the long form's rank is the prediction, θ_rank >= 64·τ and τ >= 64·max|θ behind the rank|; an N = 1 item keeps nothing.
3. Halt margin: the probes' thresholds miss every RMS value of the long form's sequence by a factor >= 1.5.
4. Block counts: the edge items have 256 | 257 row blocks and 256 | 257 vertex blocks, as derived from kPcaBlock."""
import numpy as np
import pytest

import gpa_designed_poses as GP
import pca_model_long_form as LF

CASES = GP.cases()
IDS = [c["name"] for c in CASES]


def compared_with_the_long_forms_transforms(c):
    return c["group"] != "twin" and c["rank"] > 0 and not GP.invariants_only(c)


def test_the_case_list():
    names = set(IDS)
    assert len(names) == len(CASES)
    B = GP.BLOCK
    assert GP.EDGE_N == (B * B // 3, B * B // 3 + 1, B * B, B * B + 1)
    for N in GP.EDGE_N:
        for n in GP.EDGE_MESHES:
            rounds = (1, 3) if max(GP.blocks(N)) > B else (3,)
            assert all(f"edge N={N} n={n} rounds={r}" in names for r in rounds)
    assert f"edge N={GP.EDGE_N[1]} n=2 halt" in names
    assert sum(c["group"] == "tiny" for c in CASES) == 25 and all(c["iterations"] == 8 for c in CASES if c["group"] == "tiny")
    assert any(c["iterations"] == GP.MAX_ROUNDS == 32 for c in CASES)
    assert sum(c["group"] == "twin" for c in CASES) == 4
    other_n = {"pose nearly collinear": GP.LINE_N, "pose " + GP.EXACT: GP.BLOCK}
    assert all(c["N"] == other_n.get(c["name"], GP.POSE_N) and c["n"] == GP.POSE_MESHES for c in CASES if c["group"] == "pose")
    assert all(not GP.invariants_only(c) or c["N"] == 2 or c["name"] in GP.MISS_THE_SOLVER_SPREAD for c in CASES)
    assert set(GP.MISS_THE_SOLVER_SPREAD) <= names


def test_block_counts_of_the_edge_items():
    B = GP.BLOCK
    assert max(GP.blocks(GP.EDGE_N[1])[0], GP.blocks(GP.EDGE_N[0])[0]) < B  # (the row edge crosses nothing over vertices)
    assert GP.blocks(GP.EDGE_N[0])[1] == B and GP.blocks(GP.EDGE_N[1])[1] == B + 1
    assert GP.blocks(GP.EDGE_N[2])[0] == B and GP.blocks(GP.EDGE_N[3])[0] == B + 1
    assert GP.EDGE_N[3] - B * B == 1  # the last vertex block holds one vertex …
    for c in CASES:
        if c["group"] == "edge" and c["N"] == GP.EDGE_N[3]:  # … the outlier, far outside the cloud in every mesh
            radius = max(np.linalg.norm(m[:-1] - m[:-1].mean(axis=0), axis=1).max() for m in c["meshes"])
            assert all(np.linalg.norm(m[-1] - m[:-1].mean(axis=0)) > 1.5 * radius for m in c["meshes"])
            assert all(np.linalg.norm(m[-1] - m[:-1].mean(axis=0)) > 9.0 * GP.AXES[0] for m in c["meshes"])
        elif c["group"] == "pose":
            assert GP.blocks(c["N"])[0] == (1 if c["N"] in (GP.LINE_N, GP.BLOCK) else 2)


@pytest.mark.parametrize("q", range(len(CASES)), ids=IDS)
def test_solver_spread(q):
    c, lf, kabsch = CASES[q], GP.long_forms()[q], GP.kabsch_forms()[q]
    assert lf["rounds"] == kabsch["rounds"] == c.get("stops", c["iterations"])
    if not compared_with_the_long_forms_transforms(c):
        # the aligned positions are unique where R is not: the two solvers' mean shapes agree without a gap in the bound
        if c["rank"] > 0 and c["group"] != "twin":
            assert np.abs(lf["mean"] - kabsch["mean"]).max() <= GP.data_bound(c["meshes"]) / 8.0
        return
    bound = GP.conditioning_bound(c["meshes"], lf["gap"])
    spread = GP.solver_spread(lf, kabsch)
    print(f"{c['name']}: gap {lf['gap']:.3e}, CPU spread {spread:.3e}, bound {bound:.3e}, share {spread / bound:.2e}")
    assert lf["gap"] > 0.0 and spread <= bound / 8.0
    assert GP.consistency(c["meshes"], lf) <= GP.data_bound(c["meshes"]) / 8.0


@pytest.mark.parametrize("q", range(len(CASES)), ids=IDS)
def test_rank_margins(q):
    c, lf = CASES[q], GP.long_forms()[q]
    theta, r, tau = lf["theta"], lf["rank"], lf["tau"]
    assert r == c["rank"] == GP.predicted_rank(c["n"], c["N"])
    if c["N"] == 1:
        assert r == 0 and lf["trace"] <= lf["tau0"]  # what the host reads at its synchronisation: the item fails alone
        return
    assert lf["trace"] > lf["tau0"] and r >= 1
    behind = float(np.abs(theta[r:]).max())
    print(f"{c['name']}: rank {r}, theta_rank/tau {theta[r - 1] / tau:.2e}, tau/max|theta behind| {tau / behind if behind else np.inf:.2e}")
    assert theta[r - 1] >= 64.0 * tau and tau >= 64.0 * behind


def test_halt_margins():
    probes = [c for c in CASES if "stops" in c and c["group"] != "twin"]
    assert len(probes) == 2 and probes[0]["N"] == GP.EDGE_N[1] and probes[0]["n"] == 2
    for c in probes:
        rms = LF.gpa(c["meshes"], c["iterations"], 0.0)["rms"]
        print(c["name"], "halt", c["halt"], "stops behind round", c["stops"], "rms", rms)
        assert len(rms) == c["iterations"] == 8 and 2 <= c["stops"] < 8
        assert all(v >= 1.5 * c["halt"] or v <= c["halt"] / 1.5 for v in rms)
        assert rms[c["stops"] - 2] >= 1.5 * c["halt"] and rms[c["stops"] - 1] <= c["halt"] / 1.5
        assert LF.gpa(c["meshes"], c["iterations"], c["halt"])["rounds"] == c["stops"]


def test_twins_are_exact_multiples():
    for c in CASES:
        if c["group"] != "twin":
            continue
        base = next(b for b in CASES if b["name"] == c["of"])
        s = c["scale"]
        assert s in GP.TWIN_SCALES and np.log2(s) in (-40.0, 40.0) and c["halt"] == base["halt"] * s and c["iterations"] == base["iterations"]
        assert all(np.array_equal(m / s, b) for m, b in zip(c["meshes"], base["meshes"]))  # (a power of two: no bit of a mantissa moves)
    assert {c["of"] for c in CASES if c["group"] == "twin"} == set(GP.TWINS_OF)
    assert any(b["halt"] > 0.0 for b in CASES if b["name"] in GP.TWINS_OF)


def test_the_poses_are_what_they_say():
    by = {c["name"]: c for c in CASES}
    for a in range(3):
        for q in (1, 2):
            T = GP.turn(a, q)
            assert np.array_equal(np.abs(T).sum(axis=0), np.ones(3)) and set(T.ravel()) <= {-1.0, 0.0, 1.0} and np.linalg.det(T) == 1.0
            assert np.array_equal(np.linalg.matrix_power(T, 4 // q), np.eye(3)) and T[a, a] == 1.0
    assert all(np.all(m[:, 2] == 0.0) for m in GP.deformed(GP.cloud(GP.POSE_N, 300) * np.array([1.0, 1.0, 0.0]), 2, np.random.default_rng(0), planar=True))
    for name in ("pose planar", "pose planar, one mirrored in the plane"):  # planar in 3-space: the smallest singular value is rounding
        assert all(np.linalg.svd(m - m.mean(axis=0), compute_uv=False)[2] <= 1e-12 for m in by[name]["meshes"])
    # the mirror-symmetric sets: vertex t + o is the mirror image of vertex t in y | z | x for o = B/2 | B/4 | B/8, in every mesh and so in
    # the mean shape; in numpy the cross-covariance with the mean shape is diagonal up to rounding and the fit is the exact half turn
    B, meshes = GP.BLOCK, by["pose " + GP.EXACT]["meshes"]
    for m in meshes + [LF.mean_in_order(meshes)]:
        for o, axis in ((B // 2, 1), (B // 4, 2), (B // 8, 0)):
            t = np.array([t for t in range(B) if t % (2 * o) < o])
            assert np.array_equal(m[t + o], m[t] * np.where(np.arange(3) == axis, -1.0, 1.0))
    for j, want in enumerate([np.eye(3)] * 3 + [GP.turn(a, 2) for a in range(3)]):
        S, cx, cy = LF.cross_covariance(meshes[j], LF.mean_in_order(meshes))
        assert np.abs(S - np.diag(np.diag(S))).max() <= 1e-12 * np.abs(S).max() and max(np.abs(cx).max(), np.abs(cy).max()) <= 1e-13
        assert np.abs(LF.rotation_horn(S)[0] - want).max() <= 1e-13 and np.array_equal(np.sign(np.diag(S)), np.diag(want))
    sv = [np.linalg.svd(m - m.mean(axis=0), compute_uv=False) for m in by["pose nearly collinear"]["meshes"]]
    assert all(s[1] <= 1e-2 * s[0] and s[2] >= 1e-4 * s[0] for s in sv) and by["pose nearly collinear"]["N"] == GP.LINE_N
    assert min(abs(m.mean(axis=0)).max() for m in by["pose shifts of 1e5"]["meshes"]) > 1e4
    # a mirrored mesh: the unconstrained orthogonal fit to the others' mean is a reflection; Horn's (and Kabsch's) stays proper
    meshes = by["pose one mesh mirrored"]["meshes"]
    S, _, _ = LF.cross_covariance(meshes[2], LF.mean_in_order(meshes[:2] + meshes[3:]))
    assert np.linalg.det(S) < 0.0 < np.linalg.det(LF.cross_covariance(meshes[1], LF.mean_in_order(meshes[:1] + meshes[2:]))[0])
    for lf in GP.long_forms():
        for tf in lf["transforms"]:
            R = tf[:9].reshape(3, 3)
            assert abs(np.linalg.det(R) - 1.0) <= 1e-13 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-13
