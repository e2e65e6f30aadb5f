"""GPU: PCA shape models with Procrustes alignment (icp_pca_models_many, api.pca_models) against the numpy long form
(tests/pca_model_long_form.py) on a ladder of counts derived from the constants, the halt rule, the rank rule and an item that fails
alone, bits that depend on the item alone (batch, order, chunk buffer, shared pool), canaries, and a learned model that registers.

Inputs: instances of the bundled femur model (c ~ N(0, I)) restricted to the first N vertices, under seeded random rigid motions, with
0.1 mm of vertex noise where n exceeds the model's rank.  Every device result of the ladder comes from ONE pca_models call; the long
forms are made once per item and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pca_model_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52

# (n, N, seed).  3N at 255 | 258 around kGpmBlockRows = 256 (N = 85 | 86; 256 is no multiple of 3) and at 1,023 | 1,026 around
# gpm_slab_rows = 1,024 (N = 341 | 342); a piece boundary of kGpmRowQuantum = 48 rows (N = 96: 288 = 6·48, and N = 97); n = 2, 3, 16 | 17
# (the padding to 16), 64 | 65 (Jacobi route, then the tridiagonal one) and 256 (kGpmMaxPivots, at N = 86); the femur's own N with n = 40
LADDER = ((2, 85, 11), (3, 86, 12), (16, 341, 13), (17, 342, 14), (64, 96, 15), (65, 97, 16), (256, 86, 17), (40, 1622, 18))
FEMUR_RANK = 50


def femur(pkg):
    return pkg.data.load_femur_model(FEMUR_RANK)


@functools.lru_cache(maxsize=None)
def ladder_inputs():
    from conftest import load_package
    model = femur(load_package())
    return [LF.posed_instances(model, n, N, seed, noise=0.1 if n > FEMUR_RANK else 0.0) for n, N, seed in LADDER]


@functools.lru_cache(maxsize=None)
def ladder_long_forms():
    return [LF.long_form(m, iterations=3, halt_distance=0.0) for m in ladder_inputs()]


@functools.lru_cache(maxsize=None)
def ladder_device():
    from conftest import load_package
    return load_package().pca_models(ladder_inputs(), gpa_iterations=3, halt_distance=0.0)


def conditioning_bound(meshes, gap):
    """1e3·2⁻⁵²·max|coordinate|/gap: the project's margin (§5.13's orthogonality bound) over the rotation's conditioning, the gap being
    the relative gap between the two largest eigenvalues of Horn's matrix, from the long form"""
    return 1e3 * EPS * max(float(np.abs(m).max()) for m in meshes) / gap


@pytest.mark.gpu
@pytest.mark.parametrize("q", range(len(LADDER)))
def test_alignment_against_the_long_form(q):
    """transforms and mean shape within the conditioning bound; the device's error is printed beside the CPU spread of the two solvers"""
    (n, N, _), meshes, lf, (model, info) = LADDER[q], ladder_inputs()[q], ladder_long_forms()[q], ladder_device()[q]
    kabsch = LF.gpa(meshes, 3, 0.0, "kabsch")
    bound = conditioning_bound(meshes, lf["gap"])
    spread = max(np.abs(lf["mean"] - kabsch["mean"]).max(), np.abs(lf["transforms"] - kabsch["transforms"]).max())
    err = max(np.abs(info["mean"] - lf["mean"]).max(), np.abs(info["transforms"] - lf["transforms"]).max())
    print(f"n = {n}, N = {N}: gap {lf['gap']:.4f}, device error {err:.3e}, CPU spread of the two solvers {spread:.3e}, bound {bound:.3e}")
    assert info["status"] == 0 and info["n_meshes"] == n and info["rounds"] == lf["rounds"] == 3
    assert err <= bound
    assert abs(info["rms"] - lf["rms"][-1]) <= bound
    assert np.array_equal(model.ref_points, info["mean"]) and not model.mean_def.any()
    for tf in info["transforms"]:
        R = tf[:9].reshape(3, 3)
        assert abs(np.linalg.det(R) - 1.0) <= 1e-13 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("q", range(len(LADDER)))
def test_model_against_the_long_form(q):
    """test_gpu_gp_models.py's bounds: variances, orthonormality, rows of the covariance, the trace at full rank"""
    (n, N, _), lf, (model, info) = LADDER[q], ladder_long_forms()[q], ladder_device()[q]
    lam = lf["variance"]
    # (aligned to their mean shape, the meshes have lost the six rigid degrees of freedom: at n = 256, N = 86 the rank rule leaves 252)
    r = min(n - 1, 3 * N - 6)
    assert info["rank"] == lf["rank"] == r == model.rank and model.basis.shape == (3 * N, r)
    assert np.abs(info["variance"] - lam).max() <= 1e-10 * lam[0]
    assert np.all(np.diff(info["variance"]) <= 0.0) and np.array_equal(info["variance"], model.variance)
    B = model.basis
    orth = np.abs(B.T @ B / N - np.eye(r)).max()
    print(f"n = {n}, N = {N}: |BtB/N - I| {orth:.3e}, bound {1e3 * EPS * lam[0] / lam[-1]:.3e}; lambda_1 {lam[0]:.4e}, lambda_r {lam[-1]:.4e}")
    assert orth <= 1e3 * EPS * lam[0] / lam[-1]
    rows = sorted({0, 1, 3 * N // 2, 3 * N - 1})
    L = lf["L"]
    want = L[rows] @ L.T  # rows of L·Lᵀ of the long form's aligned data
    got = (B[rows] * info["variance"]) @ B.T
    assert np.abs(got - want).max() <= 1e-9 * float(np.sum(L * L, axis=1).max())  # (the largest entry of a covariance is on its diagonal)
    assert abs(info["total_variance"] - info["approximated_variance"]) <= 1e-12 * info["total_variance"]
    assert abs(info["total_variance"] - lf["trace"] / N) <= 1e-10 * lf["trace"] / N


@pytest.mark.gpu
def test_halt(pkg):
    """the rounds run equal the long form's: every RMS value of the long form misses the threshold by a factor >= 1.5 on either side"""
    meshes = LF.posed_instances(femur(pkg), 12, seed=3)
    halt = 1e-3
    full = LF.gpa(meshes, 8, 0.0)
    assert all(r >= 1.5 * halt or r <= halt / 1.5 for r in full["rms"])
    lf = LF.gpa(meshes, 8, halt)
    assert lf["rounds"] == 3
    res = pkg.pca_models([meshes] * 4, gpa_iterations=[8, 0, 1, 8], halt_distance=[halt, halt, halt, 0.0])
    (_, stopped), (_, none), (_, one), (_, never) = res
    print("long form rms", lf["rms"], "device rounds", [r[1]["rounds"] for r in res], "device rms", [r[1]["rms"] for r in res])
    bound = conditioning_bound(meshes, lf["gap"])
    assert stopped["rounds"] == lf["rounds"] and abs(stopped["rms"] - lf["rms"][-1]) <= bound
    assert np.abs(stopped["mean"] - lf["mean"]).max() <= bound and np.abs(stopped["transforms"] - lf["transforms"]).max() <= bound
    identity = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (12, 1))
    assert none["rounds"] == 0 and none["rms"] == 0.0 and np.array_equal(none["transforms"], identity)
    assert np.array_equal(none["mean"], LF.mean_in_order(meshes))
    assert one["rounds"] == 1 and abs(one["rms"] - full["rms"][0]) <= bound
    assert never["rounds"] == 8 and abs(never["rms"] - full["rms"][-1]) <= bound
    assert all(r[1]["status"] == 0 and r[1]["rank"] == 11 for r in res)


@pytest.mark.gpu
def test_rank_rule_and_an_item_that_fails_alone(pkg):
    meshes = LF.posed_instances(femur(pkg), 6, 341, seed=21)
    dup = meshes + [meshes[2]]
    same = [meshes[0]] * 5
    res = pkg.pca_models([dup, same, meshes, same], gpa_iterations=[3, 3, 3, 0])
    (m_dup, i_dup), (m_same, i_same), (m_ok, i_ok), (m_same0, i_same0) = res
    assert i_dup["status"] == 0 and i_dup["rank"] == 7 - 2 == m_dup.rank and LF.long_form(dup)["rank"] == 5
    for model, info in ((m_same, i_same), (m_same0, i_same0)):
        assert model is None and info["status"] == -3 and info["rank"] == 0
        assert all(np.all(np.isnan(info[k])) for k in ("variance", "mean", "transforms"))
    assert i_ok["status"] == 0 and i_ok["rank"] == 5
    alone = pkg.pca_model(meshes)
    assert same_bits(alone, (m_ok, i_ok))


# ---- bits

def same_bits(a, b):
    (ma, ia), (mb, ib) = a, b
    if (ma is None) != (mb is None) or set(ia) != set(ib):
        return False
    for k in ia:
        x, y = np.asarray(ia[k]), np.asarray(ib[k])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return ma is None or all(np.array_equal(getattr(ma, f), getattr(mb, f)) and getattr(ma, f).shape == getattr(mb, f).shape
                             for f in ("ref_points", "mean_def", "basis", "variance"))


MIXED = ((5, 85, 31), (17, 342, 32), (3, 1622, 33), (65, 97, 34), (12, 341, 35), (40, 200, 36), (2, 86, 37))


def mixed_inputs(pkg):
    model = femur(pkg)
    return [LF.posed_instances(model, n, N, seed, noise=0.1 if n > FEMUR_RANK else 0.0) for n, N, seed in MIXED]


def bits_check():
    """one item alone == the same item inside a call of 7 mixed items of different N and n == that call reversed == with the chunk
    buffer forced small (several rounds per item, rounds that hold several items): every array equal as bits.  Leave-one-out over a
    shared pool == n separate pca_model calls on copies."""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    os.environ.pop("ICP_TEST_GP_MODELS_CHUNK_DOUBLES", None)
    sets = mixed_inputs(pkg)
    its, halts = [3, 2, 8, 3, 0, 3, 1], [0.0, 0.0, 1e-3, 1e-5, 0.0, 1e-5, 0.0]
    run = lambda idx: pkg.pca_models([sets[i] for i in idx], gpa_iterations=[its[i] for i in idx], halt_distance=[halts[i] for i in idx])  # noqa: E731
    order = list(range(len(MIXED)))
    whole = run(order)
    assert all(info["status"] == 0 for _, info in whole) and not same_bits(whole[0], whole[6])
    for q in order:
        assert same_bits(run([q])[0], whole[q]), ("alone", q)
    assert all(same_bits(a, b) for a, b in zip(whole, run(order[::-1])[::-1])), "reversed"
    total = sum(3 * N * (n - 1) for n, N, _ in MIXED)
    for doubles in (total // 9, 48 * 64):  # a ninth of the call's bases; the smallest buffer the item of most columns (64) allows
        os.environ["ICP_TEST_GP_MODELS_CHUNK_DOUBLES"] = str(doubles)
        assert all(same_bits(a, b) for a, b in zip(whole, run(order))), doubles
    os.environ.pop("ICP_TEST_GP_MODELS_CHUNK_DOUBLES", None)
    meshes = LF.posed_instances(femur(pkg), 7, 342, seed=41)
    loo = pkg.leave_one_out_pca_models(meshes)
    for i in range(7):
        copies = [m.copy() for j, m in enumerate(meshes) if j != i]
        assert same_bits(pkg.pca_model(copies), loo[i]), ("leave-one-out", i)
    print("bits check ok")


@pytest.mark.gpu
def test_an_items_bits_do_not_depend_on_the_batch_the_chunk_or_the_pool():
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "bits check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


# ---- canaries

@pytest.mark.gpu
def test_canaries_behind_every_output_array(pkg):
    """straight through ctypes: two items over one pool, every output array with a canary tail that must come back intact"""
    nat, lib = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    meshes = LF.posed_instances(femur(pkg), 6, 97, seed=51)
    N, TAIL, CANARY = 97, 64, -7.0
    ids = [np.array([0, 1, 2, 3, 4, 5], dtype=np.int32), np.array([5, 3, 1], dtype=np.int32)]
    ranks = np.array([4, 2], dtype=np.int32)
    sizes = {"variance": lambda n, r: r, "basis": lambda n, r: 3 * N * r, "mean": lambda n, r: 3 * N, "transforms": lambda n, r: 12 * n,
             "info": lambda n, r: 8}
    outs = {k: [np.full(f(len(ids[b]), int(ranks[b])) + TAIL, CANARY) for b in range(2)] for k, f in sizes.items()}
    ptrs = lambda arrays, t: (t * len(arrays))(*[a.ctypes.data_as(t) for a in arrays])  # noqa: E731
    pp, nm = np.full(6, N, dtype=np.int32), np.array([6, 3], dtype=np.int32)
    it, hd, st = np.array([3, 2], dtype=np.int32), np.zeros(2), np.full(2, 99, dtype=np.int32)
    rc = lib.icp_pca_models_many(2, 0, 6, pp.ctypes.data_as(ip), ptrs(meshes, dp), nm.ctypes.data_as(ip), ptrs(ids, ip), None,
                                 ranks.ctypes.data_as(ip), it.ctypes.data_as(ip), hd.ctypes.data_as(dp), ptrs(outs["variance"], dp),
                                 ptrs(outs["basis"], dp), ptrs(outs["mean"], dp), ptrs(outs["transforms"], dp), ptrs(outs["info"], dp),
                                 st.ctypes.data_as(ip))
    assert rc == 0 and list(st) == [0, 0]
    for k, arrays in outs.items():
        for b, a in enumerate(arrays):
            assert np.all(a[-TAIL:] == CANARY) and np.all(np.isfinite(a[:-TAIL])) and not np.any(a[:-TAIL] == CANARY), (k, b)
    assert outs["info"][0][0] == 6 and outs["info"][1][0] == 3 and outs["info"][0][1] == 4 and outs["info"][1][1] == 2
    # the Python surface returns these bits; item 0 has rank < n − 1: the leading eigenpairs
    for b, (rounds, rank) in enumerate(((3, 4), (2, 2))):
        model, info = pkg.pca_model([meshes[k] for k in ids[b]], rank=rank, gpa_iterations=rounds, halt_distance=0.0)
        assert np.array_equal(info["variance"], outs["variance"][b][:rank])
        assert np.array_equal(model.basis, outs["basis"][b][:-TAIL].reshape(3 * N, rank))


# ---- the model registers

@pytest.mark.gpu
def test_a_leave_one_out_model_registers(pkg):
    """leave-one-out models of 20 femur instances: each builds an IcpContext, the left-out mesh projects into it
    (model_coefficients(want_project=True)) with coefficients within test_gpu_model_projection.py's bound of the numpy solve, the
    generalisation error is finite and below the distance to the mean shape, and a 3-iteration icp_fits runs on it"""
    base = femur(pkg)
    meshes = LF.posed_instances(base, 20, seed=61)
    loo = pkg.leave_one_out_pca_models(meshes, cells=base.cells)
    assert len(loo) == 20 and all(info["status"] == 0 and info["rank"] == 18 and m.n_points == 1622 for m, info in loo)
    for i in (0, 7, 19):
        model, info = loo[i]
        R, t, cx, cy, _ = LF.rigid(meshes[i], info["mean"])  # the left-out mesh into the model's frame
        x = (meshes[i] - cx) @ R.T + cy
        ctx = pkg.IcpContext(model, pkg.data.TriangleMesh(x, base.cells), device=0)
        coeffs, proj = pkg.model_coefficients(ctx, meshes=[x], want_project=True)
        Q = model.basis * np.sqrt(model.variance)[None, :]
        want = np.linalg.solve(Q.T @ Q + 1e-5 * np.eye(model.rank), Q.T @ (x - model.ref_points - model.mean_def).reshape(-1))
        assert np.abs(coeffs[0] - want).max() <= 1e-10 * max(1.0, float(np.abs(want).max()))
        gen = float(np.mean(np.linalg.norm(proj[0] - x, axis=1)))
        to_mean = float(np.mean(np.linalg.norm(info["mean"] - x, axis=1)))
        print(f"left out {i}: generalisation error {gen:.3f} mm, distance to the mean shape {to_mean:.3f} mm")
        assert np.isfinite(gen) and gen < to_mean
        thetas, status = pkg.icp_fits(ctx, pkg.initial_parameters(model)[None, :], 3, modelPointIds=np.arange(0, 1622, 8))
        assert status[0] == 0 and np.all(np.isfinite(thetas))
        ctx.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    bits_check()
