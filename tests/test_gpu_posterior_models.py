"""GPU: posterior shape models from given correspondences (icp_posterior_models_many) through the public interface — against the numpy
long form (tests/posterior_long_form.py), against the chain's own posterior of the same correspondences, landmarks end to end (the
conditioned model makes a context and runs a chain that matches the oracle), batch / order / chunk invariance, device memory bounded
from the header's sizes, argument errors.  Tolerances are DESIGN.md §9's: 1e-9 for M, α, S and what is linear in them, 1e-7 for
anything that carries V, each relative to max(1, max|·|) of the compared quantity."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import posterior_long_form as LF
from conftest import ROOT, make_theta

pytestmark = pytest.mark.gpu

# include/icp_proposal.h
CHUNK_BYTES = 32 << 20   # ICP_POSTERIOR_MODELS_CHUNK_BYTES
GROUP = 16               # ICP_POSTERIOR_MODELS_GROUP


def slot_bytes(r, s):
    """ICP_POSTERIOR_MODELS_SLOT_BYTES(r, s)"""
    return 8 * (s * (r + 1) * (r + 1) + 50 * (r + 17) * (r + 17) + 4096)


def rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, float(np.abs(want).max())))


def hip_runtime():
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) >= 1
    return ctypes.CDLL(sorted(paths)[0])


def free_bytes(hip):
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def observations(model, n_obs, seed, noise=0.5):
    """a seeded sample of vertex ids (with one repeat) observed on a random instance of the model plus noise, in model space"""
    rng = np.random.default_rng(seed)
    ids = rng.choice(model.n_points, size=n_obs, replace=False).astype(np.int32)
    ids[-1] = ids[0]
    c = 0.7 * rng.normal(size=model.rank)
    inst = model.ref_points + model.mean_def + ((model.basis * np.sqrt(model.variance)) @ c).reshape(-1, 3)
    return ids, inst[ids] + noise * rng.normal(size=(n_obs, 3))


def random_spd(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 3, 3))
    return np.einsum("kab,kcb->kac", a, a) + 0.05 * np.eye(3)


def check_against_long_form(model, res, ids, y, sigma2, cov, tag):
    lf = LF.long_form(model, ids, y, sigma2=sigma2, covariances=cov)
    rng = np.random.default_rng(99)
    a, b = rng.integers(0, model.n_points, size=256), rng.integers(0, model.n_points, size=256)
    want_blocks = LF.covariance_blocks(lf["Q"], lf["Minv"], a, b)
    figures = {
        "alpha": (rel(res["alpha"], lf["alpha"]), 1e-9),
        "S": (rel(res["variance"], lf["S"]), 1e-9),
        "mean": (rel(res["mean"], lf["mean"]), 1e-9),
        "cov": (rel(LF.model_blocks(res["basis"], res["variance"], a, b), want_blocks), 1e-7),
        "point_variance": (rel(res["point_variance"], LF.point_variances(lf["Q"], lf["Minv"])), 1e-9),
    }
    print(tag, {k: f"{v[0]:.2e}" for k, v in figures.items()})
    assert res["status"] == 0
    assert np.all(np.diff(res["variance"]) <= 0), tag
    for k, (err, tol) in figures.items():
        assert err <= tol, (tag, k, err)
    return figures


# ---------------------------------------------------------------- 1. the long form

SIGMAS = (1.0, 0.1, 0.01)  # IcpBasedSurfaceFitting's own sequence


@pytest.mark.parametrize("n_comp", [50, 100, 200])
def test_femur_against_the_long_form(pkg, n_comp):
    model, target = pkg.data.load_femur_model_and_target(n_comp)
    ctx = pkg.IcpContext(model, target, device=0)
    ids, y = observations(model, 200, 10 + n_comp)
    cov = random_spd(200, 20 + n_comp)
    res = pkg.posterior_models(ctx, [ids] * 4, [y] * 4, sigma2=[*SIGMAS, None], covariances=[None, None, None, cov])
    for k, s2 in enumerate(SIGMAS):
        check_against_long_form(model, res[k], ids, y, s2, None, f"femur-{n_comp} sigma2={s2}")
    check_against_long_form(model, res[3], ids, y, None, cov, f"femur-{n_comp} 3x3")
    assert all(v == 0 for v in pkg._native.runtime_stats(ctx.h).values())
    ctx.close()


@pytest.fixture(scope="module")
def face(pkg):
    model = pkg.data.synthetic_face_model(grid=169, rank=200)
    target = pkg.data.synthetic_partial_target(model)
    ctx = pkg.IcpContext(model, target, device=0)
    yield model, ctx
    ctx.close()


def test_face_against_the_long_form_within_the_memory_bound(pkg, face):
    """N = 28,561, rank 200, four items (the three isotropic noises and random 3 × 3 covariances), 137 MB of basis each.  Device memory
    the call may take, from the header: the chunk buffer, one r-space slot per item, the inputs and per-item results, and 2 MiB of
    allocator granularity for each of the call's 16 buffers — far below the 548 MB the four bases take on the host."""
    model, ctx = face
    N, r, n_obs = model.n_points, model.rank, 600
    ids, y = observations(model, n_obs, 77)
    cov = random_spd(n_obs, 78)
    ctx.transformedMesh(pkg.initial_parameters(model))
    hip = hip_runtime()
    free0 = free_bytes(hip)
    res = pkg.posterior_models(ctx, [ids] * 4, [y] * 4, sigma2=[*SIGMAS, None], covariances=[None, None, None, cov])
    free1 = free_bytes(hip)
    s = min(64, -(-n_obs // 8))
    bound = CHUNK_BYTES + min(4, GROUP) * slot_bytes(r, s) + 4 * n_obs * (4 + 24 + 48) + 4 * (16 * r + 16) + 16 * (2 << 20)
    print(f"device memory taken by the call: {(free0 - free1) / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB; the bases: {4 * 3 * N * r * 8 / 2**20:.0f} MiB")
    assert free0 - free1 <= bound
    assert bound < 4 * 3 * N * r * 8 / 2
    for k, s2 in enumerate(SIGMAS):
        check_against_long_form(model, res[k], ids, y, s2, None, f"face sigma2={s2}")
    check_against_long_form(model, res[3], ids, y, None, cov, "face 3x3")
    assert all(v == 0 for v in pkg._native.runtime_stats(ctx.h).values())


# ---------------------------------------------------------------- 2. the chain's own posterior

@pytest.mark.parametrize("direction", ["ModelSampling", "TargetSampling"])
def test_same_posterior_as_the_chains(pkg, femur50, direction):
    """The kept correspondences of icp_proposal_posterior at a seeded state, handed in with the covariances of the SurfaceNoiseHelpers rule
    (σ_n² n̂n̂ᵀ + σ_t² (I − n̂n̂ᵀ), n̂ the vertex normal of the state's mesh) and the observations taken off the pose as the proposal
    takes them: α and S are the view's within 1e-9, Φ·V is Φ·view.V within 1e-7."""
    model, target = femur50
    ctx = pkg.IcpContext(model, target, device=0)
    r = model.rank
    sigma_t, sigma_n = 10.0, 5.0
    theta = make_theta(model, 31)
    theta[4:7] = 0.0  # (a translation and a shape; the rotation stays out of the test's own arithmetic)
    tp = pkg.data.decimated_point_subset(target, 2 * r)
    prop = pkg.NonRigidIcpProposal(ctx, 0.1, sigma_t, sigma_n, 2 * r, getattr(pkg, direction), True, decimatedTargetPoints=tp)
    view = prop.icpPosterior(theta)
    keep = view.keep[:prop.K].astype(bool)
    ids = view.corr_id[:prop.K][keep]
    assert ids.shape[0] > r // 2
    t, ctr = theta[1:4], theta[7:10]
    y = ((view.corr_point[:prop.K][keep] - t) - ctr) + ctr
    nrm = ctx.vertexNormals(theta)[ids]
    nn = np.einsum("ka,kb->kab", nrm, nrm)
    cov = sigma_n ** 2 * nn + sigma_t ** 2 * (np.eye(3)[None] - nn)
    res = pkg.posterior_models(ctx, [ids], [y], covariances=[cov], want=("alpha", "variance", "basis"))[0]
    assert res["status"] == 0
    figures = {"alpha": rel(res["alpha"], view.alpha), "S": rel(res["variance"], view.S), "basis": rel(res["basis"], model.basis @ view.V)}
    print(direction, {k: f"{v:.2e}" for k, v in figures.items()})
    assert figures["alpha"] <= 1e-9 and figures["S"] <= 1e-9 and figures["basis"] <= 1e-7
    prop.close()
    ctx.close()


# ---------------------------------------------------------------- 3. landmarks end to end

def test_landmarks_end_to_end(pkg, femur50, oracle):
    from test_gpu_chain import oracle_chain_config
    model, target = femur50
    _, _, lm_r = pkg.data.load_femur_mesh("femur_reference")
    _, _, lm_t = pkg.data.load_femur_mesh("femur_target")
    ids, pts = pkg.data.landmark_correspondences(model, lm_r, lm_t)
    ctx = pkg.IcpContext(model, target, device=0)
    post = ctx.posterior(ids, pts, sigma2=1.0)
    ctx.close()
    lf = LF.long_form(model, ids, pts, sigma2=1.0)
    assert post.rank == model.rank and np.all(np.diff(post.variance) <= 0)
    ctx2 = pkg.IcpContext(post, target, device=0)  # the returned model makes a new context
    theta0 = pkg.initial_parameters(post)
    mesh = ctx2.transformedMesh(theta0)
    want = model.ref_points + lf["mean"]
    print("posterior mean mesh:", rel(mesh, want))
    assert rel(mesh, want) <= 1e-9
    # a 20-step chain on the conditioned model against the oracle on the same arrays, decision for decision
    n_steps, seed = 20, 1024
    setup = pkg.femur_icp_proposal_registration(post, target)
    om, ot = oracle.OracleModel.from_model(post), oracle.OracleMesh(target.points, target.cells)
    acc_o, comp_o, logp_o, states_o = oracle.run_chain(om, ot, oracle_chain_config(oracle, setup), theta0, seed, n_steps)
    chain = pkg.SamplingRegistration(ctx2, setup, theta0, seed)
    rec = chain.run(n_steps)
    assert np.array_equal(rec[:, 1].astype(np.uint8), acc_o), "accept/reject sequences differ"
    assert np.array_equal(rec[:, 2].astype(np.int32), comp_o), "mixture components differ"
    scale = np.abs(states_o[:, 10:]).max()
    assert np.abs(rec[:, 4 + 10:] - states_o[:, 10:]).max() <= 1e-5 * scale
    assert np.abs(rec[:, 3] - logp_o).max() <= 1e-6 * np.abs(logp_o).max()
    chain.close()
    ctx2.close()


# ---------------------------------------------------------------- 4. batch invariance

WANT = ("alpha", "mean", "basis", "variance", "point_variance")


def mixed_batch(pkg, ctxs):
    """12 items over three models (ranks 51, 101, 201), both noise forms, different observation counts"""
    items = []
    for k in range(12):
        ctx = ctxs[k % 3]
        ids, y = observations(ctx.model, 40 + 37 * k, 300 + k)
        iso = k % 2 == 0
        items.append((ctx, ids, y, (0.1 + 0.2 * k) if iso else None, None if iso else random_spd(ids.shape[0], 400 + k)))
    return items


def run_items(pkg, items, order):
    sel = [items[i] for i in order]
    res = pkg.posterior_models([s[0] for s in sel], [s[1] for s in sel], [s[2] for s in sel], sigma2=[s[3] for s in sel],
                               covariances=[s[4] for s in sel], want=WANT)
    out = [None] * len(items)
    for i, rs in zip(order, res):
        out[i] = rs
    return out


def same_bits(a, b):
    return a["status"] == b["status"] and all(np.array_equal(a[w], b[w]) for w in WANT)


def test_batch_and_order_invariance(pkg):
    ctxs = []
    for n in (50, 100, 200):
        model, target = pkg.data.load_femur_model_and_target(n)
        ctxs.append(pkg.IcpContext(model, target, device=0))
    items = mixed_batch(pkg, ctxs)
    whole = run_items(pkg, items, list(range(12)))
    back = run_items(pkg, items, list(range(12))[::-1])
    for k in range(12):
        assert whole[k]["status"] == 0
        alone = run_items(pkg, items, [k])[k]
        assert same_bits(whole[k], alone), k
        assert same_bits(whole[k], back[k]), k
    for c in ctxs:
        c.close()


def _chunk_check():
    """(run as a program with the test-hooks library loaded) the mixed batch and a face item with the default chunk buffer and with
    ICP_TEST_POSTERIOR_MODELS_CHUNK_DOUBLES forcing several rounds per item: the same bits."""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    os.environ.pop("ICP_TEST_POSTERIOR_MODELS_CHUNK_DOUBLES", None)
    ctxs = []
    for n in (50, 100, 200):
        model, target = pkg.data.load_femur_model_and_target(n)
        ctxs.append(pkg.IcpContext(model, target, device=0))
    fm = pkg.data.synthetic_face_model(grid=169, rank=200)
    fctx = pkg.IcpContext(fm, pkg.data.synthetic_partial_target(fm), device=0)
    items = mixed_batch(pkg, ctxs)
    fids, fy = observations(fm, 300, 5)
    face_items = [(fctx, fids, fy, 0.1, None), (fctx, fids, fy, None, random_spd(300, 6))]
    want = run_items(pkg, items, list(range(12)))
    fwant = run_items(pkg, face_items, [0, 1])
    for doubles in (1 << 20, 300000):  # 137 MB of a face basis in 17 and in 58 rounds; a femur-200 basis (978,066 doubles) in 1 and in 4
        os.environ["ICP_TEST_POSTERIOR_MODELS_CHUNK_DOUBLES"] = str(doubles)
        got = run_items(pkg, items, list(range(12)))
        assert all(same_bits(a, b) for a, b in zip(want, got)), doubles
        fgot = run_items(pkg, face_items, [0, 1])
        assert all(same_bits(a, b) for a, b in zip(fwant, fgot)), doubles
    for c in ctxs + [fctx]:
        c.close()
    print("chunk check ok")


def test_forced_small_chunk_gives_the_same_bits():
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=900,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "chunk check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


# ---------------------------------------------------------------- 6. errors

def test_argument_errors_and_an_indefinite_covariance(pkg, femur50):
    """Every ICP_ERR_INVALID_ARG case leaves the outputs (a sentinel) and the status untouched; an indefinite covariance gives that item
    ICP_ERR_NOT_FINITE and NaN while its neighbours keep the bits of a run without it."""
    nat, L = pkg._native, pkg._native.lib()
    model, target = femur50
    ctx = pkg.IcpContext(model, target, device=0)
    r, N = model.rank, model.n_points
    dp, ip = nat.c_double_p, nat.c_int_p
    ids, y = observations(model, 30, 1)
    cov = random_spd(30, 2)
    s2 = np.array([0.5])
    alpha, var = np.full((2, r), 7.0), np.full((2, r), 7.0)
    mean, pvar = np.full((2, 3 * N), 7.0), np.full((2, N), 7.0)
    status = np.full(2, 99, dtype=np.int32)

    def ptrs(arrs, t=dp):
        return (t * len(arrs))(*[a.ctypes.data_as(t) if a is not None else None for a in arrs])

    def call(n=2, ctxs=(ctx.h, ctx.h), n_obs=(30, 30), ids_=(ids, ids), pts=(y, y), sig=(s2, None), covs=(None, cov)):
        c_ctx = (ctypes.c_void_p * len(ctxs))(*ctxs)
        nob = np.array(n_obs, dtype=np.int32)
        return L.icp_posterior_models_many(n, c_ctx, nob.ctypes.data_as(ip), ptrs(ids_, ip), ptrs(pts), ptrs(sig) if sig else None,
                                           ptrs(covs) if covs else None, ptrs([alpha[0], alpha[1]]), ptrs([mean[0], mean[1]]), None,
                                           ptrs([var[0], var[1]]), ptrs([pvar[0], pvar[1]]), status.ctypes.data_as(ip))

    bad_id, inf_y, nan_cov = ids.copy(), y.copy(), cov.copy()
    bad_id[7], inf_y[3, 1], nan_cov[5, 1, 1] = N, np.inf, np.nan
    cases = {
        "null context": dict(ctxs=(ctx.h, None)),
        "null ids": dict(ids_=(ids, None)),
        "null points": dict(pts=(None, y)),
        "n_items 0": dict(n=0),
        "n_items 65536": dict(n=65536),
        "n_obs 0": dict(n_obs=(30, 0)),
        "id out of range": dict(ids_=(bad_id, ids)),
        "negative id": dict(ids_=(ids, np.full(30, -1, dtype=np.int32))),
        "both noise forms": dict(sig=(s2, s2)),
        "neither noise form": dict(covs=(None, None)),
        "no noise at all": dict(sig=None, covs=None),
        "non-finite point": dict(pts=(inf_y, y)),
        "non-finite covariance": dict(covs=(None, nan_cov)),
        "non-finite sigma2": dict(sig=(np.array([np.nan]), None)),
        "sigma2 zero": dict(sig=(np.array([0.0]), None)),
        "sigma2 negative": dict(sig=(np.array([-1.0]), None)),
    }
    for name, kw in cases.items():
        assert call(**kw) == -1, name
        assert all(np.all(a == 7.0) for a in (alpha, var, mean, pvar)) and np.all(status == 99), name
    assert call() == 0 and np.all(status == 0) and not np.any(alpha == 7.0)
    # an indefinite covariance in the middle of a batch
    items = [(ctx, ids, y, 0.5, None), (ctx, ids, y, None, cov), (ctx, ids, y, None, cov)]
    clean = run_items(pkg, [items[0], items[2]], [0, 1])
    indef = cov.copy()
    indef[11] = np.diag([1.0, -0.5, 2.0])
    got = run_items(pkg, [items[0], (ctx, ids, y, None, indef), items[2]], [0, 1, 2])
    assert got[1]["status"] == -3 and all(np.all(np.isnan(got[1][w])) for w in WANT)
    assert same_bits(got[0], clean[0]) and same_bits(got[2], clean[1])
    assert all(v == 0 for v in pkg._native.runtime_stats(ctx.h).values())
    ctx.close()


if __name__ == "__main__":
    _chunk_check()
