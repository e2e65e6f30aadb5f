"""GPU: the batched model projection (icp_model_instances_many, icp_model_coefficients_many) through the public interface — instances
against icp_transformed_mesh bit for bit, coefficients against the long form in numpy, the reference's regularisation, poses and
registered rotation matrices, batch / order / chunk invariance, a face-sized call with its device memory bounded, argument errors."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, make_theta, open_patch_target

pytestmark = pytest.mark.gpu

SIGMA2 = 1e-5  # kSigma2 (icp-proposal_amd/csrc/abi_types.inl)
# icp-proposal_amd/csrc/abi_projection_many.inl and icp_kernels.hpp: the chunk buffer and the per-item records
CHUNK_DOUBLES = 4 << 20     # kProjChunkDoubles: meshes of a chunk; as many doubles again, in whole groups of 16 meshes, for residuals
GROUP = 16                  # kProjGroup
MIN_SLAB_ROWS, MAX_SLABS = 256, 128  # kProjMinSlabRows, kProjMaxSlabs
ITEM_RECORD_BYTES = 144     # sizeof(ProjItem): mesh pointer, Pose (16 doubles), flag
SAMPLE_RECORD_BYTES = 144   # sizeof(InstanceItem): an item given as a state, a projection
GROUP_RECORD_BYTES = 48     # sizeof(InstanceGroup); 8 instances a group


def bound_of(c):
    """1e-10 · max(1, max|c|): two f64 evaluation orders of the long form, and both against an extended-precision refinement, differ
    by at most 5.5e-14 on the three femur models (|c| up to 11, cond(QᵀQ + σ²I) up to 4,462); the smallest effect to resolve, the σ²
    shrink, is at least 2.7e-7.  1e-10 lies three orders from each."""
    return 1e-10 * max(1.0, float(np.abs(c).max()))


class LongForm:
    """np.linalg.solve(QᵀQ + σ²I, Qᵀ(x − x̄ − μ)) with Q = basis·√variance"""

    def __init__(self, model):
        self.model = model
        self.Q = model.basis * np.sqrt(model.variance)[None, :]
        self.A = self.Q.T @ self.Q + SIGMA2 * np.eye(model.rank)

    def coefficients(self, x):
        d = (np.asarray(x) - self.model.ref_points - self.model.mean_def).reshape(-1)
        return np.linalg.solve(self.A, self.Q.T @ d)

    def instance(self, c):
        return self.model.ref_points + self.model.mean_def + (self.Q @ c).reshape(-1, 3)


def unposed(theta):
    t = theta.copy()
    t[1:7] = 0.0
    return t


def rot_other_convention(angles):
    phi, t, psi = angles
    c, sn = np.cos, np.sin
    Rx = np.array([[1, 0, 0], [0, c(psi), -sn(psi)], [0, sn(psi), c(psi)]])
    Ry = np.array([[c(t), 0, sn(t)], [0, 1, 0], [-sn(t), 0, c(t)]])
    Rz = np.array([[c(phi), -sn(phi), 0], [sn(phi), c(phi), 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def hip_runtime():
    """the HIP runtime the library itself is linked to (as tests/test_gpu_variability_many.py takes it)"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) >= 1
    return ctypes.CDLL(sorted(paths)[0])


def free_bytes(hip):
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


@pytest.fixture(scope="module")
def femurs(pkg):
    return {n: pkg.data.load_femur_model_and_target(n) for n in (50, 100, 200)}


# ---------------------------------------------------------------- 1. instances

def test_instances_equal_transformed_mesh(pkg, femurs):
    """40 thetas, poses included, on two contexts with different targets; then contexts of two models (femur-50, femur-100) in one
    call: every row is ctx.transformedMesh(theta), bit for bit."""
    model, target = femurs[50]
    pts, cells = open_patch_target(target)
    a, b = pkg.IcpContext(model, target, device=0), pkg.IcpContext(model, pkg.data.TriangleMesh(pts, cells), device=0)
    th = [make_theta(model, 100 + s) for s in range(40)]
    ctxs = [a if s % 3 else b for s in range(40)]
    got = pkg.transformed_meshes(ctxs, th)
    assert got.shape == (40, model.n_points, 3)
    for s in range(40):
        assert np.array_equal(got[s], ctxs[s].transformedMesh(th[s])), s
    assert np.array_equal(pkg.transformed_meshes(a, np.stack(th))[7], a.transformedMesh(th[7]))
    m100, t100 = femurs[100]
    c = pkg.IcpContext(m100, t100, device=0)
    mixed_ctx = [a, c, c, a, b, c] * 4
    mixed_th = [make_theta(x.model, 900 + s) for s, x in enumerate(mixed_ctx)]
    got = pkg.transformed_meshes(mixed_ctx, mixed_th)
    for s, x in enumerate(mixed_ctx):
        assert np.array_equal(got[s], x.transformedMesh(mixed_th[s])), s
    for x in (a, b, c):
        x.close()


# ---------------------------------------------------------------- 2. and 3. coefficients

@pytest.mark.parametrize("n_comp", [50, 100, 200])
def test_coefficients_against_the_long_form(pkg, femurs, n_comp):
    """Model instances given as points, the same given as thetas, and instances plus 1 mm Gaussian vertex noise (not in the span):
    within 1e-10 · max(1, max|c|) of np.linalg.solve(QᵀQ + σ²I, Qᵀ(x − x̄ − μ))."""
    model, target = femurs[n_comp]
    lf = LongForm(model)
    ctx = pkg.IcpContext(model, target, device=0)
    rng = np.random.default_rng(n_comp)
    th = [unposed(make_theta(model, 10 * n_comp + s, shape_scale=1.0)) for s in range(12)]
    th[0][10:] = np.clip(rng.normal(size=model.rank) * 4.0, -11.0, 11.0)
    inst = pkg.transformed_meshes(ctx, th)
    noisy = inst + rng.normal(size=inst.shape)
    for kind, kw, meshes in (("points", dict(meshes=list(inst)), inst), ("thetas", dict(thetas=th), inst),
                             ("noisy", dict(meshes=list(noisy)), noisy)):
        got = pkg.model_coefficients(ctx, **kw)
        assert got.shape == (12, model.rank)
        worst = 0.0
        for s in range(12):
            want = lf.coefficients(meshes[s])
            err = np.abs(got[s] - want).max()
            worst = max(worst, err / bound_of(want))
            assert err <= bound_of(want), (kind, s, err, bound_of(want))
        print(f"femur-{n_comp} {kind}: worst |c - long form| / bound = {worst:.3e} (bound 1e-10 · max(1, max|c|))")
    ctx.close()


@pytest.mark.parametrize("n_comp", [50, 200])
def test_the_regularisation_is_the_references(pkg, femurs, n_comp):
    """coefficients(instance(c)) = c − σ²·P·c with P = (QᵀQ + σ²I)⁻¹ (numpy) within the bound; at rank 201 it differs from c by more
    than 1e-8: an unregularised solve fails here."""
    model, target = femurs[n_comp]
    lf = LongForm(model)
    ctx = pkg.IcpContext(model, target, device=0)
    rng = np.random.default_rng(3)
    cs = rng.normal(size=(8, model.rank)) * np.sqrt(0.1)
    got = pkg.model_coefficients(ctx, meshes=[lf.instance(c) for c in cs])
    shrink = 0.0
    for c, g in zip(cs, got):
        want = c - SIGMA2 * np.linalg.solve(lf.A, c)
        err = np.abs(g - want).max()
        print(f"femur-{n_comp}: |c' - (c - s2 P c)| = {err:.3e}, bound {bound_of(want):.3e}; |c' - c| = {np.abs(g - c).max():.3e}")
        assert err <= bound_of(want)
        shrink = max(shrink, np.abs(g - c).max())
    if n_comp == 200:
        assert shrink > 1e-8
    ctx.close()


# ---------------------------------------------------------------- 4. pose

def test_pose_is_taken_off_and_put_back(pkg, femurs):
    """coefficients(transformedMesh(theta), pose = theta[:10]) equals coefficients of the unposed instance within the bound, also on
    a context with a registered Scalismo rotation matrix; project with that pose is transformedMesh([pose | c]) bit for bit; s != 1
    is refused."""
    model, target = femurs[50]
    plain, reg = pkg.IcpContext(model, target, device=0), pkg.IcpContext(model, target, device=0)
    th = [make_theta(model, 300 + s) for s in range(6)]
    rng = np.random.default_rng(4)
    for t in th:
        t[1:4] = rng.normal(size=3) * 20.0
        t[4:7] = rng.normal(size=3) * 0.4
    for s in (0, 3):
        reg.setRotation(th[s][4:7], rot_other_convention(th[s][4:7]))
    for ctx in (plain, reg):
        posed = pkg.transformed_meshes(ctx, th)
        if ctx is reg:
            assert np.abs(posed[0] - plain.transformedMesh(th[0])).max() > 1.0  # (the other convention moved the mesh)
        base = pkg.model_coefficients(ctx, meshes=list(pkg.transformed_meshes(ctx, [unposed(t) for t in th])))
        got, proj = pkg.model_coefficients(ctx, meshes=list(posed), poses=[t[:10] for t in th], want_project=True)
        from_theta = pkg.model_coefficients(ctx, thetas=th, poses=[t[:10] for t in th])
        for s, t in enumerate(th):
            err = max(np.abs(got[s] - base[s]).max(), np.abs(from_theta[s] - base[s]).max())
            print(f"pose {s}: |c(posed, pose) - c(unposed)| = {err:.3e}, bound {bound_of(base[s]):.3e}")
            assert err <= bound_of(base[s])
            assert np.array_equal(proj[s], ctx.transformedMesh(np.concatenate([t[:10], got[s]])))
            assert np.array_equal(ctx.project(posed[s], pose=t[:10]), proj[s])
        # without a pose the projection is the instance under the identity pose
        c0, p0 = pkg.model_coefficients(ctx, meshes=[posed[1]], want_project=True)
        ident = np.zeros(10)
        ident[0] = 1.0
        assert np.array_equal(p0[0], ctx.transformedMesh(np.concatenate([ident, c0[0]])))
    bad = th[0][:10].copy()
    bad[0] = 1.01
    with pytest.raises(ValueError):
        plain.coefficients(np.zeros((model.n_points, 3)), pose=bad)
    plain.close()
    reg.close()


# ---------------------------------------------------------------- 5. batch, order and chunk invariance

def mixed_items(pkg, ctx, model, n=40, seed=7):
    rng = np.random.default_rng(seed)
    th = [make_theta(model, 500 + s) for s in range(n)]
    posed = pkg.transformed_meshes(ctx, th)
    meshes, thetas, poses = [], [], []
    for s in range(n):
        as_theta, with_pose = s % 2 == 1, s % 4 >= 2
        meshes.append(None if as_theta else posed[s] + (rng.normal(size=posed[s].shape) if s % 3 == 0 else 0.0))
        thetas.append(th[s] if as_theta else None)
        poses.append(th[s][:10] if with_pose else None)
    return meshes, thetas, poses


def run_split(pkg, ctx, items, order, size):
    meshes, thetas, poses = items
    n = len(meshes)
    c, p = np.zeros((n, ctx.rank)), np.zeros((n, ctx.N, 3))
    for k in range(0, n, size):
        idx = order[k:k + size]
        gc, gp = pkg.model_coefficients(ctx, meshes=[meshes[i] for i in idx], thetas=[thetas[i] for i in idx],
                                        poses=[poses[i] for i in idx], want_project=True)
        c[idx], p[idx] = gc, gp
    return c, p


def test_batch_and_order_invariance(pkg, femurs):
    """40 mixed items (points / thetas, with and without pose) as one call and as calls of 1 and of 7 in shuffled order: identical
    arrays; IcpContext.coefficients of one item gives the bits of its row."""
    model, target = femurs[200]
    ctx = pkg.IcpContext(model, target, device=0)
    items = mixed_items(pkg, ctx, model)
    want_c, want_p = run_split(pkg, ctx, items, list(range(40)), 40)
    order = list(np.random.default_rng(1).permutation(40))
    for size in (1, 7):
        c, p = run_split(pkg, ctx, items, order, size)
        assert np.array_equal(c, want_c) and np.array_equal(p, want_p), size
    assert np.array_equal(ctx.coefficients(items[0][4]), want_c[4])
    assert np.array_equal(ctx.coefficients(items[0][2], pose=items[2][2]), want_c[2])
    ctx.close()


def _chunk_check():
    """(run as a program with the test-hooks library loaded) the mixed batch, and 40 instances, with the default chunk buffer and with
    ICP_TEST_PROJECTION_CHUNK_DOUBLES = 5 and 1.5 femur meshes: the same bits."""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    model, target = pkg.data.load_femur_model_and_target(50)
    ctx = pkg.IcpContext(model, target, device=0)
    os.environ.pop("ICP_TEST_PROJECTION_CHUNK_DOUBLES", None)
    items = mixed_items(pkg, ctx, model)
    th = [make_theta(model, 500 + s) for s in range(40)]
    want_c, want_p = run_split(pkg, ctx, items, list(range(40)), 40)
    want_x = pkg.transformed_meshes(ctx, th)
    n3 = 3 * model.n_points
    for doubles in (5 * n3, n3 + n3 // 2):
        os.environ["ICP_TEST_PROJECTION_CHUNK_DOUBLES"] = str(doubles)
        c, p = run_split(pkg, ctx, items, list(range(40)), 40)
        assert np.array_equal(c, want_c) and np.array_equal(p, want_p), doubles
        assert np.array_equal(pkg.transformed_meshes(ctx, th), want_x), doubles
    ctx.close()
    print("chunk check ok")


def test_forced_small_chunk_gives_the_same_bits():
    """Test-hooks build: with a chunk buffer of five meshes and of one and a half (chunks of one), coefficients, projections and
    instances have the bits of the default."""
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "chunk check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


# ---------------------------------------------------------------- 6. face size

def test_face_size_within_the_bound_and_the_chunk_buffer(pkg):
    """N = 28,561, rank 200, 48 items (24 as noisy points, 24 as thetas): within the bound of the long form.  Device memory the call
    may take, from the sizes in abi_projection_many.inl: the chunk buffer (meshes, CHUNK_DOUBLES doubles at most), the residuals (the
    chunk's meshes rounded up to whole groups of 16), the slabs' partial sums (groups · slabs · rank rounded up to 16 · 16 doubles),
    the coefficient rows, the per-item records, and 2 MiB of allocator granularity for each of the call's 10 buffers."""
    model = pkg.data.synthetic_face_model(grid=169, rank=200)
    target = pkg.data.synthetic_partial_target(model)
    ctx = pkg.IcpContext(model, target, device=0)
    N, r, n = model.n_points, model.rank, 48
    lf = LongForm(model)
    rng = np.random.default_rng(11)
    th = np.tile(pkg.initial_parameters(model), (n, 1))
    th[:, 10:] = 0.5 * rng.normal(size=(n, r))
    meshes = [lf.instance(th[s, 10:]) + rng.normal(size=(N, 3)) if s < 24 else None for s in range(n)]
    thetas = [None if s < 24 else th[s] for s in range(n)]
    ctx.transformedMesh(th[0])  # (the context's own state slots are made before the first reading)
    hip = hip_runtime()
    free0 = free_bytes(hip)
    got = pkg.model_coefficients(ctx, meshes=meshes, thetas=thetas)
    free1 = free_bytes(hip)
    per_chunk = min(n, CHUNK_DOUBLES // (3 * N))
    groups = -(-per_chunk // GROUP)
    slab_rows = -(-max(MIN_SLAB_ROWS, -(-3 * N // MAX_SLABS)) // 16) * 16
    slabs = -(-3 * N // slab_rows)
    bound = (per_chunk * 3 * N * 8 + groups * GROUP * 3 * N * 8 + groups * slabs * (-(-r // 16) * 16) * GROUP * 8 + 2 * n * r * 8
             + n * (ITEM_RECORD_BYTES + SAMPLE_RECORD_BYTES + 4) + (n // 8 + 2) * GROUP_RECORD_BYTES + 10 * (2 << 20))
    assert per_chunk * 3 * N <= CHUNK_DOUBLES
    print(f"device memory taken by the call: {(free0 - free1) / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB")
    assert free0 - free1 <= bound
    worst = 0.0
    for s in range(n):
        want = lf.coefficients(meshes[s] if s < 24 else lf.instance(th[s, 10:]))
        err = np.abs(got[s] - want).max()
        worst = max(worst, err / bound_of(want))
        assert err <= bound_of(want), (s, err)
    print(f"face, 48 items: worst |c - long form| / bound = {worst:.3e}")
    st = pkg._native.runtime_stats(ctx.h)
    assert all(v == 0 for v in st.values()), st
    ctx.close()


# ---------------------------------------------------------------- 7. errors

def test_argument_errors_and_non_finite_items(pkg, femurs):
    """Every ICP_ERR_INVALID_ARG case leaves the outputs untouched (a sentinel); an item with one NaN vertex gets ICP_ERR_NOT_FINITE
    and a NaN row while its neighbours keep their bits; runtime_stats is all zero afterwards."""
    nat = pkg._native
    L = nat.lib()
    model, target = femurs[50]
    m100, t100 = femurs[100]
    ctx, other_model = pkg.IcpContext(model, target, device=0), pkg.IcpContext(m100, t100, device=0)
    N, r = model.n_points, model.rank
    dp = nat.c_double_p
    th = [make_theta(model, 70 + s) for s in range(3)]
    mesh = pkg.transformed_meshes(ctx, th)
    coeffs, proj, status = np.full((2, r), -7.0), np.full((2, N, 3), -7.0), np.full(2, 99, dtype=np.int32)
    pts_out = np.full((2, N, 3), -7.0)

    def as_p(arrs):
        return (dp * max(1, len(arrs)))(*[a.ctypes.data_as(dp) if a is not None else None for a in arrs])

    def ctx_p(cs):
        return (ctypes.c_void_p * max(1, len(cs)))(*[c.h if c is not None else None for c in cs])

    def coeff_call(cs, pts, ths, poses, n=None, want_proj=True):
        rc = L.icp_model_coefficients_many(len(cs) if n is None else n, ctx_p(cs), as_p(pts) if pts is not None else None,
                                           as_p(ths) if ths is not None else None, as_p(poses) if poses is not None else None,
                                           coeffs.ctypes.data_as(dp), as_p([proj[0], proj[1]]) if want_proj else None,
                                           status.ctypes.data_as(nat.c_int_p))
        return rc, (L.icp_last_error() or b"").decode()

    def inst_call(cs, ths, outs, n=None):
        rc = L.icp_model_instances_many(len(cs) if n is None else n, ctx_p(cs), as_p(ths), as_p(outs))
        return rc, (L.icp_last_error() or b"").decode()

    bad_th = th[1].copy()
    bad_th[12] = np.inf
    pose, bad_pose, scaled = th[0][:10].copy(), th[0][:10].copy(), th[0][:10].copy()
    bad_pose[5] = np.nan
    scaled[0] = 0.5
    cases = [
        ("null", ([ctx, None], [mesh[0], mesh[1]], None, None)),
        ("n_items", ([ctx, ctx], [mesh[0], mesh[1]], None, None, 0)),
        ("n_items", ([ctx, ctx], [mesh[0], mesh[1]], None, None, 65536)),
        ("one of the two", ([ctx, ctx], [mesh[0], mesh[1]], [None, th[1]], None)),
        ("one of the two", ([ctx, ctx], [mesh[0], None], [None, None], None)),
        ("one of the two", ([ctx, ctx], None, None, None)),
        ("non-finite", ([ctx, ctx], [mesh[0], None], [None, bad_th], None)),
        ("non-finite", ([ctx, ctx], [mesh[0], mesh[1]], None, [pose, bad_pose])),
        ("exactly 1", ([ctx, ctx], [mesh[0], mesh[1]], None, [None, scaled])),
        ("model", ([ctx, other_model], [mesh[0], mesh[1]], None, None)),
    ]
    other_dev, n_dev = None, ctypes.c_int(0)
    assert hip_runtime().hipGetDeviceCount(ctypes.byref(n_dev)) == 0
    if n_dev.value >= 2:
        other_dev = pkg.IcpContext(model, target, device=1)
        cases.append(("device", ([ctx, other_dev], [mesh[0], mesh[1]], None, None)))
    for text, args in cases:
        rc, err = coeff_call(*args)
        assert rc == -1 and text in err, (text, rc, err)
        assert np.all(coeffs == -7.0) and np.all(proj == -7.0) and np.all(status == 99), text
    inst_cases = [("null", ([ctx, None], [th[0], th[1]], [pts_out[0], pts_out[1]])),
                  ("null", ([ctx, ctx], [th[0], None], [pts_out[0], pts_out[1]])),
                  ("null", ([ctx, ctx], [th[0], th[1]], [pts_out[0], None])),
                  ("n_items", ([ctx, ctx], [th[0], th[1]], [pts_out[0], pts_out[1]], 0)),
                  ("non-finite", ([ctx, ctx], [th[0], bad_th], [pts_out[0], pts_out[1]]))]
    if other_dev is not None:
        inst_cases.append(("device", ([ctx, other_dev], [th[0], th[1]], [pts_out[0], pts_out[1]])))
    for text, args in inst_cases:
        rc, err = inst_call(*args)
        assert rc == -1 and text in err, (text, rc, err)
        assert np.all(pts_out == -7.0), text
    # the same arguments without the fault run
    rc, err = coeff_call([ctx, ctx], [mesh[0], None], [None, th[1]], [pose, None])
    assert rc == 0 and np.all(status == 0), err
    good_c, good_p = coeffs.copy(), proj.copy()
    assert np.array_equal(good_c[0], ctx.coefficients(mesh[0], pose=pose)) and np.array_equal(good_p[0], ctx.project(mesh[0], pose=pose))
    # one NaN vertex in the second of three items
    hurt = mesh[1].copy()
    hurt[100, 1] = np.nan
    c3, p3, s3 = np.zeros((3, r)), np.zeros((3, N, 3)), np.zeros(3, dtype=np.int32)
    rc = L.icp_model_coefficients_many(3, ctx_p([ctx] * 3), as_p([mesh[0], hurt, mesh[2]]), None, as_p([pose, None, None]),
                                       c3.ctypes.data_as(dp), as_p([p3[0], p3[1], p3[2]]), s3.ctypes.data_as(nat.c_int_p))
    assert rc == -3 and list(s3) == [0, -3, 0]
    assert np.all(np.isnan(c3[1])) and np.all(np.isnan(p3[1]))
    assert np.array_equal(c3[0], good_c[0]) and np.array_equal(p3[0], good_p[0])
    assert np.array_equal(c3[2], ctx.coefficients(mesh[2])) and np.array_equal(p3[2], ctx.project(mesh[2]))
    with pytest.raises(nat.IcpNativeError):
        ctx.coefficients(hurt)
    st = nat.runtime_stats(ctx.h)
    assert all(v == 0 for v in st.values()), st
    if other_dev is not None:
        other_dev.close()
    ctx.close()
    other_model.close()


if __name__ == "__main__":
    _chunk_check()
