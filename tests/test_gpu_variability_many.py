"""GPU: the posterior variability maps of many chains in one call (icp_posterior_variability_many) against the one-map entry
(icp_posterior_variability, bit for bit) and the CPU oracle; batch and chunk invariance, poses and registered rotation matrices, a
face-sized map streamed through the chunk buffer with its device memory bounded, the femur study's size, and argument errors."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, make_theta

pytestmark = pytest.mark.gpu

# icp-proposal_amd/csrc/abi_variability_many.inl: kVarChunkDoubles (the chunk buffer) and the per-sample records
CHUNK_DOUBLES = 8 << 20
SAMPLE_RECORD_BYTES = 144   # sizeof(InstanceItem): coefficient pointer, Pose (16 doubles), mesh pointer
GROUP_RECORD_BYTES = 48     # sizeof(InstanceGroup); kInstGroup = 8 samples a group
SIZES = (2, 3, 25, 41, 12)  # samples per map of the mixed batches
ORACLE_REL = 1e-12          # of the map's maximum: the bound tests/test_gpu_fit.py holds the one-map entry to


def sample_set(model, seed, n, scale=0.3):
    return np.stack([make_theta(model, seed + s, shape_scale=scale) for s in range(n)])


def hip_runtime():
    """the HIP runtime the library itself is linked to (the very file this process has mapped, as tests/test_gpu_chain.py takes it:
    torch brings a runtime of its own, which is another runtime and sees no device from this process)"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) >= 1
    return ctypes.CDLL(sorted(paths)[0])


def free_bytes(hip):
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def one_map(pkg, ctx, th, mode, ref):
    return pkg.posterior_variability(ctx, th, mode=mode, theta_ref=ref)


@pytest.fixture(scope="module")
def femur200(pkg):
    return pkg.data.load_femur_model_and_target(200)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bits_against_one_map_entry_and_oracle(pkg, oracle, femur50, femur50_oracle, mode):
    """Maps of 2, 3, 25, 41 and 12 samples in one call: each equals the one-map entry bit for bit and the oracle within the bound
    tests/test_gpu_fit.py holds the one-map entry to (1e-12 of the map's maximum); the mean mesh is the numpy mean of the samples'
    icp_transformed_mesh within 1e-12 of the largest coordinate."""
    model, target = femur50
    om, _ = femur50_oracle
    ctx = pkg.IcpContext(model, target, device=0)
    sets = [sample_set(model, 1000 * (k + 1), n) for k, n in enumerate(SIZES)]
    refs = [th[1] for th in sets]
    got, means = pkg.posterior_variability_maps(ctx, sets, mode=mode, theta_refs=refs, want_mean=True)
    for th, ref, g, mu in zip(sets, refs, got, means):
        assert g.shape == (model.n_points,) and np.all(g >= 0)
        assert np.array_equal(g, one_map(pkg, ctx, th, mode, ref))
        want = oracle.posterior_variability(om, th, mode=mode, theta_ref=ref)
        err = np.abs(g - want).max()
        print(f"mode {mode} S {th.shape[0]}: |map - oracle| = {err:.3e}, bound {ORACLE_REL * np.abs(want).max():.3e}")
        assert err <= ORACLE_REL * np.abs(want).max()
        x = np.stack([ctx.transformedMesh(t) for t in th])
        assert np.abs(mu - x.mean(axis=0)).max() <= 1e-12 * np.abs(x).max()
    ctx.close()


def test_batch_invariance_across_models(pkg, femur50, femur200):
    """The same map alone, first, last, duplicated and between maps of another model and rank (femur-200): identical bits, in every
    mode; the other model's maps are those of its own one-map entry."""
    m50, t50 = femur50
    m200, t200 = femur200
    c50, c200 = pkg.IcpContext(m50, t50, device=0), pkg.IcpContext(m200, t200, device=0)
    a, b, w = sample_set(m50, 10, 25), sample_set(m50, 500, 7), sample_set(m200, 900, 9)
    for mode in (0, 1, 2):
        alone = pkg.posterior_variability_maps(c50, [a], mode=mode, theta_refs=[a[0]])[0]
        ctxs = [c50, c200, c50, c50, c200, c50]
        sets = [a, w, b, a, w, a]
        modes = [mode, 2, 0, mode, mode, mode]
        got = pkg.posterior_variability_maps(ctxs, sets, mode=modes, theta_refs=[s[0] for s in sets])
        for k in (0, 3, 5):
            assert np.array_equal(got[k], alone)
        assert np.array_equal(alone, one_map(pkg, c50, a, mode, a[0]))
        assert np.array_equal(got[1], one_map(pkg, c200, w, 2, w[0])) and np.array_equal(got[4], one_map(pkg, c200, w, mode, w[0]))
        assert np.array_equal(got[2], one_map(pkg, c50, b, 0, None))
    c50.close()
    c200.close()


def _chunk_check():
    """(run as a program with the test-hooks library loaded) the mixed batch of every mode with the default chunk buffer and with
    ICP_TEST_VARIABILITY_CHUNK_DOUBLES = 5 and 1.5 femur meshes: the same bits, maps and means."""
    from conftest import load_package
    pkg = load_package()
    assert pkg._native.LIB_PATH.endswith("_testhooks.so")
    model, target = pkg.data.load_femur_model_and_target(50)
    ctx = pkg.IcpContext(model, target, device=0)
    sets = [sample_set(model, 1000 * (k + 1), n) for k, n in enumerate(SIZES)] * 3
    modes = [0] * len(SIZES) + [1] * len(SIZES) + [2] * len(SIZES)
    refs = [th[1] for th in sets]
    os.environ.pop("ICP_TEST_VARIABILITY_CHUNK_DOUBLES", None)
    want, want_mu = pkg.posterior_variability_maps(ctx, sets, mode=modes, theta_refs=refs, want_mean=True)
    for k in (0, len(SIZES) + 2, 2 * len(SIZES) + 3):
        assert np.array_equal(want[k], one_map(pkg, ctx, sets[k], modes[k], refs[k]))
    n3 = 3 * model.n_points
    for doubles in (5 * n3, n3 + n3 // 2):
        os.environ["ICP_TEST_VARIABILITY_CHUNK_DOUBLES"] = str(doubles)
        got, got_mu = pkg.posterior_variability_maps(ctx, sets, mode=modes, theta_refs=refs, want_mean=True)
        for k in range(len(sets)):
            assert np.array_equal(got[k], want[k]), (doubles, k)
            assert np.array_equal(got_mu[k], want_mu[k]), (doubles, k)
    ctx.close()
    print("chunk check ok")


def test_forced_small_chunk_gives_the_same_bits():
    """Test-hooks build: with a chunk buffer of five meshes (maps of 25, 41 and 12 samples run in segments, twice) and of one and a
    half (a mode-2 sample and its normals do not fit: the buffer grows to hold one), every map and mean has the bits of the default."""
    hooks = os.path.join(ROOT, "icp-proposal_amd", "libicp_proposal_amd_testhooks.so")
    assert os.path.exists(hooks), "build the test-hooks library (python -c 'import __graft_entry__ as g; g.build()')"
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                          env={**os.environ, "ICP_LIBRARY_PATH": hooks})
    assert done.returncode == 0 and "chunk check ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


def test_poses_and_registered_rotation(pkg, femur50):
    """Samples with large rotations and translations, on a context with a registered rotation matrix of another convention for some
    of the samples' Euler triples: the bits of the one-map entry, and the registered matrix is the one that was used."""
    model, target = femur50
    ctx = pkg.IcpContext(model, target, device=0)
    plain = pkg.IcpContext(model, target, device=0)
    th = sample_set(model, 40, 12)
    rng = np.random.default_rng(3)
    th[:, 1:4] = rng.normal(size=(12, 3)) * 20.0
    th[:, 4:7] = rng.normal(size=(12, 3)) * 0.4
    for s in (0, 5, 11):
        phi, t, psi = th[s, 4:7]
        c, sn = np.cos, np.sin
        Rx = np.array([[1, 0, 0], [0, c(psi), -sn(psi)], [0, sn(psi), c(psi)]])
        Ry = np.array([[c(t), 0, sn(t)], [0, 1, 0], [-sn(t), 0, c(t)]])
        Rz = np.array([[c(phi), -sn(phi), 0], [sn(phi), c(phi), 0], [0, 0, 1]])
        ctx.setRotation(th[s, 4:7], Rx @ Ry @ Rz)
    for mode in (0, 1, 2):
        got, mu = pkg.posterior_variability_maps([ctx, plain], [th, th], mode=mode, theta_refs=[th[5], th[5]], want_mean=True)
        assert np.array_equal(got[0], one_map(pkg, ctx, th, mode, th[5]))
        assert np.array_equal(got[1], one_map(pkg, plain, th, mode, th[5]))
        assert np.abs(mu[0] - mu[1]).max() > 1.0  # (the other convention moved three samples)
    ctx.close()
    plain.close()


def test_face_map_streams_through_the_chunk_buffer(pkg):
    """N = 28,561, rank 200.  S = 400 (274 MB of sample meshes, four chunk buffers): the bits of the one-map entry in modes 0 and 2.
    S = 4,000 in mode 0 (2.7 GB if held resident) completes without time-outs or fall-backs.  Device memory the two batched calls
    may take, from the sizes alone: the chunk buffer (64 MiB), 10 N doubles of per-map state, each call's coefficients (S · rank
    doubles), its sample records (two sweeps of S), group and segment records, and 2 MiB of allocator granularity for each of the 9
    buffers of a call.  (The mode-2 call and the one-map yardstick run after the second reading.)  Free memory is hipMemGetInfo of the
    runtime the library runs on — what torch.cuda.mem_get_info reports where torch shares that runtime, which it does not here."""
    model = pkg.data.synthetic_face_model(grid=169, rank=200)
    target = pkg.data.synthetic_partial_target(model)
    ctx = pkg.IcpContext(model, target, device=0)
    N, r = model.n_points, model.rank
    rng = np.random.default_rng(11)

    def states(S):
        th = np.tile(pkg.initial_parameters(model), (S, 1))
        th[:, 10:] = 0.3 * rng.normal(size=(S, r))
        th[:, 1:4] = rng.normal(size=(S, 3))
        th[:, 4:7] = 0.01 * rng.normal(size=(S, 3))
        return th

    def call_bytes(S):
        return S * r * 8 + 2 * S * SAMPLE_RECORD_BYTES + 2 * (S // 8 + S // 16 + 2) * GROUP_RECORD_BYTES + 64 * 1024 + 9 * (2 << 20)

    small, big = states(400), states(4000)
    assert 400 * 3 * N * 8 > 4 * CHUNK_DOUBLES * 8
    hip = hip_runtime()
    free0 = free_bytes(hip)
    got0 = pkg.posterior_variability_maps(ctx, [small], mode=0)[0]
    got_big = pkg.posterior_variability_maps(ctx, [big], mode=0)[0]
    free1 = free_bytes(hip)
    bound = CHUNK_DOUBLES * 8 + 10 * N * 8 + call_bytes(400) + call_bytes(4000)
    print(f"device memory taken by the batched calls: {(free0 - free1) / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB")
    assert free0 - free1 <= bound
    assert got_big.shape == (N,) and np.all(np.isfinite(got_big)) and np.all(got_big >= 0) and got_big.max() > 0
    st = pkg._native.runtime_stats(ctx.h)
    assert all(v == 0 for v in st.values()), st
    assert np.array_equal(got0, one_map(pkg, ctx, small, 0, None))
    got2 = pkg.posterior_variability_maps(ctx, [small], mode=2)[0]
    assert np.array_equal(got2, one_map(pkg, ctx, small, 2, None))
    ctx.close()


def test_study_size(pkg, femur200):
    """200 maps of 20 samples on one femur-200 context (the chains of one target of the femur study), modes 0 and 2: every tenth map
    against the one-map entry."""
    model, target = femur200
    ctx = pkg.IcpContext(model, target, device=0)
    rng = np.random.default_rng(5)
    base = pkg.initial_parameters(model)
    sets = []
    for m in range(200):
        th = np.tile(base, (20, 1))
        th[:, 10:] = 0.3 * rng.normal(size=(20, model.rank))
        th[:, 1:4] = 0.5 * rng.normal(size=(20, 3))
        th[:, 4:7] = 0.01 * rng.normal(size=(20, 3))
        sets.append(th)
    for mode in (0, 2):
        got = pkg.posterior_variability_maps(ctx, sets, mode=mode)
        assert len(got) == 200
        for m in range(0, 200, 10):
            assert np.array_equal(got[m], one_map(pkg, ctx, sets[m], mode, None)), (mode, m)
    ctx.close()


def test_argument_errors(pkg, femur50):
    """n_maps = 0 is accepted; a null entry, S < 2, an unknown mode, mode 1 without a reference, a non-finite theta (and contexts on
    two devices where there are two) return ICP_ERR_INVALID_ARG with icp_last_error's text, and nothing is written."""
    nat = pkg._native
    L = nat.lib()
    model, target = femur50
    ctx = pkg.IcpContext(model, target, device=0)
    N = model.n_points
    th = sample_set(model, 70, 4)
    dp = nat.c_double_p

    def call(ctxs, ns, thetas, modes, refs, outs, n_maps=None):
        n = len(ctxs) if n_maps is None else n_maps
        c_ctx = (ctypes.c_void_p * max(1, len(ctxs)))(*[c.h if c is not None else None for c in ctxs])
        c_n = np.array(ns, dtype=np.int32)
        c_mode = np.array(modes, dtype=np.int32)
        as_p = lambda arrs: (dp * max(1, len(arrs)))(*[a.ctypes.data_as(dp) if a is not None else None for a in arrs])
        rc = L.icp_posterior_variability_many(n, c_ctx, c_n.ctypes.data_as(nat.c_int_p), as_p(thetas), c_mode.ctypes.data_as(nat.c_int_p),
                                              as_p(refs) if refs is not None else None, as_p(outs), None)
        return rc, (L.icp_last_error() or b"").decode()

    assert L.icp_posterior_variability_many(0, None, None, None, None, None, None, None) == 0
    out = np.full(N, -7.0)
    good = np.full(N, -7.0)
    bad = th.copy()
    bad[2, 12] = np.inf
    cases = [
        ("null", ([ctx, None], [4, 4], [th, th], [0, 0], None, [good, out])),
        ("null", ([ctx, ctx], [4, 4], [th, None], [0, 0], None, [good, out])),
        ("null", ([ctx, ctx], [4, 4], [th, th], [0, 0], None, [good, None])),
        ("two samples", ([ctx, ctx], [4, 1], [th, th], [0, 0], None, [good, out])),
        ("mode", ([ctx, ctx], [4, 4], [th, th], [0, 3], None, [good, out])),
        ("mode", ([ctx, ctx], [4, 4], [th, th], [0, -1], None, [good, out])),
        ("theta_ref", ([ctx, ctx], [4, 4], [th, th], [0, 1], None, [good, out])),
        ("theta_ref", ([ctx, ctx], [4, 4], [th, th], [0, 1], [th[0], None], [good, out])),
        ("non-finite", ([ctx, ctx], [4, 4], [th, bad], [0, 0], None, [good, out])),
        ("non-finite", ([ctx, ctx], [4, 4], [th, th], [0, 1], [None, bad[2]], [good, out])),
    ]
    other, n_dev = None, ctypes.c_int(0)
    assert hip_runtime().hipGetDeviceCount(ctypes.byref(n_dev)) == 0
    if n_dev.value >= 2:
        other = pkg.IcpContext(model, target, device=1)
        cases.append(("device", ([ctx, other], [4, 4], [th, th], [0, 0], None, [good, out])))
    for text, args in cases:
        rc, err = call(*args)
        assert rc == -1 and text in err, (text, rc, err)
        assert np.all(good == -7.0) and np.all(out == -7.0)
    assert call([], [], [], [], None, [], n_maps=-1)[0] == -1
    # and the same arguments without the fault run
    rc, err = call([ctx, ctx], [4, 4], [th, th], [0, 1], [None, th[2]], [good, out])
    assert rc == 0, err
    assert np.array_equal(good, one_map(pkg, ctx, th, 0, None)) and np.array_equal(out, one_map(pkg, ctx, th, 1, th[2]))
    if other is not None:
        other.close()
    ctx.close()


if __name__ == "__main__":
    _chunk_check()
