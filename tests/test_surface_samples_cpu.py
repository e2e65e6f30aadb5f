"""CPU: uniform surface samples and a kernel's total variance (icp_surface_samples_many, icp_kernel_total_variance_many,
api.surface_samples, api.total_variance, data.surface_samples / approx_total_variance / fit_samples) — the numpy long
form the GPU tests compare with (tests/surface_samples_long_form.py): its generator against the oracle's, its bounds, its law on two
triangles, its barycentric rows; the ABI surface; and the real library's refusal of every bad argument before it touches a device."""
import ctypes
import os

import numpy as np
import pytest

import surface_samples_long_form as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_generator_is_the_oracles(oracle):
    L = oracle.lib()
    for seed in (0, 5, 2 ** 63 + 7):
        for step in (0, 1, 2):
            lanes = [0, 1, 4095, 2 ** 40]
            got = LF.u(seed, step, lanes)
            want = [L.orc_rng_uniform(seed, step, lane) for lane in lanes]
            assert got.tolist() == want, (seed, step)
            hh = LF.h(seed, step, lanes)
            assert np.all(hh < np.uint64(1 << 53)) and np.all(got > 0.0) and np.all(got < 1.0)


def two_triangles():
    """areas 1 : 3"""
    pts = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [10.0, 0.0, 0.0], [13.0, 0.0, 0.0], [10.0, 2.0, 0.0]])
    return pts, np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)


def test_bounds_of_the_pick():
    pts, cells = two_triangles()
    q, C, Q, amax = LF.weights(pts, cells)
    assert LF.double_areas(pts, cells).tolist() == [2.0, 6.0] and amax == 6.0
    assert q.tolist() == [1431655765, 4294967296] and C.tolist() == [1431655765, 5726623061] and Q == 5726623061
    for seed in (0, 5, 1024, 2 ** 64 - 1):
        x = LF.picks(seed, 4096, Q)
        assert int(x.max()) < Q
    # … with zero weights at the first, a middle and the last triangle: never chosen, whatever x is
    pts, cells = LF.strip(9)
    cells = np.concatenate([[[0, 0, 1]], cells[:4], [[2, 3, 3]], cells[4:], [[1, 2, 3]]]).astype(np.int32)  # (the last: collinear, on the lower row)
    q, C, Q, _ = LF.weights(pts, cells)
    assert q[0] == 0 and q[5] == 0 and q[-1] == 0 and (q > 0).sum() == 9
    for x in (0, 1, int(C[3]) - 1, int(C[4]) - 1, int(C[4]), int(C[5]), Q - 1):
        t = int(np.searchsorted(C, np.uint64(x), side="right"))
        assert q[t] > 0 and int(C[t]) > x and (t == 0 or int(C[t - 1]) <= x)
    lf = LF.long_form(pts, cells, 2000, 3, vertex_ids=False)
    assert not np.isin(lf["cells"], [0, 5, 11]).any() and lf["info"][0] == 9.0
    # the largest product the pick can meet: h = 2^53 − 1, Q = 2^58 − 1
    assert (((1 << 53) - 1) * ((1 << 58) - 1)) >> 53 < (1 << 58) - 1


@pytest.mark.parametrize("seed", [5, 1024])
def test_triangles_are_drawn_in_proportion_to_their_areas(seed):
    """n = 4096 draws, p = q_0 / Q = 1/4 up to 2^-32: the count of triangle 0 is binomial with mean 1024 and σ = 27.7; 5σ = 139"""
    pts, cells = two_triangles()
    lf = LF.long_form(pts, cells, 4096, seed, vertex_ids=False)
    count = int((lf["cells"] == 0).sum())
    print("seed", seed, "count of triangle 0:", count)
    assert abs(count - 1024) <= 139
    assert lf["info"].tolist() == [2.0, 3.0, 3.0 * (5726623061.0 / 4294967296.0), 0.0]
    assert abs(lf["info"][2] - 4.0) <= 4.0 * 2.0 ** -31  # the surface area, 1 + 3, up to the quantisation


def test_barycentric_rows_and_points(pkg):
    _, target = pkg.data.load_femur_model_and_target(50)
    lf = LF.long_form(target.points, target.cells, 3000, 11, vertex_ids=False)
    w = lf["bary"]
    assert np.all(w >= 0.0) and np.all(np.abs(w.sum(axis=1) - 1.0) <= 2 * 2.0 ** -52)
    c = target.cells[lf["cells"]]
    a, b, cc = target.points[c[:, 0]], target.points[c[:, 1]], target.points[c[:, 2]]
    normal = np.cross(b - a, cc - a)
    normal = normal / np.linalg.norm(normal, axis=1)[:, None]
    extent = float(np.abs(target.points).max())
    assert np.all(np.abs(((lf["points"] - a) * normal).sum(axis=1)) <= 1e-12 * extent)
    # … and inside its triangle: the point is the weights' combination of the corners
    assert np.abs(lf["points"] - (w[:, 0:1] * a + w[:, 1:2] * b + w[:, 2:3] * cc)).max() <= 1e-12 * extent
    # the nearest vertex of a sample is at most as far as the triangle's nearest corner, and ties go to the lowest id
    ids = LF.nearest_vertices(target.points, lf["points"][:200])
    corner = np.min([LF.squared_distance(lf["points"][:200], x[:200]) for x in (a, b, cc)], axis=0)
    assert np.all(LF.squared_distance(lf["points"][:200], target.points[ids]) <= corner)
    twice = np.concatenate([target.points[:5], target.points[:5]])
    assert LF.nearest_vertices(twice, target.points[:5] + 1e-3).tolist() == [0, 1, 2, 3, 4]


def test_the_tree_sum_has_a_fixed_shape(pkg):
    assert LF.tree_mean(np.full(50000, 3.0)) == 3.0 and LF.tree_mean([1.0]) == 1.0
    tr = np.arange(1.0, 258.0)
    assert LF.tree_mean(tr) == (tr[:256].sum() + 257.0) / 257.0  # (whole numbers: exact in any order)
    femur, _, _ = pkg.data.load_femur_mesh("femur_reference")
    kernel = pkg.data.femur_kernel(femur)
    want = 10.0 * np.trace(kernel[0].A) + 24.0
    got = LF.total_variance(femur.points[:300], kernel)
    assert abs(got - want) <= 1e-12 * want


def test_symbols_header_and_signatures(pkg):
    nat = pkg._native
    header = open(os.path.join(ROOT, "include", "icp_proposal.h")).read()
    for word in ("icp_surface_samples_many(", "icp_kernel_total_variance_many(", "ICP_SURFACE_SAMPLES_ROUND_BYTES", "AN INTEGER WEIGHT",
                 "A TRIANGLE BELOW 2^-32 OF THE LARGEST IS NEVER DRAWN", "THE FIRST t WITH C_t > x", "EQUAL DISTANCES GO TO THE LOWEST ID"):
        assert word in header, word
    for name, n_args in (("icp_surface_samples_many", 14), ("icp_kernel_total_variance_many", 9)):
        assert hasattr(nat.lib(), name)
        res, args = nat.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args and args[1] is ctypes.c_int
    for fn in (pkg.surface_samples, pkg.total_variance, pkg.data.surface_samples, pkg.data.approx_total_variance, pkg.data.fit_samples):
        assert callable(fn)
    assert "variance.sum() / approx_total_variance(" in pkg.data.approx_total_variance.__doc__


class _NoNative:
    """stands in for the loaded library: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native {name} reached")


def test_the_python_layer_validates(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "lib", lambda: _NoNative())
    Mesh = pkg.data.TriangleMesh
    pts, cells = two_triangles()
    mesh = Mesh(pts, cells)
    far = pts.copy()
    far[1, 2] = 2.0 ** 61
    bad = [dict(meshes=[], counts=3, seeds=0), dict(meshes=[pts], counts=3, seeds=0), dict(meshes=[mesh], counts=0, seeds=0),
           dict(meshes=[mesh], counts=(1 << 24) + 1, seeds=0), dict(meshes=[mesh], counts=2.0, seeds=0), dict(meshes=[mesh], counts=3, seeds=-1),
           dict(meshes=[mesh], counts=3, seeds=2 ** 64), dict(meshes=[mesh, mesh], counts=[3], seeds=0),
           dict(meshes=[Mesh(pts, np.zeros((0, 3)))], counts=3, seeds=0), dict(meshes=[Mesh(far, cells)], counts=3, seeds=0),
           dict(meshes=[Mesh(pts, cells + 1)], counts=3, seeds=0), dict(meshes=[mesh], counts=3, seeds=0, vertex_ids=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            pkg.surface_samples(**kw)
    for kw in (dict(meshes=mesh, counts=3, seeds=0), dict(meshes=[mesh, mesh], counts=[1, 1 << 24], seeds=[0, 2 ** 64 - 1], vertex_ids=[True, False])):
        with pytest.raises(AssertionError, match="icp_surface_samples_many reached"):
            pkg.surface_samples(**kw)
    with pytest.raises(AssertionError, match="icp_surface_samples_many reached"):
        pkg.data.fit_samples(pkg.data.StatisticalMeshModel(pts, cells, 0 * pts, np.zeros((18, 1)), np.ones(1)), mesh, 5)
    kernel = pkg.data.femur_kernel(pts)
    w = np.ones(6)
    weighted = [pkg.data.BSplineKernelTerm(4.0, -2, np.eye(3), np.ones(99), 0.7, 0)]
    for kw in (dict(points_list=[], kernels=kernel), dict(points_list=[pts[:, :2]], kernels=kernel), dict(points_list=[pts], kernels=[]),
               dict(points_list=[pts, pts], kernels=[kernel]), dict(points_list=[pts], kernels=weighted),
               dict(points_list=[pts], kernels=kernel, point_weights=[[w, None, None]]),
               dict(points_list=[pts], kernels=weighted, point_weights=[[np.ones(5)]]), dict(points_list=[pts], kernels=weighted, point_weights=[[0 * w]])):
        with pytest.raises(ValueError):
            pkg.total_variance(**kw)
    for kw in (dict(points_list=[pts, pts[:2]], kernels=kernel), dict(points_list=pts, kernels=[kernel]),
               dict(points_list=[pts], kernels=[weighted], point_weights=[[w]])):
        with pytest.raises(AssertionError, match="icp_kernel_total_variance_many reached"):
            pkg.total_variance(**kw)


def _items(n=3):
    pts, cells = two_triangles()
    return [LF.make(pts, cells, 4, seed=b) for b in range(n)]


def test_the_library_refuses_bad_arguments_before_touching_a_device(pkg):
    """every limit, in every item: ICP_ERR_INVALID_ARG per item and nothing written — also on a machine without a GPU, where touching
    the device would be ICP_ERR_DEVICE instead.  Then one item wrong among good ones: that item's status alone (where there is no device
    the good ones cannot run, the whole call is ICP_ERR_DEVICE and nothing is written)."""
    pts, cells = two_triangles()

    def moved(value, i=4, j=1):
        p = pts.copy()
        p[i, j] = value
        return LF.make(p, cells, 4)

    def tri(value):
        c = cells.copy()
        c[1, 2] = value
        return LF.make(pts, c, 4)

    good = LF.make(pts, cells, 4)
    M, T = 6, 2
    cases = [dict(item=moved(np.inf)), dict(item=moved(-np.inf)), dict(item=moved(np.nan)), dict(item=moved(2.0 ** 61)),
             dict(item=moved(-2.0 ** 60 * (1 + 2.0 ** -52), 5, 2)), dict(item=tri(6)), dict(item=tri(-1)),
             dict(sizes=(0, T, 4)), dict(sizes=(-1, T, 4)), dict(sizes=((1 << 24) + 1, T, 4)), dict(sizes=(M, 0, 4)), dict(sizes=(M, -1, 4)),
             dict(sizes=(M, (1 << 26) + 1, 4)), dict(sizes=(M, T, 0)), dict(sizes=(M, T, -2)), dict(sizes=(M, T, (1 << 24) + 1))]
    for kw in cases:
        item, sizes = kw.get("item", good), kw.get("sizes", (M, T, 4))
        rc, got = LF.raw_call(pkg, [item] * 2, counts=[sizes] * 2, expect=(-1,))
        assert all(g["status"] == -1 and LF.untouched(g) for g in got), kw
        assert b"outside the limits" in pkg._native.lib().icp_last_error()
        rc, got = LF.raw_call(pkg, [good, item, good], counts=[(M, T, 4), sizes, (M, T, 4)], expect=(-1, -2))
        assert LF.untouched(got[1]), kw
        if rc == -1:
            assert [g["status"] for g in got] == [0, -1, 0], kw
            lf = LF.long_form(pts, cells, 4, 0)
            LF.assert_item(got[0], lf, kw)
            LF.assert_item(got[2], lf, kw)
        else:
            assert all(g["status"] == 99 and LF.untouched(g) for g in got), kw
    # whole-call errors: nothing is written, status included
    for kw in (dict(n_items=0), dict(n_items=-3), dict(n_items=65536), dict(status=False), dict(whole_null=LF.OUTPUTS)):
        rc, got = LF.raw_call(pkg, _items(), expect=(-1,), **kw)
        assert all(g["status"] == 99 and LF.untouched(g) for g in got), kw
    assert b"null argument" in pkg._native.lib().icp_last_error()


def test_total_variance_refuses_bad_arguments_before_touching_a_device(pkg):
    nat, lib = pkg._native, pkg._native.lib()
    dp, ip = nat.c_double_p, nat.c_int_p
    pts, _ = two_triangles()

    def call(points=pts, n=6, n_terms=1, weights=None, n_items=2, status=True, out=True, **term):
        k = (nat.KernelTermGeneral * 1)()
        k[0].struct_size, k[0].kind, k[0].scale, k[0].sigma = ctypes.sizeof(nat.KernelTermGeneral), 0, 1.0, 10.0
        k[0].A[:] = np.eye(3).reshape(-1).tolist()
        for name, v in term.items():
            setattr(k[0], name, v)
        m = max(n_items, 1)
        p = np.ascontiguousarray(points, dtype=np.float64)
        res, st = np.full(m, 7.0), np.full(m, 99, dtype=np.int32)
        pw = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            one = (dp * 1)(w.ctypes.data_as(dp))
            pw = (ctypes.POINTER(dp) * m)(*[ctypes.cast(one, ctypes.POINTER(dp))] * m)
        rc = lib.icp_kernel_total_variance_many(n_items, 0, np.full(m, n, dtype=np.int32).ctypes.data_as(ip), (dp * m)(*[p.ctypes.data_as(dp)] * m),
                                                np.full(m, n_terms, dtype=np.int32).ctypes.data_as(ip),
                                                (ctypes.POINTER(nat.KernelTermGeneral) * m)(*[ctypes.cast(k, ctypes.POINTER(nat.KernelTermGeneral))] * m),
                                                pw, res.ctypes.data_as(dp) if out else None, st.ctypes.data_as(ip) if status else None)
        return rc, st, res

    bad_point = pts.copy()
    bad_point[2, 0] = np.nan
    for kw in (dict(n=0), dict(n=-1), dict(n=(1 << 24) + 1), dict(points=bad_point), dict(n_terms=0), dict(n_terms=9), dict(struct_size=8),
               dict(kind=2), dict(scale=0.0), dict(sigma=0.0), dict(sigma=np.inf), dict(kind=1, level=33), dict(kind=1, level=30),
               dict(mirror_gain=1.5), dict(mirror_axis=3), dict(weights=-np.ones(6)), dict(weights=np.zeros(6)),
               dict(weights=np.array([1.0, np.nan, 1, 1, 1, 1]))):
        rc, st, res = call(**kw)
        assert rc == -1 and np.all(st == -1) and np.all(res == 7.0), kw
    assert b"outside the limits" in lib.icp_last_error()
    for kw in (dict(n_items=0), dict(n_items=65536), dict(status=False), dict(out=False)):
        rc, st, res = call(**kw)
        assert rc == -1 and np.all(st == 99) and np.all(res == 7.0), kw
