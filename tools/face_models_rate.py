"""dev: Gaussian-process shape models from the face kernel (gp_models / icp_gp_models_general_many; what apps/bfm/CreateGPModel.scala
makes): five cubic B-spline terms, smoothed region weights, mirrored about x = 0.  tools/gp_models_rate.py's method.  Cases:
  face45   the mesh of synthetic_face_model(grid=45) (N = 2,025: the reference builds its face model on about 2,000 vertices) x 200 pivots;
  face169  the stand-in's own mesh (N = 28,561) x 256 pivots.
The mask is -4 where x lies in the lowest 30 % of the mesh, else 3: levels -3 and -2 carry weights below 1 there.
Three ways, 8 items each: one batched call, one call per item, and the numpy long form (tests/face_kernel_long_form.py) at the box's
thread count — timed on `--host-items` items and `--host-repeats` runs (for face169 one item, once, without a warm-up: it takes the
better part of a minute), its rate per item all the same.  Every way delivers variance, basis, pivots and residual per item.  Warm-up
of the device ways first; then `--repeats` timed runs of each, interleaved; host clock around the calls.  The region weights call
(icp_region_weights_many, five levels in one call) is timed the same way.  Prints one JSON line.
  --only-batched   time the batched way alone (for a kernel-trace run)
  --kernel femur   the femur kernel on the same meshes and pivots instead (the plain pivot step, for the kernel-trace comparison)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402
import face_kernel_long_form as F  # noqa: E402

pkg = g.load_package()
ITEMS = 8


def timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return time.perf_counter() - t0, res


def rate(n, ts):
    r = sorted(n / t for t in ts)
    return {"median": float(np.median(r)), "min": r[0], "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only-batched", action="store_true")
    ap.add_argument("--cases", default="face45,face169")
    ap.add_argument("--kernel", default="face", choices=("face", "femur"))
    ap.add_argument("--host-items", type=int, default=1)
    ap.add_argument("--host-repeats", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_models_rate.json"))
    a = ap.parse_args()
    all_cases = {"face45": (45, 200), "face169": (169, 256)}
    res = {"repeats": a.repeats, "host_threads": os.environ.get("OMP_NUM_THREADS"), "kernel": a.kernel}
    for name in a.cases.split(","):
        grid, m = all_cases[name]
        face = pkg.data.synthetic_face_model(grid=grid, rank=1)
        mesh = pkg.data.TriangleMesh(face.ref_points, face.cells)
        mask = pkg.data.FaceMask(np.where(mesh.points[:, 0] < np.quantile(mesh.points[:, 0], 0.3), -4, 3))
        R = 3 * mesh.n_points
        r = {"items": ITEMS, "vertices": mesh.n_points, "pivots": m, "basis_out_bytes_per_item": R * m * 8}
        weights = lambda: pkg.face_kernel(mesh, mask)  # noqa: E731
        terms = weights()
        if a.kernel == "face":
            # the items differ (a scale of their own on the finest term), as the meshes of a study would
            kernels = [terms[:4] + [pkg.data.BSplineKernelTerm(4.0 + 0.1 * b, -2, np.eye(3), terms[4].weights, 0.7, 0)] for b in range(ITEMS)]
            long_form = F.long_form
        else:
            import gp_model_long_form as LF
            ft = pkg.data.femur_kernel(mesh)
            kernels = [ft[:2] + [pkg.data.GaussianKernelTerm(3.0 + 0.1 * b, 10.0)] for b in range(ITEMS)]
            long_form = LF.long_form
        batched = lambda: pkg.gp_models([mesh] * ITEMS, kernels, m)  # noqa: E731
        per_item = lambda: [pkg.gp_model(mesh, kernels[b], m) for b in range(ITEMS)]  # noqa: E731
        host = lambda: [long_form(mesh.points, kernels[b], m) for b in range(a.host_items)]  # noqa: E731
        got = batched()
        r["effective_pivots"] = [i["n_pivots"] for _, i in got]
        if a.only_batched:
            r["batched_items_per_s"] = rate(ITEMS, [timed(batched)[0] for _ in range(a.repeats)])
        else:
            big = name == "face169"
            host_repeats = a.host_repeats if a.host_repeats is not None else (1 if big else a.repeats)
            one = per_item()
            if not big:
                host()
            tb, to, th, tw = [], [], [], []
            for k in range(a.repeats):
                tb.append(timed(batched)[0])
                to.append(timed(per_item)[0])
                tw.append(timed(weights)[0])
                if k < host_repeats:
                    th.append(timed(host)[0])
            r["batched_items_per_s"], r["one_call_per_item_items_per_s"] = rate(ITEMS, tb), rate(ITEMS, to)
            r["numpy_long_form_items_per_s"] = rate(a.host_items, th)
            r["host_items_timed"], r["host_repeats"], r["host_warm_up"] = a.host_items, host_repeats, not big
            r["region_weights_five_levels_ms"] = {"median": 1e3 * float(np.median(tw)), "min": 1e3 * min(tw), "max": 1e3 * max(tw)}
            r["batched_over_one_call_per_item"] = r["batched_items_per_s"]["median"] / r["one_call_per_item_items_per_s"]["median"]
            r["batched_over_numpy_long_form"] = r["batched_items_per_s"]["median"] / r["numpy_long_form_items_per_s"]["median"]
            r["one_item_bits_equal"] = bool(all(np.array_equal(x[0].basis, y[0].basis) and np.array_equal(x[1]["variance"], y[1]["variance"])
                                                and np.array_equal(x[1]["pivots"], y[1]["pivots"]) for x, y in zip(got, one)))
            if not big:
                lf = long_form(mesh.points, kernels[0], m, pivots=got[0][1]["pivots"])
                r["max_rel_diff_of_variance_from_long_form"] = float(np.abs(got[0][1]["variance"] - lf["variance"]).max() / lf["variance"][0])
            r["share_of_trace_explained"] = got[0][1]["approximated_variance"] / got[0][1]["total_variance"]
        res[name] = r
        print(name, json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
