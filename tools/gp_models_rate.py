"""dev: Gaussian-process shape models from analytic kernels by pivoted Cholesky (gp_models / icp_gp_models_many; what
apps/femur/CreateGPModel.scala makes).  Cases:
  femur reference (N = 1,622) with femur_kernel x {64, 128, 256} pivots, rank = pivots;
  the face-sized stand-in mesh (N = 28,561) with the same kernel family x 256 pivots.
Three ways, 8 items each: one batched call, one call per item, and the numpy long form (tests/gp_model_long_form.py) at the box's thread
count — for the face the long form is timed on `--face-host-items` items (default 1) and its rate is per item all the same.
Every way delivers variance, basis, pivots and residual per item.  Warm-up of all ways first; then `--repeats` timed runs of each,
interleaved; host clock around the calls (the entry point returns after its last synchronisation).  Prints one JSON line: per case
items/s as median [min, max] of each way, the ratios of the medians, whether the batched and the one-item forms agree bit for bit, the
largest relative difference of the variances from the long form run on the device's pivots, and the bytes of L the pivot loop reads.
  --only-batched   time the batched way alone (for a kernel-trace or counter run)"""
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
import gp_model_long_form as LF  # noqa: E402

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
    ap.add_argument("--skip-face", action="store_true")
    ap.add_argument("--skip-femur", action="store_true")
    ap.add_argument("--face-host-items", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_models_rate.json"))
    a = ap.parse_args()
    femur, _, _ = pkg.data.load_femur_mesh("femur_reference")
    cases = [] if a.skip_femur else [(f"femur_m{m}_x{ITEMS}", femur, m, ITEMS) for m in (64, 128, 256)]
    if not a.skip_face:
        face = pkg.data.synthetic_face_model(grid=169, rank=1)
        cases.append((f"face_m256_x{ITEMS}", pkg.data.TriangleMesh(face.ref_points, face.cells), 256, a.face_host_items))
    res = {"repeats": a.repeats, "host_threads": os.environ.get("OMP_NUM_THREADS")}
    for name, mesh, m, host_items in cases:
        terms = pkg.data.femur_kernel(mesh)
        # the items differ (a scale of their own on the finest term), as the meshes of a study would
        kernels = [terms[:2] + [pkg.data.GaussianKernelTerm(3.0 + 0.1 * b, 10.0)] for b in range(ITEMS)]
        batched = lambda: pkg.gp_models([mesh] * ITEMS, kernels, m)  # noqa: E731
        per_item = lambda: [pkg.gp_model(mesh, kernels[b], m) for b in range(ITEMS)]  # noqa: E731
        host = lambda: [LF.long_form(mesh.points, kernels[b], m) for b in range(host_items)]  # noqa: E731
        R = 3 * mesh.n_points
        r = {"items": ITEMS, "vertices": mesh.n_points, "pivots": m, "basis_out_bytes_per_item": R * m * 8,
             "pivot_loop_reads_of_L_bytes_per_item": 8 * R * m * (m - 1) // 2, "host_items_timed": host_items}
        got = batched()
        r["effective_pivots"] = [i["n_pivots"] for _, i in got]
        if a.only_batched:
            r["batched_items_per_s"] = rate(ITEMS, [timed(batched)[0] for _ in range(a.repeats)])
        else:
            one = per_item()
            host()
            tb, to, th = [], [], []
            for _ in range(a.repeats):
                tb.append(timed(batched)[0])
                to.append(timed(per_item)[0])
                th.append(timed(host)[0])
            r["batched_items_per_s"], r["one_call_per_item_items_per_s"] = rate(ITEMS, tb), rate(ITEMS, to)
            r["numpy_long_form_items_per_s"] = rate(host_items, th)
            r["batched_over_one_call_per_item"] = r["batched_items_per_s"]["median"] / r["one_call_per_item_items_per_s"]["median"]
            r["batched_over_numpy_long_form"] = r["batched_items_per_s"]["median"] / r["numpy_long_form_items_per_s"]["median"]
            r["one_item_bits_equal"] = bool(all(np.array_equal(x[0].basis, y[0].basis) and np.array_equal(x[1]["variance"], y[1]["variance"])
                                                and np.array_equal(x[1]["pivots"], y[1]["pivots"]) for x, y in zip(got, one)))
            lf = LF.long_form(mesh.points, kernels[0], m, pivots=got[0][1]["pivots"])
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
