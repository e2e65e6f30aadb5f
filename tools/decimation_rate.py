"""dev: mesh decimation (icp_decimate_many) at three sizes — 50 copies of the bundled femur target (1,622 vertices) at k = 102 and 400,
8 copies of synthetic_face_model()'s reference (28,561) at 500 and 2,000, 10 copies of data.synthetic_femur_target() (58,322) at
1,000 — three ways:
  (a) one batched decimated_meshes call; (b) one decimated_meshes call per item; (c) the numpy long form (tests/decimation_long_form.py).
With the test-hooks library loaded (ICP_LIBRARY_PATH) the femur cases are also timed with the general selection forced
(ICP_TEST_DECIMATE_GROUP_VERTICES=0): (a) against (a') measures the one-workgroup route.
Warm-up first, then --repeats interleaved repeats of the ways; host clock around synchronised calls.  Prints one JSON line: meshes/s as
median [min, max] per way, the ratios of the medians, and whether all ways deliver the same arrays bit for bit."""
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
import decimation_long_form as LF  # noqa: E402

pkg = g.load_package()
GENERAL = "ICP_TEST_DECIMATE_GROUP_VERTICES"


def rates(n, ts):
    r = sorted(n / t for t in ts)
    return {"median": float(np.median(r)), "min": r[0], "max": r[-1]}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, lf):
    return got["counts"] == lf["counts"] and all(got[k].shape == lf[k].shape and np.array_equal(bits(got[k]), bits(lf[k]))
                                                 for k in ("ids", "points", "cover2", "labels", "cells"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="femur102,femur400,face500,face2000,synthetic58k")
    ap.add_argument("--only-batched", action="store_true", help="warm-up and --repeats batched calls alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hooks = pkg._native.LIB_PATH.endswith("_testhooks.so")
    os.environ.pop(GENERAL, None)
    meshes = {"femur": lambda: pkg.data.load_femur_model_and_target(50)[1], "face": lambda: pkg.data.synthetic_face_model(rank=1).reference_mesh,
              "synthetic58k": lambda: pkg.data.synthetic_femur_target()[1]}
    cases = {"femur102": ("femur", 50, 102), "femur400": ("femur", 50, 400), "face500": ("face", 8, 500), "face2000": ("face", 8, 2000),
             "synthetic58k": ("synthetic58k", 10, 1000)}
    made = {}
    res = {"repeats": a.repeats, "numpy_threads": os.environ.get("OMP_NUM_THREADS"), "test_hooks_library": hooks}
    for name in a.cases.split(","):
        kind, n, k = cases[name]
        if kind not in made:
            made[kind] = meshes[kind]()
        mesh = made[kind]
        batch = [mesh] * n
        run_a = lambda: pkg.decimated_meshes(batch, k)  # noqa: E731
        run_b = lambda: [pkg.decimated_mesh(m, k) for m in batch]  # noqa: E731
        run_c = lambda: [LF.long_form(m.points, m.cells, k) for m in batch]  # noqa: E731

        def run_g():  # the general selection forced (test-hooks library)
            os.environ[GENERAL] = "0"
            try:
                return run_a()
            finally:
                os.environ.pop(GENERAL)

        forced = hooks and kind == "femur"
        if a.only_batched:
            for _ in range(1 + a.repeats):
                run_a()
                if forced:
                    run_g()
            continue
        run_a(); run_b(); run_c()  # warm-up
        if forced:
            run_g()
        ta, tb, tc, tg = [], [], [], []
        rg = None
        for _ in range(a.repeats):
            t0 = time.perf_counter(); ra = run_a(); ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); rb = run_b(); tb.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); rc = run_c(); tc.append(time.perf_counter() - t0)
            if forced:
                t0 = time.perf_counter(); rg = run_g(); tg.append(time.perf_counter() - t0)
        equal = all(same(x, z) and same(y, z) for x, y, z in zip(ra, rb, rc)) and (rg is None or all(same(x, z) for x, z in zip(rg, rc)))
        res[name] = {"meshes": n, "vertices": mesh.n_points, "triangles": mesh.n_cells, "k": k, "counts": list(ra[0]["counts"]),
                     "meshes_per_s_batched": rates(n, ta), "meshes_per_s_per_item": rates(n, tb), "meshes_per_s_long_form": rates(n, tc),
                     "batched_over_per_item": float(np.median(tb) / np.median(ta)), "batched_over_long_form": float(np.median(tc) / np.median(ta)),
                     "per_item_over_long_form": float(np.median(tc) / np.median(tb)), "all_ways_equal_bitwise": bool(equal)}
        if forced:
            res[name]["meshes_per_s_batched_general_selection"] = rates(n, tg)
            res[name]["one_workgroup_over_general_selection"] = float(np.median(tg) / np.median(ta))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
