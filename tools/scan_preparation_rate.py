"""dev: target preparation (icp_scans_prepare_many) at three sizes — 50 copies of the bundled femur target (1,622 vertices), 10 scans of
data.synthetic_femur_target() (58,322) and 10 scans of an 8-way subdivision (103,682) — each with the femur landmark alignment, one
cut of 1,000 vertices around a landmark and a mask list of 300 ids, three ways:
  (a) one batched prepare_scans call; (b) one prepare_scans call per item; (c) the numpy long form (tests/scan_preparation_long_form.py).
Warm-up first, then --repeats interleaved repeats of the three; host clock around synchronised calls.  Prints one JSON line: scans/s
as median [min, max] per way, the ratios of the medians, and whether all three deliver the same arrays bit for bit."""
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
import scan_preparation_long_form as LF  # noqa: E402

pkg = g.load_package()


def rates(n, ts):
    r = sorted(n / t for t in ts)
    return {"median": float(np.median(r)), "min": r[0], "max": r[-1]}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, lf):
    pairs = ((got["aligned"].points, lf["aligned"]), (got["landmarks"], lf["landmarks"]), (got["cut_flags"], lf["cut_flags"]),
             (got["kept_ids"], lf["kept_ids"]), (got["partial"].points, lf["partial_points"]), (got["partial"].cells, lf["partial_cells"]))
    return all(a.shape == b.shape and np.array_equal(bits(a), bits(b)) for a, b in pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="femur,synthetic58k,subdivided8")
    ap.add_argument("--only-batched", action="store_true", help="warm-up and --repeats batched calls alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _, ref_ids, ref_lms = pkg.data.load_femur_mesh("femur_reference")
    raw, tgt_ids, tgt_lms = pkg.data.load_femur_mesh("femur_target")
    scan_lms = dict(zip(tgt_ids, np.asarray(tgt_lms, dtype=np.float64)))
    tf = pkg.data.landmark_alignment(scan_lms, dict(zip(ref_ids, np.asarray(ref_lms, dtype=np.float64))))
    lms = np.asarray([scan_lms[k] for k in scan_lms])
    rng = np.random.Generator(np.random.PCG64(1024))

    def scan(n_subdiv):  # the RAW target subdivided and jittered (synthetic_femur_target's recipe, in front of the alignment)
        big = pkg.data.subdivide(raw, n_subdiv) if n_subdiv > 1 else raw
        return pkg.data.TriangleMesh(big.points + rng.normal(0.0, 0.05, size=big.points.shape), big.cells)

    cases = {"femur": (50, 1), "synthetic58k": (10, 6), "subdivided8": (10, 8)}
    res = {"repeats": a.repeats, "cut": 1000, "mask_ids": 300, "numpy_threads": os.environ.get("OMP_NUM_THREADS")}
    for name in a.cases.split(","):
        n, sub = cases[name]
        mesh = scan(sub)
        M = mesh.n_points
        mask = (np.arange(300, dtype=np.int64) * 7919) % M
        scans = [mesh] * n
        run_a = lambda: pkg.prepare_scans(scans, tf, lms, [(0, 1000)], mask)  # noqa: E731
        run_b = lambda: [pkg.prepare_scans(m, tf, lms, [(0, 1000)], mask)[0] for m in scans]  # noqa: E731
        run_c = lambda: [LF.long_form(m.points, m.cells, tf.pre_scale, tf.rotation, tf.centre, tf.translation, lms, [(0, 1000)], mask)  # noqa: E731
                         for m in scans]
        if a.only_batched:
            for _ in range(1 + a.repeats):
                run_a()
            continue
        run_a(); run_b(); run_c()  # warm-up
        ta, tb, tc = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter(); ra = run_a(); ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); rb = run_b(); tb.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); rc = run_c(); tc.append(time.perf_counter() - t0)
        res[name] = {"scans": n, "vertices": M, "triangles": mesh.n_cells, "kept_vertices": int(ra[0]["partial"].n_points),
                     "scans_per_s_batched": rates(n, ta), "scans_per_s_per_item": rates(n, tb), "scans_per_s_long_form": rates(n, tc),
                     "batched_over_per_item": float(np.median(tb) / np.median(ta)), "batched_over_long_form": float(np.median(tc) / np.median(ta)),
                     "all_three_equal_bitwise": bool(all(same(x, z) and same(y, z) for x, y, z in zip(ra, rb, rc)))}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
