"""dev: the scoring leg of the femur study (apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:43-64, appendExperiment): femur-200
(rank 201), 300 thetas from random_initial_parameters, against the bundled target and against data.synthetic_femur_target() (58,322
vertices).  Three ways per target:
  (a) one icp_mesh_metrics call per item (avg, hausdorff, the boundary-aware pair; no Dice);
  (b) icp_mesh_metrics_many, every item in one call, dice_samples = 0;
  (c) the same with dice_samples = 10,000.
Warm-up first; host clock around synchronised calls (each entry point returns after its final synchronisation).  Prints one JSON line:
items/s of each way per target, the speed-ups of (b) and (c) over (a), and whether (b)'s slots 0-4 equal (a)'s bit for bit.
  --only-c   time (c) alone (for a kernel-trace run of the batched path)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()


def best(fn, reps):
    ts, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=300)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-c", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model, bundled = pkg.data.load_femur_model_and_target(200)
    _, big = pkg.data.synthetic_femur_target()
    n = a.items
    th = np.stack([pkg.random_initial_parameters(model, i) for i in range(n)])
    res = {"items": n, "rank": model.rank, "dice_samples": a.samples}
    for name, target in (("bundled", bundled), ("synthetic58k", big)):
        ctx = pkg.IcpContext(model, target, device=0)
        run_b = lambda: pkg.registration_metrics(ctx, th, dice_samples=0)  # noqa: E731
        run_c = lambda: pkg.registration_metrics(ctx, th, dice_samples=a.samples, seed=1024)  # noqa: E731
        run_c()  # warm-up (module loads, pools, the target's Dice geometry)
        t_c, _ = best(run_c, a.repeats)
        r = {"target_vertices": target.n_points, "items_per_s_c": n / t_c}
        if not a.only_c:
            run_b()
            pkg.evaluate_reconstruction_to_ground_truth(ctx, th[0])
            t_b, mb = best(run_b, a.repeats)

            def run_a():
                return [pkg.evaluate_reconstruction_to_ground_truth(ctx, th[b]) for b in range(n)]
            t_a, ma = best(run_a, 1)
            same = all(np.array_equal([ma[b]["average2surface"], ma[b]["hausdorff"], ma[b]["average2surface_boundary_aware"],
                                       ma[b]["max_boundary_aware"], ma[b]["kept"]],
                                      [mb["avg"][b], mb["hausdorff"][b], mb["average2surface_boundary_aware"][b], mb["max_boundary_aware"][b],
                                       mb["kept"][b]], equal_nan=True) for b in range(n))
            r.update({"items_per_s_a": n / t_a, "items_per_s_b": n / t_b, "speedup_b_over_a": t_a / t_b, "speedup_c_over_a": t_a / t_c,
                      "b_equals_a_bitwise": bool(same)})
        res[name] = r
        ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
