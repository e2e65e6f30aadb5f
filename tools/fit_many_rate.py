"""dev: the ICP leg of the femur study (apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:106-163 through IcpRegistration.fitting):
femur-200 (rank 201) against the bundled target, 100 inits from random_initial_parameters, all 1,622 model ids and 1,622 target samples,
iterationSeq (1e-15,), 100 iterations (101 recursions per fit).  Three ways:
  (a) one icp_fit_deterministic call per fit, ModelSampling throughout;
  (b) the one-fit path driven recursion by recursion (n_iterations = 0), ModelAndTargetSampling with a seeded schedule;
  (c) icp_fit_deterministic_many, every fit in one call, the same schedule.
Warm-up first; host clock around synchronised calls (each entry point returns after its final synchronisation).  Prints one JSON line:
fits/s of each way, ms per recursion of (c), the speed-up of (c) over (a) and (b), and max |Δθ| between (b) and (c) on the fits (b) ran.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fits", type=int, default=100)
    ap.add_argument("--fits-b", type=int, default=10, help="fits that way (b) runs (it is slow); its rate is per fit")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-c", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model, target = pkg.data.load_femur_model_and_target(200)
    ctx = pkg.IcpContext(model, target, device=0)
    n, n_it, seq = a.fits, a.iterations, (1e-15,)
    R = len(seq) * (n_it + 1)
    ids = np.arange(model.n_points, dtype=np.int32)
    tps = target.points.copy()
    th0 = np.stack([pkg.random_initial_parameters(model, i) for i in range(n)])
    dirs = pkg.direction_schedule(n, R, seed=1024)

    def run_c():
        out, st = pkg.icp_fits(ctx, th0, n_it, seq, pkg.ModelAndTargetSampling, ids, tps, directions=dirs)
        assert np.all(st == 0), st
        return out

    def run_a(b):
        fit = pkg.IcpBasedSurfaceFitting(ctx, 1.0, pkg.ModelSampling, ids, tps)
        return fit.runfitting(n_it, seq, th0[b])

    def run_b(b):
        th = th0[b].copy()
        for rec in range(R):
            fit = pkg.IcpBasedSurfaceFitting(ctx, 1.0, pkg.ModelSampling if dirs[b, rec] == 0 else pkg.TargetSampling, ids, tps)
            th = fit.runfitting(0, (seq[rec // (n_it + 1)],), th)
        return th

    def best(fn, reps):
        ts = []
        res = None
        for _ in range(reps):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        return min(ts), res

    # warm-up: every path once (module loads, pools, first-launch costs)
    run_c()
    if a.only_c:
        t_c, _ = best(run_c, a.repeats)
        res = {"fits": n, "recursions": R, "fits_per_s_c": n / t_c, "ms_per_recursion_c": 1e3 * t_c / R}
    else:
        run_a(0)
        run_b(0)
        t_c, out_c = best(run_c, a.repeats)
        t_a, _ = best(lambda: [run_a(b) for b in range(n)], 1)
        nb = min(a.fits_b, n)
        t_b, out_b = best(lambda: [run_b(b) for b in range(nb)], 1)
        d = max(float(np.abs(out_b[b][10:] - out_c[b][10:]).max()) for b in range(nb))
        scale = max(float(np.abs(out_c[b][10:]).max()) for b in range(nb))
        fa, fb, fc = n / t_a, nb / t_b, n / t_c
        res = {"fits": n, "recursions": R, "fits_b": nb,
               "fits_per_s_a": fa, "fits_per_s_b": fb, "fits_per_s_c": fc,
               "ms_per_recursion_a": 1e3 * t_a / (n * R), "ms_per_recursion_b": 1e3 * t_b / (nb * R), "ms_per_recursion_c": 1e3 * t_c / R,
               "speedup_c_over_a": fc / fa, "speedup_c_over_b": fc / fb, "max_abs_dtheta_b_c": d, "max_abs_theta": scale}
    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
