"""dev: re-scoring the states of a log under an evaluator, against data.synthetic_femur_target() (58,322 vertices).  Three legs:
  (i)   femur-50, independent point distance evaluator, K_e = 204, model -> target, 10,000 states;
  (ii)  the same with the symmetric mode;
  (iii) femur-200 (rank 201), Hausdorff evaluator, 300 states.
The states are a seeded walk from the mean shape (small steps in the coefficients and the pose, as a chain's accepted states follow
each other), pairwise distinct, so that no call of (a) meets the evaluator's memo.  Two ways per leg:
  (a) one icp_evaluator_log_value call per state;
  (b) ONE icp_evaluator_log_values_many call.
Warm-up first; host clock around synchronised calls (each entry point returns after its final synchronisation); medians of
--repeats runs, (a) and (b) alternating.  Prints one JSON line: items/s of each way per leg, the ratio, and whether (b)'s values equal
(a)'s bit for bit.
  --only-b   run (b) alone (for a kernel-trace run of the batched path)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()


def walk(model, n, seed):
    rng = np.random.default_rng(seed)
    th = np.tile(pkg.initial_parameters(model), (n, 1))
    th[:, 10:] = np.cumsum(0.02 * rng.normal(size=(n, model.rank)), axis=0)
    th[:, 1:4] = np.cumsum(0.01 * rng.normal(size=(n, 3)), axis=0)
    th[:, 4:7] = np.cumsum(0.0005 * rng.normal(size=(n, 3)), axis=0)
    assert len({t.tobytes() for t in th}) == n
    return th


def timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=10000)
    ap.add_argument("--hausdorff-states", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--legs", default="i,ii,iii")
    ap.add_argument("--only-b", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _, big = pkg.data.synthetic_femur_target()
    res = {"target_vertices": big.n_points, "repeats": a.repeats}
    legs = {"i": (50, "independent", pkg.ModelToTargetEvaluation, a.states), "ii": (50, "independent", pkg.SymmetricEvaluation, a.states),
            "iii": (200, "hausdorff", None, a.hausdorff_states)}
    for name in a.legs.split(","):
        size, kind, mode, n = legs[name]
        model, _ = pkg.data.load_femur_model_and_target(size)
        ctx = pkg.IcpContext(model, big, device=0)
        ev = (pkg.IndependentPointDistanceEvaluator(ctx, 0.0, 2.0, mode, 204) if kind == "independent"
              else pkg.HausdorffDistanceEvaluator(ctx, 1.0))
        th = walk(model, n, 11)
        run_b = lambda: pkg.log_values(ev, th)["value"]  # noqa: E731
        run_a = lambda: np.array([ev.logValue(t) for t in th])  # noqa: E731
        run_b()  # warm-up (module loads, pools)
        tb, ta, vb, va = [], [], None, None
        if not a.only_b:
            run_a()
        for _ in range(a.repeats):
            t, vb = timed(run_b)
            tb.append(t)
            if not a.only_b:
                t, va = timed(run_a)
                ta.append(t)
        r = {"model": f"femur-{size}", "evaluator": kind, "mode": mode, "states": n, "items_per_s_b": n / float(np.median(tb))}
        if not a.only_b:
            r.update({"items_per_s_a": n / float(np.median(ta)), "b_over_a": float(np.median(ta) / np.median(tb)),
                      "b_equals_a_bitwise": bool(np.array_equal(va, vb, equal_nan=True))})
        res[name] = r
        ev.close()
        ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
