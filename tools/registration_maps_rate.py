"""dev: the per-vertex leg of the femur study: femur-200 (rank 201), 300 states from random_initial_parameters, against the bundled
target and against data.synthetic_femur_target() (58,322 vertices).
  maps       (a) the per-state route: transformedMesh, closestPointOnTarget, [closestTargetVertex where the target has a boundary,]
                 closestPointOnModel, square roots and flags in numpy;
             (b) icp_registration_maps_many, every state in one call, every output.
  summaries  200 sets of 20 states (bundled target; --sets-big of them on the 58k target):
             (a) the per-state route of every state plus the numpy fold; (b) icp_distance_summaries_many.
Warm-up first, then --repeats alternating repeats of each way; host clock around synchronised calls.  Prints one JSON line: items/s
(maps) and sets/s (summaries) as median [min, max], the ratio of the medians, and whether (b) equals (a) bit for bit."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()


def per_state(ctx, target, flags, theta):
    x = ctx.transformedMesh(theta)
    cp, tri, d2 = ctx.closestPointOnTarget(x)
    onb = np.zeros(x.shape[0], dtype=np.uint8)
    if flags is not None:
        idx, _ = ctx.closestTargetVertex(cp)
        onb = flags[idx]
    cpt, trit, d2t = ctx.closestPointOnModel(theta, target.points)
    return {"m2t_point": cp, "m2t_triangle": tri, "m2t_distance": np.sqrt(d2), "m2t_on_boundary": onb, "t2m_point": cpt,
            "t2m_triangle": trit, "t2m_distance": np.sqrt(d2t)}


def fold(rows):
    acc = rows[0].copy()
    for row in rows[1:]:
        acc = acc + row
    return acc / len(rows), np.max(rows, axis=0)


def alternate(fa, fb, reps):
    ta, tb, ra, rb = [], [], None, None
    for _ in range(reps):
        t0 = time.perf_counter(); ra = fa(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); rb = fb(); tb.append(time.perf_counter() - t0)
    return ta, tb, ra, rb


def rates(n, ts):
    r = sorted(n / t for t in ts)
    return {"median": float(np.median(r)), "min": r[0], "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=300)
    ap.add_argument("--sets", type=int, default=200)
    ap.add_argument("--sets-big", type=int, default=10)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model, bundled = pkg.data.load_femur_model_and_target(200)
    _, big = pkg.data.synthetic_femur_target()
    n = a.items
    th = np.stack([pkg.random_initial_parameters(model, i) for i in range(n)])
    res = {"items": n, "rank": model.rank, "repeats": a.repeats, "samples_per_set": a.samples}
    for name, target, n_sets in (("bundled", bundled, a.sets), ("synthetic58k", big, a.sets_big)):
        ctx = pkg.IcpContext(model, target, device=0)
        f = np.asarray(pkg.data.boundary_vertex_flags(target)).astype(np.uint8)
        flags = f if f.any() else None
        run_a = lambda: [per_state(ctx, target, flags, t) for t in th]  # noqa: E731
        run_b = lambda: pkg.registration_maps(ctx, th)  # noqa: E731
        run_b(); per_state(ctx, target, flags, th[0])  # warm-up
        ta, tb, ma, mb = alternate(run_a, run_b, a.repeats)
        same = all(np.array_equal(ma[b][k], mb[b][k]) for b in range(n) for k in ma[b])
        r = {"target_vertices": target.n_points, "maps_items_per_s_a": rates(n, ta), "maps_items_per_s_b": rates(n, tb),
             "maps_b_over_a": float(np.median(ta) / np.median(tb)), "maps_b_equals_a_bitwise": bool(same)}
        sets = [th[(np.arange(a.samples) + 7 * m) % n] for m in range(n_sets)]

        def sum_a():
            out = []
            for s in sets:
                maps = [per_state(ctx, target, None, t) for t in s]
                out.append(fold([v["m2t_distance"] for v in maps]) + fold([v["t2m_distance"] for v in maps]))
            return out
        sum_b = lambda: pkg.distance_summaries(ctx, sets)  # noqa: E731
        sum_b()
        ta, tb, sa, sb = alternate(sum_a, sum_b, a.repeats)
        same = all(np.array_equal(sa[m][i], sb[m][k]) for m in range(n_sets) for i, k in enumerate(("m2t_mean", "m2t_max", "t2m_mean", "t2m_max")))
        r.update({"summary_sets": n_sets, "summaries_sets_per_s_a": rates(n_sets, ta), "summaries_sets_per_s_b": rates(n_sets, tb),
                  "summaries_b_over_a": float(np.median(ta) / np.median(tb)), "summaries_b_equals_a_bitwise": bool(same)})
        res[name] = r
        ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
