"""dev: the variability-map leg of the femur study (apps/util/PosteriorVariability.scala:30-73 over every chain's sub-sampled log):
posterior_variability_maps (icp_posterior_variability_many, every map in one call) against the yardstick, one
posterior_variability call (icp_posterior_variability) per map in the same process.  Cases:
  (a) study size: femur-200 (rank 201), 200 maps of 20 samples, modes 0 and 2;
  (b) one femur-200 map of 200 samples, modes 0 and 2;
  (c) one face stand-in map (N = 28,561, rank 200) of 200 samples, mode 0.
Warm-up of both ways first; then `--repeats` timed runs of each, interleaved; host clock around the calls (each entry point returns
after its final synchronisation).  Prints one JSON line: per case maps/s as median [min, max] of both ways, the ratio of the medians,
and whether the bits agree.
  --only-batched   time the batched way alone (for a kernel-trace run)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()


def states(model, rng, S):
    th = np.tile(pkg.initial_parameters(model), (S, 1))
    th[:, 10:] = 0.3 * rng.normal(size=(S, model.rank))
    th[:, 1:4] = 0.5 * rng.normal(size=(S, 3))
    th[:, 4:7] = 0.01 * rng.normal(size=(S, 3))
    return th


def timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return time.perf_counter() - t0, res


def rate(n_maps, ts):
    r = sorted(n_maps / t for t in ts)
    return {"median": float(np.median(r)), "min": r[0], "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only-batched", action="store_true")
    ap.add_argument("--skip-face", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    femur, target = pkg.data.load_femur_model_and_target(200)
    cases = [("a_study_200x20", femur, target, 200, 20, (0, 2)), ("b_one_map_200", femur, target, 1, 200, (0, 2))]
    if not a.skip_face:
        face = pkg.data.synthetic_face_model(grid=169, rank=200)
        cases.append(("c_face_one_map_200", face, pkg.data.synthetic_partial_target(face), 1, 200, (0,)))
    res = {"repeats": a.repeats}
    for name, model, tgt, n_maps, S, modes in cases:
        ctx = pkg.IcpContext(model, tgt, device=0)
        sets = [states(model, rng, S) for _ in range(n_maps)]
        for mode in modes:
            batched = lambda: pkg.posterior_variability_maps(ctx, sets, mode=mode)  # noqa: E731
            one_by_one = lambda: [pkg.posterior_variability(ctx, th, mode=mode) for th in sets]  # noqa: E731
            got = batched()  # warm-up (code objects, pools)
            r = {"maps": n_maps, "samples": S, "vertices": model.n_points, "rank": model.rank}
            if a.only_batched:
                r["batched_maps_per_s"] = rate(n_maps, [timed(batched)[0] for _ in range(a.repeats)])
            else:
                want = one_by_one()
                tb, ty = [], []
                for _ in range(a.repeats):
                    tb.append(timed(batched)[0])
                    ty.append(timed(one_by_one)[0])
                r["batched_maps_per_s"], r["one_call_per_map_maps_per_s"] = rate(n_maps, tb), rate(n_maps, ty)
                r["ratio_of_medians"] = r["batched_maps_per_s"]["median"] / r["one_call_per_map_maps_per_s"]["median"]
                r["bits_equal"] = bool(all(np.array_equal(x, y) for x, y in zip(got, want)))
            res[f"{name}_mode{mode}"] = r
        ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
