"""dev: the model-projection legs of the femur study (model.coefficients(best mesh) of apps/femur/
StdIcpVsChainICPrandomInitComparisonAll.scala:53-55; the instancing loops of ReplayFittingFromLog / RandomSamplesFromModel).  Cases:
  (a) instances: 300 femur-200 states in one transformed_meshes call (icp_model_instances_many) against one
      IcpContext.transformedMesh (icp_transformed_mesh) per state;
  (b) coefficients of 300 femur-200 states, given as thetas and as points, in one model_coefficients call
      (icp_model_coefficients_many) against what the library offered before: transformedMesh per state, then the long form
      np.linalg.solve(QᵀQ + σ²I, Qᵀ(x − x̄ − μ)) on the host (QᵀQ + σ²I and Q made once, outside the timed part);
  (c) the same for 100 items of the face stand-in (N = 28,561, rank 200).
Warm-up of both ways first; then `--repeats` timed runs of each, interleaved; host clock around the calls (each entry point returns
after its final synchronisation).  Prints one JSON line: per case items/s as median [min, max] of both ways, the ratio of the medians,
whether the batched and the one-item forms agree bit for bit, and the largest difference from the long form.
  --only-batched   time the batched way alone (for a kernel-trace or counter run)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
SIGMA2 = 1e-5


def states(model, rng, n):
    th = np.tile(pkg.initial_parameters(model), (n, 1))
    th[:, 10:] = np.sqrt(0.1) * rng.normal(size=(n, model.rank))
    return th


def timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return time.perf_counter() - t0, res


def rate(n, ts):
    r = sorted(n / t for t in ts)
    return {"median": float(np.median(r)), "min": r[0], "max": r[-1]}


def compare(n, batched, yardstick, repeats, only_batched, equal):
    got = batched()  # warm-up (code objects, pools)
    r = {}
    if only_batched:
        r["batched_items_per_s"] = rate(n, [timed(batched)[0] for _ in range(repeats)])
        return r, got
    want = yardstick()
    tb, ty = [], []
    for _ in range(repeats):
        tb.append(timed(batched)[0])
        ty.append(timed(yardstick)[0])
    r["batched_items_per_s"], r["yardstick_items_per_s"] = rate(n, tb), rate(n, ty)
    r["ratio_of_medians"] = r["batched_items_per_s"]["median"] / r["yardstick_items_per_s"]["median"]
    r.update(equal(got, want))
    return r, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only-batched", action="store_true")
    ap.add_argument("--skip-face", action="store_true")
    ap.add_argument("--only-face", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    cases = []
    if not a.only_face:
        femur, target = pkg.data.load_femur_model_and_target(200)
        cases.append(("femur200_300", femur, target, 300))
    if not a.skip_face:
        face = pkg.data.synthetic_face_model(grid=169, rank=200)
        cases.append(("face_100", face, pkg.data.synthetic_partial_target(face), 100))
    res = {"repeats": a.repeats, "host_threads": os.environ.get("OMP_NUM_THREADS")}
    for name, model, tgt, n in cases:
        ctx = pkg.IcpContext(model, tgt, device=0)
        th = states(model, rng, n)
        Q = model.basis * np.sqrt(model.variance)[None, :]
        A = Q.T @ Q + SIGMA2 * np.eye(model.rank)
        off = model.ref_points + model.mean_def

        def long_form(x):
            return np.linalg.solve(A, Q.T @ (x - off).reshape(-1))

        shape = {"items": n, "vertices": model.n_points, "rank": model.rank}
        if name.startswith("femur"):
            r, meshes = compare(n, lambda: pkg.transformed_meshes(ctx, th), lambda: np.stack([ctx.transformedMesh(t) for t in th]),
                                a.repeats, a.only_batched, lambda x, y: {"bits_equal": bool(np.array_equal(x, y))})
            res[f"a_instances_{name}"] = {**shape, **r}
        else:
            meshes = pkg.transformed_meshes(ctx, th)
        mesh_list = list(meshes)

        def against_host(x, y):
            one = ctx.coefficients(meshes[n // 2])
            return {"one_item_bits_equal": bool(np.array_equal(x[n // 2], one)), "max_abs_diff_from_long_form": float(np.abs(x - y).max())}

        r, _ = compare(n, lambda: pkg.model_coefficients(ctx, thetas=list(th)),
                       lambda: np.stack([long_form(ctx.transformedMesh(t)) for t in th]), a.repeats, a.only_batched, against_host)
        res[f"b_coefficients_thetas_{name}"] = {**shape, **r}
        r, _ = compare(n, lambda: pkg.model_coefficients(ctx, meshes=mesh_list),
                       lambda: np.stack([long_form(x) for x in mesh_list]), a.repeats, a.only_batched, against_host)
        res[f"b_coefficients_points_{name}"] = {**shape, **r}
        ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
