"""dev: posterior shape models from correspondences (model.posterior(correspondences, noise) of api/other/IcpBasedSurfaceFitting.scala:81
as a model).  Cases:
  (a) femur-200 (N = 1,622, rank 201) x 100 landmark sets (12 pairs each, sigma2 = 1) in one posterior_models call
      (icp_posterior_models_many);
  (b) the face stand-in (N = 28,561, rank 200) x 16 items (600 observations each, sigma2 = 0.1).
Yardsticks: the numpy long form (np.linalg for M^-1 and the eigen-decomposition, Phi @ V, at the box's thread count) and one
icp_posterior_models_many call per item.  Every way delivers mean, basis, variance and point variances per item.
Warm-up of all ways first; then `--repeats` timed runs of each, interleaved; host clock around the calls (the entry point returns after
its final synchronisation).  Prints one JSON line: per case items/s as median [min, max] of each way, the ratios of the medians,
whether the batched and the one-item forms agree bit for bit, and the largest relative difference of S from the long form.
  --only-batched   time the batched way alone (for a kernel-trace or counter run)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
WANT = ("mean", "basis", "variance", "point_variance")


def long_form(model, Q, D, ids, y, sigma2):
    r, N = model.rank, model.n_points
    Qo = Q.reshape(N, 3, r)[ids].reshape(-1, r)
    M = np.eye(r) + (Qo.T @ Qo) / sigma2
    e = ((y - model.ref_points[ids]) - model.mean_def[ids]).reshape(-1)
    alpha = np.linalg.solve(M, Qo.T @ e / sigma2)
    Minv = np.linalg.inv(M)
    S, V = np.linalg.eigh(D[:, None] * (0.5 * (Minv + Minv.T)) * D[None, :])
    S, V = S[::-1], V[:, ::-1]
    basis = model.basis @ V
    pv = ((basis * basis) @ S).reshape(N, 3).sum(axis=1)
    return dict(mean=model.mean_def + (Q @ alpha).reshape(N, 3), basis=basis, variance=S, point_variance=pv)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_models_rate.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    femur, ftarget = pkg.data.load_femur_model_and_target(200)
    cases = [("femur200_x100_landmark_sets", femur, ftarget, 100, 12, 1.0)]
    if not a.skip_face:
        face = pkg.data.synthetic_face_model(grid=169, rank=200)
        cases.append(("face_x16", face, pkg.data.synthetic_partial_target(face), 16, 600, 0.1))
    res = {"repeats": a.repeats, "host_threads": os.environ.get("OMP_NUM_THREADS")}
    for name, model, tgt, n, k, s2 in cases:
        ctx = pkg.IcpContext(model, tgt, device=0)
        D = np.sqrt(model.variance)
        Q = model.basis * D[None, :]
        ids = [rng.choice(model.n_points, size=k, replace=False).astype(np.int32) for _ in range(n)]
        ys = [model.ref_points[i] + model.mean_def[i] + 2.0 * rng.normal(size=(k, 3)) for i in ids]
        batched = lambda: pkg.posterior_models(ctx, ids, ys, sigma2=[s2] * n, want=WANT)  # noqa: E731
        per_item = lambda: [pkg.posterior_models(ctx, [ids[b]], [ys[b]], sigma2=[s2], want=WANT)[0] for b in range(n)]  # noqa: E731
        host = lambda: [long_form(model, Q, D, ids[b], ys[b], s2) for b in range(n)]  # noqa: E731
        r = {"items": n, "vertices": model.n_points, "rank": model.rank, "observations": k, "basis_out_bytes_per_item": 3 * model.n_points * model.rank * 8}
        got = batched()
        if a.only_batched:
            r["batched_items_per_s"] = rate(n, [timed(batched)[0] for _ in range(a.repeats)])
        else:
            one, want = per_item(), host()
            tb, to, th = [], [], []
            for _ in range(a.repeats):
                tb.append(timed(batched)[0])
                to.append(timed(per_item)[0])
                th.append(timed(host)[0])
            r["batched_items_per_s"], r["one_call_per_item_items_per_s"], r["numpy_long_form_items_per_s"] = rate(n, tb), rate(n, to), rate(n, th)
            r["batched_over_one_call_per_item"] = r["batched_items_per_s"]["median"] / r["one_call_per_item_items_per_s"]["median"]
            r["batched_over_numpy_long_form"] = r["batched_items_per_s"]["median"] / r["numpy_long_form_items_per_s"]["median"]
            r["one_item_bits_equal"] = bool(all(np.array_equal(x[w], y[w]) for x, y in zip(got, one) for w in WANT))
            r["max_rel_diff_of_S_from_long_form"] = float(max(np.abs(x["variance"] - y["variance"]).max() / max(1.0, y["variance"].max())
                                                              for x, y in zip(got, want)))
        res[name] = r
        ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
