"""dev: PCA shape models from registered meshes with Procrustes alignment (pca_models / icp_pca_models_many).  Cases:
  femur leave-one-out: 50 posed instances of the femur model (N = 1,622), 50 items x 49 meshes over one pool;
  face: 8 items x 256 face-sized meshes (N = 28,561, instances of data.synthetic_face_model), item b = meshes b .. b + 255 of one pool.
Three ways: one batched call, one call per item, and the numpy long form (tests/pca_model_long_form.py) at the box's thread count — the
long form is timed on `--femur-host-items` / `--face-host-items` items and its rate is per item all the same.  Every way delivers
variance, basis, mean shape and transforms per item (3 rounds at most, halt_distance 1e-5).  Warm-up of all ways first; then `--repeats`
timed runs of each, interleaved; host clock around the calls (the entry point returns after its last synchronisation).  Prints one
JSON line: per case items/s as median [min, max] of each way, the ratios of the medians, whether the batched and the one-item forms
agree bit for bit, the largest relative difference of the variances from the long form, and the bytes a round of the alignment moves.
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
import pca_model_long_form as LF  # noqa: E402

pkg = g.load_package()
ROUNDS, HALT = 3, 1e-5


def timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return time.perf_counter() - t0, res


def rate(n, ts):
    r = sorted(n / t for t in ts)
    return {"median": float(np.median(r)), "min": r[0], "max": r[-1]}


def face_meshes(count, seed=5):
    """`count` instances of the face stand-in under small seeded rigid motions: one matrix product for all of them"""
    model = pkg.data.synthetic_face_model(grid=169, rank=200)
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(model.rank, count)) * np.sqrt(model.variance)[:, None]
    x = (model.ref_points + model.mean_def).reshape(-1, 1) + model.basis @ c
    out = []
    for j in range(count):
        m = x[:, j].reshape(-1, 3)
        R, centre = LF.random_rotation(rng, 0.05), m.mean(axis=0)
        out.append(np.ascontiguousarray((m - centre) @ R.T + centre + 2.0 * rng.normal(size=3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only-batched", action="store_true")
    ap.add_argument("--skip-face", action="store_true")
    ap.add_argument("--skip-femur", action="store_true")
    ap.add_argument("--femur-host-items", type=int, default=8)
    ap.add_argument("--face-host-items", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_models_rate.json"))
    a = ap.parse_args()
    cases = []
    if not a.skip_femur:
        meshes = LF.posed_instances(pkg.data.load_femur_model(50), 50, seed=50, noise=0.1)
        cases.append(("femur_leave_one_out_50x49", [meshes[:i] + meshes[i + 1:] for i in range(50)], a.femur_host_items))
    if not a.skip_face:
        meshes = face_meshes(256 + 7)
        cases.append(("face_8x256", [meshes[b:b + 256] for b in range(8)], a.face_host_items))
    res = {"repeats": a.repeats, "host_threads": os.environ.get("OMP_NUM_THREADS"), "rounds_at_most": ROUNDS, "halt_distance": HALT}
    for name, sets, host_items in cases:
        items, n, N = len(sets), len(sets[0]), sets[0][0].shape[0]
        batched = lambda: pkg.pca_models(sets, gpa_iterations=ROUNDS, halt_distance=HALT)  # noqa: E731
        per_item = lambda: [pkg.pca_model(s, gpa_iterations=ROUNDS, halt_distance=HALT) for s in sets]  # noqa: E731
        host = lambda: [LF.long_form(s, None, ROUNDS, HALT) for s in sets[:host_items]]  # noqa: E731
        r = {"items": items, "meshes_per_item": n, "vertices": N, "basis_out_bytes_per_item": 3 * N * (n - 1) * 8,
             "alignment_bytes_per_item_and_round": 8 * 3 * N * (6 * n + 3), "pool_meshes_uploaded": len({id(m) for s in sets for m in s}),
             "host_items_timed": host_items}
        got = batched()
        r["rounds"] = sorted({i["rounds"] for _, i in got})
        r["effective_ranks"] = sorted({i["rank"] for _, i in got})
        if a.only_batched:
            r["batched_items_per_s"] = rate(items, [timed(batched)[0] for _ in range(a.repeats)])
        else:
            one = per_item()
            lf = host()
            tb, to, th = [], [], []
            for _ in range(a.repeats):
                tb.append(timed(batched)[0])
                to.append(timed(per_item)[0])
                th.append(timed(host)[0])
            r["batched_items_per_s"], r["one_call_per_item_items_per_s"] = rate(items, tb), rate(items, to)
            r["numpy_long_form_items_per_s"] = rate(host_items, th)
            r["batched_over_one_call_per_item"] = r["batched_items_per_s"]["median"] / r["one_call_per_item_items_per_s"]["median"]
            r["batched_over_numpy_long_form"] = r["batched_items_per_s"]["median"] / r["numpy_long_form_items_per_s"]["median"]
            r["one_item_bits_equal"] = bool(all(np.array_equal(x[0].basis, y[0].basis) and np.array_equal(x[1]["variance"], y[1]["variance"])
                                                and np.array_equal(x[1]["transforms"], y[1]["transforms"]) for x, y in zip(got, one)))
            k = min(len(got[0][1]["variance"]), len(lf[0]["variance"]))
            r["max_rel_diff_of_variance_from_long_form"] = float(np.abs(got[0][1]["variance"][:k] - lf[0]["variance"][:k]).max() / lf[0]["variance"][0])
            r["max_diff_of_mean_shape_from_long_form_mm"] = float(np.abs(got[0][1]["mean"] - lf[0]["mean"]).max())
        res[name] = r
        print(name, json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
