"""dev: Gaussian-process shape models by the Nyström approximation (nystrom_models / icp_nystrom_models_many; what
apps/femur/CreateGPModel.scala and apps/bfm/CreateGPModel.scala call).  Cases, (sample points n, basis functions k):
  femur reference (N = 1,622) with femur_kernel x (100, 51), (200, 101), (400, 201);
  the face-sized stand-in mesh (N = 28,561) with the same kernel family x (800, 200).
Three ways, 8 items each (every item has sample points of its own, data.uniform_mesh_samples with the item's seed): one batched call,
one call per item, and the numpy long form (tests/nystrom_model_long_form.py) at the box's thread count — for the face the long form is
timed on `--face-host-items` items (default 1), at most three times, and its rate is per item all the same.  Warm-up of all ways first;
then `--repeats` timed runs of each, interleaved; host clock around the calls (the entry point returns after its last synchronisation).
Prints one JSON line: per case items/s as median [min, max] of each way, the ratios of the medians, whether the batched and the
one-item forms agree bit for bit, the sweeps used, and the largest relative difference of the eigenvalues from eigh's.
  --only-batched   time the batched way alone (for a kernel-trace run)"""
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
import nystrom_model_long_form as NLF  # noqa: E402

pkg = g.load_package()
ITEMS = 8


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
    ap.add_argument("--skip-femur", action="store_true")
    ap.add_argument("--face-host-items", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nystrom_models_rate.json"))
    a = ap.parse_args()
    femur, _, _ = pkg.data.load_femur_mesh("femur_reference")
    cases = [] if a.skip_femur else [(f"femur_n{n}_k{k}_x{ITEMS}", femur, n, k, ITEMS, a.repeats) for n, k in ((100, 51), (200, 101), (400, 201))]
    if not a.skip_face:
        face = pkg.data.synthetic_face_model(grid=169, rank=1)
        cases.append((f"face_n800_k200_x{ITEMS}", pkg.data.TriangleMesh(face.ref_points, face.cells), 800, 200, a.face_host_items, min(a.repeats, 3)))
    res = {"repeats": a.repeats, "host_threads": os.environ.get("OMP_NUM_THREADS")}
    for name, mesh, n, k, host_items, host_repeats in cases:
        terms = pkg.data.femur_kernel(mesh)
        items = [(mesh, pkg.data.uniform_mesh_samples(mesh, n, seed=b), terms, k) for b in range(ITEMS)]
        batched = lambda: pkg.nystrom_models(items)  # noqa: E731
        per_item = lambda: [pkg.nystrom_models([it])[0] for it in items]  # noqa: E731
        host = lambda: [NLF.long_form(mesh.points, items[b][1], terms, k) for b in range(host_items)]  # noqa: E731
        r = {"items": ITEMS, "vertices": mesh.n_points, "samples": n, "rank": k, "rows": 3 * n, "basis_out_bytes_per_item": 3 * mesh.n_points * k * 8,
             "host_items_timed": host_items}
        got = batched()
        r["sweeps"] = [i["sweeps"] for _, i in got]
        r["effective_rank"] = [i["rank"] for _, i in got]
        r["status"] = [i["status"] for _, i in got]
        if a.only_batched:
            r["batched_items_per_s"] = rate(ITEMS, [timed(batched)[0] for _ in range(a.repeats)])
        else:
            one = per_item()
            lf = host()[0]
            tb, to, th = [], [], []
            for rep in range(a.repeats):
                tb.append(timed(batched)[0])
                to.append(timed(per_item)[0])
                if rep < host_repeats:
                    th.append(timed(host)[0])
            r["batched_items_per_s"], r["one_call_per_item_items_per_s"] = rate(ITEMS, tb), rate(ITEMS, to)
            r["numpy_long_form_items_per_s"] = rate(host_items, th)
            r["batched_over_one_call_per_item"] = r["batched_items_per_s"]["median"] / r["one_call_per_item_items_per_s"]["median"]
            r["batched_over_numpy_long_form"] = r["batched_items_per_s"]["median"] / r["numpy_long_form_items_per_s"]["median"]
            r["one_item_bits_equal"] = bool(all(np.array_equal(x[0].basis, y[0].basis) and np.array_equal(x[1]["sample_eigenvalues"], y[1]["sample_eigenvalues"])
                                                for x, y in zip(got, one)))
            w = lf["eigh_values"]
            r["max_rel_diff_of_eigenvalues_from_eigh"] = float(np.abs(got[0][1]["sample_eigenvalues"] - w).max() / w[0])
        res[name] = r
        print(name, json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
