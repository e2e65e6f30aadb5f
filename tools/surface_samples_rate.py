"""dev: uniform surface samples with nearest vertices (icp_surface_samples_many) at two sizes:
  femur1k        50 copies of the bundled femur target (1,622 vertices) x 1,000 samples: (a) one batched surface_samples call against
                 (b) one call per mesh;
  synthetic58k   10 copies of data.synthetic_femur_target() (58,322 vertices) x 50,000 samples: (a) and (b) as above against (c) the host
                 route that was there before — data.uniform_mesh_samples plus a numpy nearest-vertex search (another generator: other
                 points, the same law).  (c) is 2.9e9 pair tests per mesh, so it is timed on --numpy-meshes meshes, --numpy-repeats
                 times; what was run is in the result.
Warm-up first, then --repeats interleaved repeats; host clock around synchronised calls.  Prints one JSON line: meshes/s as median
[min, max] per way, the ratios of the medians, and whether (a) and (b) deliver the same arrays bit for bit."""
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
import surface_samples_long_form as LF  # noqa: E402

pkg = g.load_package()


def rates(n, ts):
    r = sorted(n / t for t in ts)
    return {"median": float(np.median(r)), "min": r[0], "max": r[-1]}


def same(x, y):
    return all(LF.same(getattr(x, k), getattr(y, k)) for k in ("points", "cells", "bary", "vertex_ids"))


def numpy_route(mesh, n, seed):
    pts = pkg.data.uniform_mesh_samples(mesh, n, seed)
    return pts, LF.nearest_vertices(mesh.points, pts, chunk=256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-repeats", type=int, default=7)
    ap.add_argument("--numpy-meshes", type=int, default=10)
    ap.add_argument("--cases", default="femur1k,synthetic58k")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    meshes = {"femur1k": lambda: pkg.data.load_femur_model_and_target(50)[1], "synthetic58k": lambda: pkg.data.synthetic_femur_target()[1]}
    cases = {"femur1k": (50, 1000, False), "synthetic58k": (10, 50000, True)}
    res = {"repeats": a.repeats, "numpy_threads": os.environ.get("OMP_NUM_THREADS")}
    for name in a.cases.split(","):
        n, k, with_numpy = cases[name]
        mesh = meshes[name]()
        batch, seeds = [mesh] * n, list(range(n))
        run_a = lambda: pkg.surface_samples(batch, k, seeds)  # noqa: E731
        run_b = lambda: [pkg.surface_samples([m], k, [s])[0] for m, s in zip(batch, seeds)]  # noqa: E731
        run_a(); run_b()  # warm-up
        ta, tb, tc = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter(); ra = run_a(); ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); rb = run_b(); tb.append(time.perf_counter() - t0)
        res[name] = {"meshes": n, "vertices": mesh.n_points, "triangles": mesh.n_cells, "samples": k,
                     "meshes_per_s_batched": rates(n, ta), "meshes_per_s_per_item": rates(n, tb),
                     "batched_over_per_item": float(np.median(tb) / np.median(ta)),
                     "batched_equals_per_item_bitwise": bool(all(same(x, y) for x, y in zip(ra, rb)))}
        if with_numpy and a.numpy_repeats > 0:
            m = min(a.numpy_meshes, n)
            for _ in range(a.numpy_repeats):
                t0 = time.perf_counter()
                for s in range(m):
                    numpy_route(mesh, k, s)
                tc.append(time.perf_counter() - t0)
            res[name].update({"meshes_per_s_numpy_route": rates(m, tc), "numpy_route_meshes": m, "numpy_route_repeats": a.numpy_repeats,
                              "batched_over_numpy_route": float((np.median(tc) / m) / (np.median(ta) / n))})
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
