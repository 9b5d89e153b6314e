"""Time the point-cloud stage (csrc/cloud.hip) on the GPU against scipy's cKDTree on the host.

Clouds: the tools/scene.py terrain patch at the fixture's ECEF offset (km) with 1 % of the points displaced 1-5 km
(tests/cloud_ref.py terrain_cloud), n in {0.3 M, 1 M, 4 M}; k in {8, 16, 32}.  Per point: ms per ssrlcv_hip_knn call
(automatic cell size, grid build included) and queries/s, the fraction of queries that took the exact far path, ms of
the neighbour-distance filter (sigma 2) and of the normals on that k-NN, and cKDTree(...).query(k + 1, workers=16) on
the same cloud (build + query; skipped at 4 M for k != 16).  HIP events after warm-up.  One JSON line per point; --out
writes the list.
usage: python tools/bench_cloud.py [--reps 10] [--out profiles/cloud_bench.json] [--sizes 300000,1000000,4000000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--sizes", default="300000,1000000,4000000")
    ap.add_argument("--ks", default="8,16,32")
    a = ap.parse_args()
    import numpy as np
    import torch
    import cloud_ref as R
    from ssrlcv_amd import capi, _lib
    from scipy.spatial import cKDTree
    assert torch.cuda.is_available(), "bench_cloud needs a GPU"

    def timed(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        p, out, up = R.terrain_cloud(n, seed=17, device="cuda")
        pd = torch.from_numpy(p).cuda()
        vp = (p.astype(np.float64).mean(0) + 400.0 * up).astype(np.float32)
        for k in [int(x) for x in a.ks.split(",")]:
            nbr, d2, far = capi.knn(pd, k, far=True)
            knn_ms = timed(lambda: capi.knn(pd, k))
            filt_ms = timed(lambda: capi.neighbor_distance_filter(pd, d2, k, 2.0))
            nrm_ms = timed(lambda: capi.point_normals(pd, nbr, k, vp))
            row = {"n": n, "k": k, "knn_ms": round(knn_ms, 4), "knn_queries_per_s": round(n / knn_ms * 1e3),
                   "far_fraction": int(far.item()) / n, "filter_ms": round(filt_ms, 4), "normals_ms": round(nrm_ms, 4),
                   "library": _lib.flavour()}
            if n < 2000000 or k == 16:
                q = p.astype(np.float64)
                t0 = time.perf_counter()
                tree = cKDTree(q)
                t1 = time.perf_counter()
                tree.query(q, k=k + 1, workers=16)
                t2 = time.perf_counter()
                row.update({"ckdtree_build_ms": round((t1 - t0) * 1e3, 1), "ckdtree_query_ms": round((t2 - t1) * 1e3, 1),
                            "speedup_vs_ckdtree": round((t2 - t0) * 1e3 / knn_ms, 1)})
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
