"""Time the fundamental-matrix RANSAC (ssrlcv_hip_fmatrix_ransac) and its scoring kernel on the GPU.

For M in {13534 (the Pipeline2View stage-0 tie points), 1e5, 3e5 (synthetic scenes of tests/ransac_ref.py)} x samples in
{1024, 4096}: ms per whole call, and ms of the candidates x matches scoring alone (ssrlcv_hip_fmatrix_score over the
3 * samples candidates the call produced: k_fmatrix_score plus its two tiny normalisation launches), tests/s, and the
fraction of the VALU issue floor: tests x VALU_PER_TEST / 64 lanes over bench.py's VALU_PEAK_GINST.  HIP events after
warm-up.  One JSON line per point; --out writes the list.
usage: python tools/bench_ransac.py [--reps 20] [--out profiles/ransac_bench.json] [--label name]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALU_PEAK_GINST = 1228.8  # bench.py: 256 CUs x 4 SIMDs x 1.2 GHz wave-instructions/s
VALU_PER_TEST = 20        # k_fmatrix_score inner loop: 19 fp (v_fma / v_fmac / v_mul) + 1 v_cmp per Sampson test (ISA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers as H
    import ransac_ref as R
    from ssrlcv_amd import capi, _lib
    assert torch.cuda.is_available(), "bench_ransac needs a GPU"
    v = H.load_view("Pipeline2View")
    scenes = {13534: H.matches_from_matchset(v["kp0"])}
    for n in (100000, 300000):
        scenes[n] = R.synthetic(n, seed=11)[0]
    rows = []
    for n, m in scenes.items():
        md = capi.to_dev(m)
        for S in (1024, 4096):
            K = 3 * S
            ws = capi.dev_bytes(capi.LIB.ssrlcv_hip_fmatrix_ransac_workspace_bytes(capi.c_u32(n), capi.c_u32(S)))
            F = torch.empty(9, dtype=torch.float32, device="cuda")
            cnt = torch.empty(1, dtype=torch.int32, device="cuda")
            cand = torch.empty(9 * K, dtype=torch.float32, device="cuda")
            counts = torch.empty(K, dtype=torch.int32, device="cuda")
            aux = capi.dev_bytes(capi.FMATRIX_AUX_WORKSPACE_BYTES)

            def ransac():
                capi.check(capi.LIB.ssrlcv_hip_fmatrix_ransac(
                    capi.ptr(md), capi.c_u32(n), capi.c_u32(S), capi.c_f32(2.0), capi.ctypes.c_uint64(0), capi.ptr(ws),
                    capi.c_sz(ws.numel()), capi.ptr(F), capi.ptr(cnt), capi.c_vp(0), capi.ptr(cand), capi.ptr(counts),
                    capi.stream_ptr()))

            def score():
                capi.check(capi.LIB.ssrlcv_hip_fmatrix_score(
                    capi.ptr(md), capi.c_u32(n), capi.ptr(cand), capi.c_u32(K), capi.c_f32(2.0), capi.ptr(aux),
                    capi.c_sz(aux.numel()), capi.ptr(counts), capi.c_vp(0), capi.stream_ptr()))

            def timed(fn):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / a.reps

            t_call = timed(ransac)
            count = int(cnt.item())
            t_score = timed(score)
            tests = float(K) * n
            floor_ms = tests * VALU_PER_TEST / 64 / (VALU_PEAK_GINST * 1e9) * 1e3
            row = {"label": a.label, "lib": _lib.flavour(), "matches": n, "samples": S, "candidates": K,
                   "inliers": count, "ms_per_call": round(t_call, 4), "ms_score": round(t_score, 4),
                   "tests_per_s": tests / (t_score * 1e-3), "valu_floor_ms": round(floor_ms, 4),
                   "fraction_of_valu_floor": round(floor_ms / t_score, 3)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
