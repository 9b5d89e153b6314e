#!/usr/bin/env python
"""Developer tool: dense stereo (ssrlcv_hip_stereo_sad_u8) on a 4096^2 rectified pair, on the library ssrlcv_amd/_lib.py
loads (release by default).  Not part of the driver contract (bench.py).

The pair: one 4096^2 view of tools/scene.py's terrain is the right image; the left image is that view displaced by a two-plane
integer disparity field (12 px behind, 40 px on a rectangle in front), so the pair is rectified by construction.
Configurations: radius 1, 4, 15 x 64 and 128 disparities from 0, with the left-right check (tolerance 1), the sub-pixel step
and the cost map -- the whole call -- and, beside it, the cost pass alone (no left-right check).  Per configuration one warm-up
and `repeats` timed calls between stream events, every buffer allocated beforehand; the median is reported with min and max.

Per configuration:
  ms              median time of the call
  evals/s         cost evaluations per second, w h D / t (one evaluation = one C(x, y, d), whatever the window)
  hbm             the HBM floor of the call's own minimum traffic over t: 2 B/pixel read, 4 + 4 B/pixel written (disparity and
                  cost), plus the workspace (1 + 1 B/pixel written, read once, and the disparity re-read by the left-right
                  check) at the 6.3 TB/s a copy achieves on this chip
  issue           the issue floor of the v_sad_u8 instructions alone over t: passes x w h D x 2 ceil((2r + 1) / 4) / 64
                  wave-instructions (entering and leaving row of the separable sum) at the measured cycles per instruction and
                  SIMD (tools/valu_rate.hip, --sad-cycles) on 1024 SIMDs at 2.4 GHz
and once: t(r = 15) / t(r = 4).  The window area grows 11.9 x, the separable form's work at most 31 / 9 = 3.4 x; a ratio near
the area ratio would mean the windows are being re-summed.

usage: bench_stereo.py [repeats] [--size N] [--sad-cycles C] [--out FILE]      (defaults 7, 4096, 4.45: v_sad_u8 at four waves per SIMD, profiles/stereo_sad_rate.txt)"""
import ctypes
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ssrlcv_amd import _lib, capi  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SIMDS, CLOCK = 1024, 2.4e9
RADII, DISPARITIES = (1, 4, 15), (64, 128)
FAR, NEAR = 12, 40


def take(args, flag, default, kind):
    if flag in args:
        i = args.index(flag)
        v = kind(args[i + 1])
        del args[i:i + 2]
        return v
    return default


def make_pair(size):
    import scene
    views, _, _, _ = scene.pinhole_views(1, size)
    right = views[0].contiguous()
    xs = torch.arange(size, device=right.device)[None, :].expand(size, size)
    field = torch.full((size, size), FAR, device=right.device, dtype=torch.long)
    field[size // 5: size - size // 4, (2 * size) // 5: (4 * size) // 5] = NEAR
    left = torch.gather(right, 1, (xs - field).clamp(0, size - 1)).contiguous()
    return left, right, field


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def commit():
    try:
        return open(os.path.join(ROOT, "ssrlcv_amd", "_build_commit.txt")).read().strip()
    except OSError:
        return "unknown"


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None, str)
    size = take(args, "--size", 4096, int)
    sad_cycles = take(args, "--sad-cycles", 4.45, float)
    repeats = max(3, int(args[0])) if args else 7
    assert torch.cuda.is_available(), "bench_stereo.py needs a GPU"
    torch.cuda.set_device(0)
    left, right, field = make_pair(size)
    w = h = size
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")
    rows = []
    for r in RADII:
        for D in DISPARITIES:
            row = dict(radius=r, numDisparities=D)
            for label, lr in (("call", 1), ("cost_pass", -1)):
                p = capi.StereoParams(r, 0, D, capi.STEREO_NO_LIMIT, lr, 1)
                ws = capi.stereo_workspace(w, h, p)

                def call():
                    capi.check(capi.LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), capi.c_u32(w), capi.c_u32(h), ctypes.byref(p),
                                                                 capi.ptr(ws), capi.c_sz(ws.numel()), capi.ptr(disp), capi.ptr(cost),
                                                                 capi.stream_ptr()))

                t = timed(call, repeats)
                med = float(np.median(t))
                passes = 2 if lr >= 0 else 1
                min_bytes = w * h * (2 + 8 + ((2 + 2 + 4) if lr >= 0 else 1))
                sads = passes * w * h * D * 2 * ((2 * r + 1 + 3) // 4) / 64.0
                row[label] = dict(ms=round(med, 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                                  evals_per_s=round(w * h * D / (med * 1e-3), 1),
                                  hbm_floor_fraction=round(min_bytes / HBM_BYTES_PER_S / (med * 1e-3), 4),
                                  sad_issue_floor_fraction=round(sads * sad_cycles / (SIMDS * CLOCK) / (med * 1e-3), 4))
            valid = disp.view(torch.int32) != capi.STEREO_INVALID_BITS
            good = valid & ((disp - field.float()).abs() <= 0.5)
            row["valid_share"] = round(float(valid.float().mean()), 4)
            row["within_half_px_of_field_share_of_valid"] = round(float(good.sum()) / max(int(valid.sum()), 1), 4)
            rows.append(row)
            print("r %2d D %3d: call %8.3f ms (%.3f .. %.3f)  %.3e evals/s  hbm %.3f  sad issue %.3f | cost pass alone %8.3f ms  sad issue %.3f | "
                  "valid %.3f, within 0.5 px of the field %.3f" %
                  (r, D, row["call"]["ms"], row["call"]["min_ms"], row["call"]["max_ms"], row["call"]["evals_per_s"],
                   row["call"]["hbm_floor_fraction"], row["call"]["sad_issue_floor_fraction"], row["cost_pass"]["ms"],
                   row["cost_pass"]["sad_issue_floor_fraction"], row["valid_share"], row["within_half_px_of_field_share_of_valid"]), flush=True)
    ratios = {}
    for D in DISPARITIES:
        t = {row["radius"]: row["call"]["ms"] for row in rows if row["numDisparities"] == D}
        ratios[str(D)] = round(t[15] / t[4], 3)
    result = dict(tool="bench_stereo", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
                  device=torch.cuda.get_device_name(0), size=size, repeats=repeats, sad_cycles_per_instruction_per_simd=sad_cycles,
                  hbm_bytes_per_s=HBM_BYTES_PER_S, r15_over_r4=ratios, configs=rows)
    line = json.dumps(result)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
