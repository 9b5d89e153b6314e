#!/usr/bin/env python
"""Developer tool: the rectification steps (include/ssrlcv_hip.h "rectification") around dense stereo on a 4096^2 pair, on the
library ssrlcv_amd/_lib.py loads (release by default).  Not part of the driver contract (bench.py).

The pair: views 0 and 2 of tools/scene.py's PinholeRig, a converging pair 70 km apart; ssrlcv_rectify_cameras_host gives the
two homographies.  Timed, each with one warm-up and `repeats` calls between stream events, every buffer allocated beforehand,
the median reported with min and max:
  warp_left, warp_right   ssrlcv_hip_warp_homography_u8 of either view
  stereo                  ssrlcv_hip_stereo_sad_u8 at r = 4, D = 64 on the rectified pair (left-right check, sub-pixel, cost map)
  mask                    ssrlcv_hip_stereo_mask_rectified on a copy of that call's maps (the copy is not timed)
  unrectify               ssrlcv_hip_matches_apply_homography on a copy of ssrlcv_hip_stereo_matches' records at step 1
Per step the floor of its own minimum traffic at the 6.3 TB/s a copy achieves on this chip: the warp reads 1 B and
writes 1 B per pixel; the mask reads 4 B per pixel and writes at most 8 B; the un-rectify step reads and writes the two
locations of a record, 16 B each way.  And the one figure: (two warps + mask + unrectify) / stereo.

usage: bench_rectify.py [repeats] [--size N] [--out FILE]      (defaults 7, 4096)"""
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
from bench_stereo import HBM_BYTES_PER_S, commit, take, timed  # noqa: E402

RADIUS, DISPARITIES, VIEWS = 4, 64, (0, 2)


def summary(times, min_bytes):
    med = float(np.median(times))
    return dict(ms=round(med, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4), min_bytes=int(min_bytes),
                hbm_floor_ms=round(min_bytes / HBM_BYTES_PER_S * 1e3, 4), hbm_floor_fraction=round(min_bytes / HBM_BYTES_PER_S / (med * 1e-3), 4))


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None, str)
    size = take(args, "--size", 4096, int)
    repeats = max(3, int(args[0])) if args else 7
    assert torch.cuda.is_available(), "bench_rectify.py needs a GPU"
    torch.cuda.set_device(0)
    import scene
    rig = scene.PinholeRig(3, size)
    sc = scene.Scene(size, rig.gsd)
    left, right = [rig.render(sc, v).contiguous() for v in VIEWS]
    rect = capi.rectify_cameras(rig.cameras[VIEWS[0]], rig.cameras[VIEWS[1]])
    w = h = size
    u32 = capi.c_u32
    Hl, Hr = capi.homography9(rect["Hl"]), capi.homography9(rect["Hr"])
    left_r = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    right_r = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    steps = {}

    def warp(src, Hm, dst):
        return lambda: capi.check(capi.LIB.ssrlcv_hip_warp_homography_u8(capi.ptr(src), u32(w), u32(h), Hm, capi.ptr(dst), u32(w), u32(h),
                                                                         capi.stream_ptr()))

    steps["warp_left"] = summary(timed(warp(left, Hl, left_r), repeats), 2 * w * h)
    steps["warp_right"] = summary(timed(warp(right, Hr, right_r), repeats), 2 * w * h)

    # the disparities the rectified pair holds lie around 0 (both old image centres land on the rectified centre)
    p = capi.StereoParams(RADIUS, -(DISPARITIES // 2), DISPARITIES, capi.STEREO_NO_LIMIT, 1, 1)
    ws = capi.stereo_workspace(w, h, p)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")

    def stereo():
        capi.check(capi.LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left_r), capi.ptr(right_r), u32(w), u32(h), ctypes.byref(p), capi.ptr(ws),
                                                     capi.c_sz(ws.numel()), capi.ptr(disp), capi.ptr(cost), capi.stream_ptr()))

    steps["stereo"] = summary(timed(stereo, repeats), w * h * (2 + 8 + 8))
    valid_before = int((disp.view(torch.int32) != capi.STEREO_INVALID_BITS).sum())

    # the mask and the un-rectify step work in place: each timed call runs on a fresh copy made outside the events
    def timed_in_place(make, fn):
        times = []
        for k in range(repeats + 1):
            bufs = make()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(*bufs)
            e1.record()
            torch.cuda.synchronize()
            if k:   # the first is the warm-up
                times.append(e0.elapsed_time(e1))
        return times, bufs

    def mask(d, c):
        capi.check(capi.LIB.ssrlcv_hip_stereo_mask_rectified(capi.ptr(d), capi.ptr(c), u32(w), u32(h), u32(RADIUS), Hl, Hr, u32(w), u32(h),
                                                             capi.stream_ptr()))

    t, (masked, _) = timed_in_place(lambda: (disp.clone(), cost.clone()), mask)
    steps["mask"] = summary(t, w * h * (4 + 8))
    valid_after = int((masked.view(torch.int32) != capi.STEREO_INVALID_BITS).sum())

    matches, n = capi.stereo_matches(masked, 1, 0, 1)

    def unrectify(m):
        capi.check(capi.LIB.ssrlcv_hip_matches_apply_homography(capi.ptr(m), u32(n), Hl, Hr, capi.stream_ptr()))

    t, (moved,) = timed_in_place(lambda: (matches.clone(),), unrectify)
    steps["unrectify"] = summary(t, n * 32)
    flagged = int((moved.view(-1, 40)[:, 0] != 0).sum())

    around = steps["warp_left"]["ms"] + steps["warp_right"]["ms"] + steps["mask"]["ms"] + steps["unrectify"]["ms"]
    ratio = round(around / steps["stereo"]["ms"], 4)
    for name in ("warp_left", "warp_right", "stereo", "mask", "unrectify"):
        s = steps[name]
        print("%-10s %9.4f ms (%.4f .. %.4f)  floor %.4f ms = %.3f of it" % (name, s["ms"], s["min_ms"], s["max_ms"], s["hbm_floor_ms"],
                                                                           s["hbm_floor_fraction"]), flush=True)
    print("valid pixels %d -> %d after the mask; %d records, %d flagged by the un-rectify step; (two warps + mask + unrectify) / stereo = %.4f" %
          (valid_before, valid_after, n, flagged, ratio))
    result = dict(tool="bench_rectify", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
                  device=torch.cuda.get_device_name(0), size=size, repeats=repeats, views=list(VIEWS), radius=RADIUS,
                  numDisparities=DISPARITIES, minDisparity=-(DISPARITIES // 2), hbm_bytes_per_s=HBM_BYTES_PER_S,
                  doffset=float(rect["doffset"]), foc=float(rect["foc"]), baseline=float(rect["baseline"]),
                  valid_before_mask=valid_before, valid_after_mask=valid_after, records=n, records_flagged=flagged,
                  rectification_over_stereo=ratio, steps=steps)
    line = json.dumps(result)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
