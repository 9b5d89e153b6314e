#!/usr/bin/env python
"""Developer tool: the census cost (include/ssrlcv_hip.h "census cost") next to the SAD passes it replaces, on the rectified
pair tools/bench_sgm.py uses, on the library ssrlcv_amd/_lib.py loads (release by default).  Not part of the driver contract
(bench.py).  Nothing is gated on these numbers: the SAD passes of the same run are the yardstick.

At size^2 (4096 by default), D = 64, minDisparity -32, every buffer allocated beforehand, one warm-up and `repeats` timed runs
between stream events, medians with min and max:
  census             ssrlcv_hip_census_u8 alone, c = 1, 2, 3 (reads 1 B/pixel, writes 8 B/pixel)
  block matching     the call without the left-right check, with the sub-pixel step and the cost map: census at (c, r) = (2, 2),
                     (1, 7) and (3, 7) (fill + two census passes + cost pass), each beside SAD at the same footprint, radius
                     r + c (fill + cost pass).  "less two census passes" is DERIVED: the whole call's time less twice the census
                     pass timed on its own above; nothing is timed between events inside the block-matching call
  volume pass        events [0] .. [1] of ssrlcv_hip_stereo_sgm_set_pass_events: SAD at radius 2 (fill + cost pass) and census at
                     (c = 2, r = 0) (fill + two census passes + cost pass), again also less the census passes (derived the same
                     way); both store 2 K B/pixel of M and the fill's 8 B/pixel; beside them that traffic's copy floor at 8 TB/s
  the 8-path call    ssrlcv_hip_stereo_sgm_u8 at radius 2, costClamp 1000, P1 40, P2 400 and ssrlcv_hip_stereo_sgm_census_u8 at
                     (c = 2, r = 0), costClamp 24, P1 3, P2 20, both with the left-right check, the sub-pixel step and the cost map

usage: bench_census.py [repeats] [--size N] [--out FILE]      (defaults 7, 4096, profiles/census_bench.txt)"""
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
from bench_sgm import rectified_pair  # noqa: E402
from bench_stereo import commit, take, timed  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
D, DMIN = 64, -32


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "census_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    repeats = max(3, int(args[0])) if args else 7
    assert torch.cuda.is_available(), "bench_census.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    w = h = size
    left, right = rectified_pair(size)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")
    codes = torch.empty((h, w), dtype=torch.int64, device="cuda")
    res = dict(tool="bench_census", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size, numDisparities=D, minDisparity=DMIN)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def valid_share():
        return round(float((disp.view(torch.int32) != capi.STEREO_INVALID_BITS).float().mean()), 4)

    say("bench_census %s commit %s library %s on %s: %d^2, D = %d, minDisparity %d, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, D, DMIN, repeats))
    px = w * h
    # ---- the census pass alone
    res["census"] = {}
    for c in (1, 2, 3):
        s = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_census_u8(capi.ptr(left), u32(w), u32(h), u32(c), capi.ptr(codes), capi.stream_ptr())),
                          repeats))
        s["floor_ms"] = round(px * 9 / PEAK_BYTES_PER_S * 1e3, 4)
        res["census"][str(c)] = s
        say("census pass c = %d                               %8.4f ms (%.4f .. %.4f); 9 B/pixel at 8 TB/s: %.4f ms" % (
            c, s["ms"], s["min_ms"], s["max_ms"], s["floor_ms"]))
    census2 = res["census"]["2"]["ms"]

    # ---- block matching without the left-right check
    def block_matching(radius, c):
        p = capi.StereoParams(radius, DMIN, D, capi.STEREO_NO_LIMIT, -1, 1)
        if c:
            ws = capi.dev_bytes(int(LIB.ssrlcv_hip_stereo_census_workspace_bytes(u32(w), u32(h), ctypes.byref(p), u32(c))))
            fn = lambda: capi.check(LIB.ssrlcv_hip_stereo_census_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p), u32(c),
                                                                    capi.ptr(ws), capi.c_sz(ws.numel()), capi.ptr(disp), capi.ptr(cost),
                                                                    capi.stream_ptr()))
        else:
            ws = capi.stereo_workspace(w, h, p)
            fn = lambda: capi.check(LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p), capi.ptr(ws),
                                                                 capi.c_sz(ws.numel()), capi.ptr(disp), capi.ptr(cost), capi.stream_ptr()))
        s = summary(timed(fn, repeats))
        s["valid_share"] = valid_share()
        return s

    # (c, r) beside SAD at the same footprint: the issue's 9 x 9, then the widest aggregation and the widest footprint
    res["block_matching"] = {}
    for c, r in ((2, 2), (1, 7), (3, 7)):
        sad_bm, cen_bm = block_matching(r + c, 0), block_matching(r, c)
        cen_bm["less_census_ms"] = round(cen_bm["ms"] - 2 * res["census"][str(c)]["ms"], 4)
        res["block_matching"]["sad_radius%d" % (r + c)] = sad_bm
        res["block_matching"]["census_c%d_r%d" % (c, r)] = cen_bm
        say("block matching, no LR check: SAD radius %-2d         %8.4f ms (%.4f .. %.4f), valid %.3f" % (
            r + c, sad_bm["ms"], sad_bm["min_ms"], sad_bm["max_ms"], sad_bm["valid_share"]))
        say("block matching, no LR check: census (c %d, r %d)     %8.4f ms (%.4f .. %.4f), valid %.3f; less two census passes (derived) %.4f ms = "
            "%.2f x SAD" % (c, r, cen_bm["ms"], cen_bm["min_ms"], cen_bm["max_ms"], cen_bm["valid_share"], cen_bm["less_census_ms"],
                            cen_bm["less_census_ms"] / sad_bm["ms"]))

    # ---- semi-global matching: the volume pass between the library's own events, and the whole 8-path call
    K = 8
    while K < D:
        K *= 2
    volume_floor = px * (8 + 2 * K) / PEAK_BYTES_PER_S * 1e3

    def sgm(radius, c, clamp, p1, p2):
        p = capi.SgmParams(radius, DMIN, D, clamp, p1, p2, 0xFF, 1, 1)
        if c:
            ws = capi.dev_bytes(int(LIB.ssrlcv_hip_stereo_sgm_census_workspace_bytes(u32(w), u32(h), ctypes.byref(p), u32(c))))
            fn = lambda: capi.check(LIB.ssrlcv_hip_stereo_sgm_census_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p), u32(c),
                                                                        capi.ptr(ws), capi.c_sz(ws.numel()), capi.ptr(disp), capi.ptr(cost),
                                                                        capi.stream_ptr()))
        else:
            ws = capi.dev_bytes(int(LIB.ssrlcv_hip_stereo_sgm_workspace_bytes(u32(w), u32(h), ctypes.byref(p))))
            fn = lambda: capi.check(LIB.ssrlcv_hip_stereo_sgm_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p), capi.ptr(ws),
                                                                 capi.c_sz(ws.numel()), capi.ptr(disp), capi.ptr(cost), capi.stream_ptr()))
        call = summary(timed(fn, repeats))
        call["valid_share"] = valid_share()
        events = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        capi.stereo_sgm_set_pass_events(events)
        times = []
        for k in range(repeats + 1):
            fn()
            torch.cuda.synchronize()
            if k:   # the first is the warm-up
                times.append(events[0].elapsed_time(events[1]))
        capi.stereo_sgm_set_pass_events(None)
        del ws
        return call, summary(times)

    sad_call, sad_vol = sgm(2, 0, 1000, 40, 400)
    cen_call, cen_vol = sgm(0, 2, 24, 3, 20)
    cen_vol["less_census_ms"] = round(cen_vol["ms"] - 2 * census2, 4)
    res["volume_pass"] = dict(sad_radius2=sad_vol, census_c2_r0=cen_vol, copy_floor_ms=round(volume_floor, 4))
    res["sgm_call"] = dict(sad_radius2=sad_call, census_c2_r0=cen_call)
    say("volume pass (fill + cost): SAD radius 2            %8.4f ms (%.4f .. %.4f); its %d B/pixel at 8 TB/s: %.4f ms" % (
        sad_vol["ms"], sad_vol["min_ms"], sad_vol["max_ms"], 8 + 2 * K, volume_floor))
    say("volume pass (fill + census + cost): census (2, 0)  %8.4f ms (%.4f .. %.4f); less two census passes (derived) %.4f ms = %.2f x SAD" % (
        cen_vol["ms"], cen_vol["min_ms"], cen_vol["max_ms"], cen_vol["less_census_ms"], cen_vol["less_census_ms"] / sad_vol["ms"]))
    say("8-path SGM call: SAD radius 2                      %8.4f ms (%.4f .. %.4f), valid %.3f" % (
        sad_call["ms"], sad_call["min_ms"], sad_call["max_ms"], sad_call["valid_share"]))
    say("8-path SGM call: census (c 2, r 0)                 %8.4f ms (%.4f .. %.4f), valid %.3f = %.3f x SAD" % (
        cen_call["ms"], cen_call["min_ms"], cen_call["max_ms"], cen_call["valid_share"], cen_call["ms"] / sad_call["ms"]))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
