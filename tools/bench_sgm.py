#!/usr/bin/env python
"""Developer tool: semi-global matching (ssrlcv_hip_stereo_sgm_u8) on the rectified pair tools/bench_rectify.py uses (views 0
and 2 of tools/scene.py's PinholeRig, warped by the homographies of ssrlcv_rectify_cameras_host), on the library
ssrlcv_amd/_lib.py loads (release by default).  Not part of the driver contract (bench.py).

Configurations: 4096^2 at r = 2, D = 64 and 1024^2 at r = 2, D = 128, both with paths 0xFF, costClamp 1000, P1 40, P2 400, the
left-right check (tolerance 1), the sub-pixel step and the cost map.  Per configuration one warm-up and `repeats` timed calls,
every buffer allocated beforehand; medians with min and max of
  call            the whole call between two stream events of the tool
  cost            fill + cost pass, between the events the library records itself (ssrlcv_hip_stereo_sgm_set_pass_events)
  dir0 .. dir7    each direction's pass (dir0 stores S, the others read and add)
  winners, lr     the winner pass and the left-right check
and, per pass, the bytes it must move by this design and the share of 8 TB/s that is over its time, with K = D rounded up to
the volume's entry (8 nD):
  cost            reads 2 B/pixel, writes the fill's 8 B/pixel and M: 2 K B/pixel
  dir (storing)   reads M, writes S: 4 K B/pixel;   dir (adding) reads M and S, writes S: 6 K B/pixel
  winners         reads S once plus, per strip of T = min(1024, 16384 / K) pixels, the D - 1 pixels beside it whose entries
                  belong to the strip's right pixels: 2 K (1 + (D - 1) / T) B/pixel, writes 8 + 2 B/pixel
  lr              reads 4 + 1 + 1 B/pixel
Beside it the SAD call (ssrlcv_hip_stereo_sad_u8) at the same r and D with the same check, sub-pixel step and cost map, and
the ratio SGM / SAD.

usage: bench_sgm.py [repeats] [--size N] [--out FILE]      (defaults 7, both sizes; --size N runs N^2 at D = 64 alone)"""
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
from bench_stereo import commit, take, timed  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
RADIUS, CLAMP, P1, P2, PATHS, VIEWS = 2, 1000, 40, 400, 0xFF, (0, 2)
CONFIGS = ((4096, 64), (1024, 128))


def summary(times, nbytes=None):
    med = float(np.median(times))
    out = dict(ms=round(med, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))
    if nbytes is not None:
        out.update(bytes=int(nbytes), floor_ms=round(nbytes / PEAK_BYTES_PER_S * 1e3, 4),
                   share_of_8TBps=round(nbytes / PEAK_BYTES_PER_S / (med * 1e-3), 4))
    return out


def rectified_pair(size):
    import scene
    rig = scene.PinholeRig(3, size)
    sc = scene.Scene(size, rig.gsd)
    left, right = [rig.render(sc, v).contiguous() for v in VIEWS]
    rect = capi.rectify_cameras(rig.cameras[VIEWS[0]], rig.cameras[VIEWS[1]])
    return capi.warp_homography(left, rect["Hl"], (size, size)), capi.warp_homography(right, rect["Hr"], (size, size))


def run(size, D, repeats):
    u32 = capi.c_u32
    w = h = size
    left, right = rectified_pair(size)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")
    dmin = -(D // 2)   # the disparities of the rectified pair lie around 0 (bench_rectify.py)
    p = capi.SgmParams(RADIUS, dmin, D, CLAMP, P1, P2, PATHS, 1, 1)
    ws = capi.dev_bytes(int(capi.LIB.ssrlcv_hip_stereo_sgm_workspace_bytes(u32(w), u32(h), ctypes.byref(p))))

    def sgm():
        capi.check(capi.LIB.ssrlcv_hip_stereo_sgm_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p), capi.ptr(ws),
                                                     capi.c_sz(ws.numel()), capi.ptr(disp), capi.ptr(cost), capi.stream_ptr()))

    call = timed(sgm, repeats)
    sgm_valid = float((disp.view(torch.int32) != capi.STEREO_INVALID_BITS).float().mean())
    # the passes, between the events the library records
    names = ["cost"] + ["dir%d" % i for i in range(8) if (PATHS >> i) & 1] + ["winners", "lr"]
    events = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
    capi.stereo_sgm_set_pass_events(events)
    passes = {n: [] for n in names}
    for k in range(repeats + 1):
        sgm()
        torch.cuda.synchronize()
        if k:   # the first is the warm-up
            for i, n in enumerate(names):
                passes[n].append(events[i].elapsed_time(events[i + 1]))
    capi.stereo_sgm_set_pass_events(None)
    K = 8
    while K < D:
        K *= 2
    px = w * h
    T = min(1024, 16384 // K)
    nbytes = dict(cost=px * (2 + 8 + 2 * K), winners=int(px * (2 * K * (1 + (D - 1) / T) + 10)), lr=px * 6)
    first = True
    for n in names:
        if n.startswith("dir"):
            nbytes[n] = px * (4 * K if first else 6 * K)
            first = False
    row = dict(size=size, numDisparities=D, minDisparity=dmin, workspace_bytes=int(ws.numel()), valid_share=round(sgm_valid, 4),
               call=summary(call, sum(nbytes.values())), passes={n: summary(passes[n], nbytes[n]) for n in names})
    del ws
    sp = capi.StereoParams(RADIUS, dmin, D, capi.STEREO_NO_LIMIT, 1, 1)
    sws = capi.stereo_workspace(w, h, sp)

    def sad():
        capi.check(capi.LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(sp), capi.ptr(sws),
                                                     capi.c_sz(sws.numel()), capi.ptr(disp), capi.ptr(cost), capi.stream_ptr()))

    row["sad_call"] = summary(timed(sad, repeats))
    row["sad_valid_share"] = round(float((disp.view(torch.int32) != capi.STEREO_INVALID_BITS).float().mean()), 4)
    row["sgm_over_sad"] = round(row["call"]["ms"] / row["sad_call"]["ms"], 3)
    print("%d^2 r %d D %d paths 0x%02X: call %.3f ms (%.3f .. %.3f), %.3f of its %.3f ms floor at 8 TB/s; SAD call %.3f ms; SGM / SAD %.2f; "
          "valid %.3f (SAD %.3f)" % (size, RADIUS, D, PATHS, row["call"]["ms"], row["call"]["min_ms"], row["call"]["max_ms"],
                                     row["call"]["share_of_8TBps"], row["call"]["floor_ms"], row["sad_call"]["ms"], row["sgm_over_sad"],
                                     row["valid_share"], row["sad_valid_share"]), flush=True)
    for n in names:
        s = row["passes"][n]
        print("  %-8s %9.4f ms (%.4f .. %.4f)  %7.1f MB, floor %.4f ms = %.3f of it" % (n, s["ms"], s["min_ms"], s["max_ms"], s["bytes"] / 1e6,
                                                                                      s["floor_ms"], s["share_of_8TBps"]), flush=True)
    return row


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None, str)
    size = take(args, "--size", None, int)
    repeats = max(3, int(args[0])) if args else 7
    assert torch.cuda.is_available(), "bench_sgm.py needs a GPU"
    torch.cuda.set_device(0)
    rows = [run(s, D, repeats) for s, D in (CONFIGS if size is None else ((size, 64),))]
    result = dict(tool="bench_sgm", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
                  device=torch.cuda.get_device_name(0), repeats=repeats, radius=RADIUS, costClamp=CLAMP, P1=P1, P2=P2, paths=PATHS,
                  lrTolerance=1, subpixel=1, peak_bytes_per_s=PEAK_BYTES_PER_S, configs=rows)
    line = json.dumps(result)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
