#!/usr/bin/env python
"""Developer tool: the ortho-image (include/ssrlcv_hip.h "ortho-image") on the library ssrlcv_amd/_lib.py loads (release by
default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: the block-matching call and a plain
device copy of the same run are the yardsticks, the spread of identical repeats is the noise.

A size^2 grid (4096 by default) of cells of 1, and size^2 source images of random bytes from cameras 5 size above it: the first
at nadir, the others 30 degrees off it, spread evenly in azimuth.  Two maps: "flat", noise of 0.2, and "towers", the same with one
8 x 8 tower of height 40 every 64 x 64 cells.  Every buffer is allocated beforehand, one warm-up and `repeats` timed runs between
stream events, medians with min and max, for maxSteps 0, 64, 256 x m = 1, 3, 8 views (bias 0.5, rule MEDIAN, seen and which
written).  Beside each time the bytes the call must move at least -- 4 B a cell read, 3 B a cell written, 4 source bytes a seeing
view and cell -- the time of a plain device-to-device copy moving as many bytes in the same run, the ratio to the block-matching
call (SAD radius 2, D = 64, on the pair of tools/bench_stereo.py), and a checksum of the three outputs: every form gives the same.

--form NAME labels the run (the A/B of the march's forms: a library built aside with -DSSRLCV_ORTHO_PLAIN, the march without
its early stop, and loaded through SSRLCV_HIP_LIB); --append adds to the file instead of replacing it.

usage: bench_ortho.py [repeats] [--size N] [--form NAME] [--append] [--out FILE]   (defaults 5, 4096, profiles/ortho_bench.txt)"""
import ctypes
import datetime
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ssrlcv_amd import _lib, capi  # noqa: E402
from bench_stereo import commit, make_pair, take, timed  # noqa: E402
from bench_dsm import summary  # noqa: E402
import scene  # noqa: E402

RADIUS, D = 2, 64



def camera(pos, target, size, fov):
    """an Image::Camera record at `pos` looking at `target`, image x as near world x as the view allows"""
    a3 = (target - pos) / np.linalg.norm(target - pos)
    a1 = np.array([1.0, 0.0, 0.0]) - a3[0] * a3
    a1 /= np.linalg.norm(a1)
    cam = np.zeros(1, scene.CAMERA)
    cam["cam_pos"][0], cam["fov"][0], cam["foc"][0], cam["size"][0] = pos, fov, 0.16, size
    cam["cam_rot"][0] = scene._rotation_to_euler(np.stack([a1, np.cross(a3, a1), a3], 1)).astype(np.float32)
    return cam[0]


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "ortho_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    form = take(args, "--form", "shipped", str)
    append = "--append" in args
    args = [a for a in args if a != "--append"]
    repeats = max(3, int(args[0])) if args else 5
    assert torch.cuda.is_available(), "bench_ortho.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    w = h = size
    res = dict(tool="bench_ortho", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(), form=form,
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_ortho %s commit %s library %s (march form: %s) on %s: %d^2 cells, %d^2 images, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], form, res["device"], size, size, repeats))

    left, right, _ = make_pair(size)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")
    p = capi.StereoParams(RADIUS, 0, D, capi.STEREO_NO_LIMIT, 1, 1)
    sad_ws = capi.stereo_workspace(w, h, p)
    sad = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p),
                                                                        capi.ptr(sad_ws), capi.c_sz(sad_ws.numel()), capi.ptr(disp), capi.ptr(cost),
                                                                        capi.stream_ptr())), repeats))
    del sad_ws, cost, left, right, disp
    res["block_matching"] = sad
    say("block matching, SAD radius %d, D %d, LR 1, sub-pixel   %8.4f ms (%.4f .. %.4f)" % (RADIUS, D, sad["ms"], sad["min_ms"], sad["max_ms"]))

    frame = capi.DsmFrame.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1.0, w, h)
    centre, up = np.array([w / 2.0, h / 2.0, 0.0]), 5.0 * size
    fov = 2.0 * math.atan(0.75 * size / up)
    positions = [centre + (0.0, 0.0, up)]
    for k in range(7):
        az = 2.0 * math.pi * k / 7.0
        positions.append(centre + (up * math.tan(math.radians(30)) * math.cos(az), up * math.tan(math.radians(30)) * math.sin(az), up))
    views = [capi.dsm_ortho_view(camera(pos, centre, (size, size), fov), frame) for pos in positions]
    gen = torch.Generator("cuda").manual_seed(1)
    images = [torch.randint(0, 256, (size, size), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(8)]
    flat = torch.rand((h, w), device="cuda", generator=gen) * 0.2
    towers = flat.clone()
    towers.view(h // 64, 64, w // 64, 64)[:, 28:36, :, 28:36] = 40.0
    maps = {"flat": flat, "towers": towers}

    ortho, seen, which = (torch.empty((h, w), dtype=torch.uint8, device="cuda") for _ in range(3))
    ws = capi.dev_bytes(int(LIB.ssrlcv_hip_dsm_ortho_workspace_bytes(u32(w), u32(h), u32(8))))

    def copy_of(nbytes):
        a, b = capi.dev_bytes(nbytes // 2), capi.dev_bytes(nbytes // 2)
        return summary(timed(lambda: b.copy_(a), repeats))

    for name, height in maps.items():
        for m in (1, 3, 8):
            arr = (capi.OrthoView * m)()
            for k in range(m):
                ctypes.memmove(ctypes.byref(arr[k]), ctypes.byref(views[k]), ctypes.sizeof(capi.OrthoView))
                arr[k].image = images[k].data_ptr()
            for steps in (0, 64, 256):
                params = capi.OrthoParams(steps, 0.5, capi.ORTHO_MEDIAN)
                s = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_dsm_ortho(capi.ptr(height), ctypes.byref(frame), arr, u32(m), ctypes.byref(params),
                                                                              capi.ptr(ortho), capi.ptr(seen), capi.ptr(which), capi.ptr(ws),
                                                                              capi.c_sz(ws.numel()), capi.stream_ptr())), repeats))
                seeing = int(sum((seen & (1 << k)).ne(0).sum().item() for k in range(m)))
                check = "%08x" % (int(ortho.to(torch.int64).sum().item()) * 31 + int(seen.to(torch.int64).sum().item()) * 7 +
                                  int(which.to(torch.int64).sum().item()) & 0xFFFFFFFF)
                nbytes = (4 + 3) * w * h + 4 * seeing
                c = copy_of(nbytes)
                s.update(bytes=nbytes, seeing=seeing, copy_ms=c["ms"], over_copy=round(s["ms"] / c["ms"], 2),
                         over_block_matching=round(s["ms"] / sad["ms"], 4), checksum=check)
                res["%s/m%d/steps%d" % (name, m, steps)] = s
                say("  %-7s m = %d maxSteps %3d  %9.4f ms (%.4f .. %.4f); %5.2f views see a cell; at least %6.1f MB, whose copy takes %.4f ms: "
                    "%7.2f x the copy, %.4f x block matching; checksum %s" % (name, m, steps, s["ms"], s["min_ms"], s["max_ms"], seeing / float(w * h),
                                                                              nbytes / 1e6, c["ms"], s["over_copy"], s["over_block_matching"], check))

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a" if append else "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
