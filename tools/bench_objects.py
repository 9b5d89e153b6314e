#!/usr/bin/env python
"""Developer tool: surface objects (include/ssrlcv_hip.h "surface objects") on the library ssrlcv_amd/_lib.py loads (release by
default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: a plain device copy of the bytes a
call must move at least -- the map once, plus ids: 8 bytes a cell --, measured in the same run, is the yardstick, and the spread of
identical repeats is the noise.

Four object-height maps at size^2 (4096 by default): `scene`, the `objects` map of tools/bench_terrain.py's chain behind
pipeline.surface_terrain, and the three adversarial ones: `whole`, one object over the whole map (every tile flushes into one
record); `checker`, the one-cell checkerboard (the most objects a map can hold); `none`, no member at all.  Every buffer is
allocated beforehand, one warm-up and `repeats` timed runs between stream events, medians with min and max.  Per map:
  call        ssrlcv_hip_dsm_objects, ids and every record written, beside the copy
  lab         tools/objects_lab.hip on the same map in a child process: the reduction alone (the shipped form: runs of a wave, then
              LDS per tile-local root, one flush per tile, object and field), the naive form (one global atomic per cell and
              field), the labelling alone, the copy, and whether the two forms left equal bytes
Every row also as a multiple of the 2.31 ms matching call the README measures every stage against.

usage: bench_objects.py [repeats] [--size N] [--out FILE]      (defaults 7, 4096, profiles/objects_bench.txt)"""
import ctypes
import datetime
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ssrlcv_amd import _lib, capi, pipeline  # noqa: E402
from bench_stereo import commit, take, timed  # noqa: E402
from bench_terrain import scene_map, summary  # noqa: E402

LAB = os.path.join(ROOT, "tools", "_build", "objects_lab")
MATCH_MS = 2.31
MIN_HEIGHT = 1.0
LAB_LINE = re.compile(r"(\d+) objects; reduction ([\d.]+) ms \(([\d.]+) \.\. ([\d.]+)\), naive ([\d.]+) ms \(([\d.]+) \.\. ([\d.]+)\), "
                      r"labelling ([\d.]+) ms \(([\d.]+) \.\. ([\d.]+)\), copy of 8 B a cell ([\d.]+) ms, equal (\d)")


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "objects_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    repeats = max(3, int(args[0])) if args else 7
    assert torch.cuda.is_available(), "bench_objects.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    res = dict(tool="bench_objects", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size, match_ms=MATCH_MS, min_height=MIN_HEIGHT, rows={})
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_objects %s commit %s library %s on %s: %d^2, min height %.1f, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, MIN_HEIGHT, repeats))
    height, frame = scene_map(size)
    scene = pipeline.surface_terrain(height, frame, 128, 0.3, 0.5, 3.0, want_level=False)["objects"].contiguous()
    del height
    h, w = scene.shape
    gen = torch.Generator("cuda").manual_seed(7)
    noise = torch.rand((h, w), device="cuda", generator=gen)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    maps = [("scene", scene), ("whole", MIN_HEIGHT + 1.0 + noise), ("checker", torch.where((xx + yy) % 2 == 0, MIN_HEIGHT + 1.0 + noise, noise * 0.5)),
            ("none", noise * 0.5)]
    del yy, xx
    for name, objects in maps:
        objects = objects.contiguous()
        cells = w * h
        p = capi.ObjectParams(MIN_HEIGHT, float("inf"), 256.0, 1)
        ws = capi.dev_bytes(int(LIB.ssrlcv_hip_dsm_objects_workspace_bytes(u32(w), u32(h))))
        count, _, _ = capi.dsm_objects(objects, MIN_HEIGHT, capacity=0, want_ids=False, workspace=ws)
        ids = torch.empty((h, w), dtype=torch.int32, device="cuda")
        records = torch.empty(max(count, 1) * 13, dtype=torch.int64, device="cuda")
        count_d = torch.zeros(1, dtype=torch.int32, device="cuda")
        t = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_dsm_objects(capi.ptr(objects), u32(w), u32(h), ctypes.byref(p), capi.ptr(ids), capi.ptr(records),
                                                                        u32(count), capi.ptr(count_d), capi.ptr(ws), capi.c_sz(ws.numel()), capi.stream_ptr())),
                          repeats))
        a, b = capi.dev_bytes(4 * cells), capi.dev_bytes(4 * cells)   # 4 B a cell read, 4 B a cell written
        c8 = summary(timed(lambda: b.copy_(a), repeats))
        del a, b
        row = dict(w=w, h=h, objects=count, members=int((ids >= 0).sum()), call=t, copy_ms=c8["ms"], over_copy=round(t["ms"] / c8["ms"], 2),
                   over_match=round(t["ms"] / MATCH_MS, 2))
        say("%s: %d x %d cells, %d members in %d objects" % (name, w, h, row["members"], count))
        say("  call             %8.4f ms (%.4f .. %.4f); its 8 B a cell copy in %.4f ms: %6.2f x the copy, %5.2f x the matching call" % (
            t["ms"], t["min_ms"], t["max_ms"], c8["ms"], row["over_copy"], row["over_match"]))
        del ids, records, ws
        if os.path.exists(LAB):
            with tempfile.NamedTemporaryFile(suffix=".raw") as f:
                objects.cpu().numpy().tofile(f.name)
                lab = subprocess.run([LAB, str(w), str(h), f.name, str(MIN_HEIGHT), str(repeats)], capture_output=True, text=True, timeout=900)
            m = LAB_LINE.search(lab.stdout)
            if lab.returncode == 0 and m and int(m.group(1)) == count:
                v = [float(x) for x in m.groups()[1:11]]
                row["lab"] = dict(reduction_ms=v[0], reduction_min=v[1], reduction_max=v[2], naive_ms=v[3], naive_min=v[4], naive_max=v[5], labelling_ms=v[6],
                                  labelling_min=v[7], labelling_max=v[8], copy_ms=v[9], equal=int(m.group(12)))
                for what, k in (("reduction", 0), ("naive form", 3), ("labelling", 6)):
                    say("  lab %-12s %8.4f ms (%.4f .. %.4f): %6.2f x the copy, %5.2f x the matching call" % (
                        what, v[k], v[k + 1], v[k + 2], v[k] / v[9], v[k] / MATCH_MS))
                say("  lab              the shipped reduction takes %.2f x the naive form's time; equal bytes %d; the lab's copy %.4f ms" % (
                    v[0] / v[3], int(m.group(12)), v[9]))
            else:
                row["lab"] = "failed (%d): %s" % (lab.returncode, (lab.stdout + lab.stderr).strip()[-300:])
                say("  lab              %s" % row["lab"])
        res["rows"][name] = row
        del objects
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
