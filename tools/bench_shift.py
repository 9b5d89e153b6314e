#!/usr/bin/env python
"""Developer tool: the shift search (include/ssrlcv_hip.h "shift search") on the library ssrlcv_amd/_lib.py loads (release by
default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: a plain device copy of the two maps'
bytes, one iteration of surface_register on the same cloud and the 2.31 ms matching call, the first two measured in the same
run, are the yardsticks, and the spread of identical repeats is the noise.

The reference is `scene`, the fused map of the chain as tools/bench_terrain.py builds it (about size^2 cells, holes included;
4096 by default); the subject is the cloud of that map 7.3, -4.6 and 0.5 cells off, rasterised into the reference's frame.
Every buffer is allocated beforehand, one warm-up and `repeats` timed runs between stream events, medians with min and max.
  search         ssrlcv_hip_shift_search at stride 1 and radii 4, 8, 16 and 32; at radius 16 also with 30 % of the moving map's
                 cells made holes, and gated at 3 NMAD about the median of the differences at shift 0.  Pairs are the cell
                 pairs inside the grid, summed over the shifts, whether valid or not
  quantise       the same call with a centre so far out that no shift meets the grid: the table's memset, the quantise pass and
                 a search launch whose blocks skip every tile
  shift_search   a whole pipeline.surface_shift_search of the cloud: the rasterisation, strides (4, 1), radius 8, the two gates,
                 the read-backs
Every row also as a multiple of the copy, of the registration iteration and of the matching call.

usage: bench_shift.py [repeats] [--size N] [--out FILE]      (defaults 7, 4096, profiles/shift_bench.txt)"""
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
from ssrlcv_amd import _lib, capi, pipeline  # noqa: E402
from bench_stereo import commit, take, timed  # noqa: E402
from bench_terrain import scene_map, summary  # noqa: E402

INVALID = capi.STEREO_INVALID_BITS
RADII = (4, 8, 16, 32)
MATCH_MS = 2.31
MOTION_CELLS = (7.3, -4.6, 0.5)


def pairs_of(w, h, radius, center=(0, 0)):
    """the cell pairs inside the grid, summed over the shifts of the window"""
    xs = sum(max(0, w - abs(center[0] + k)) for k in range(-radius, radius + 1))
    ys = sum(max(0, h - abs(center[1] + k)) for k in range(-radius, radius + 1))
    return xs * ys


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "shift_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    repeats = max(3, int(args[0])) if args else 7
    assert torch.cuda.is_available(), "bench_shift.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    res = dict(tool="bench_shift", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(), device=torch.cuda.get_device_name(0),
               repeats=repeats, size=size, match_ms=MATCH_MS, rows=[])
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_shift %s commit %s library %s on %s: %d^2, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, repeats))
    reference, frame = scene_map(size)
    h, w = reference.shape
    cell = float(frame.cell)
    cloud = capi.dsm_points(reference, frame)[0]
    ex, ey, ez = (torch.tensor(list(v), dtype=torch.float64) for v in (frame.ex, frame.ey, frame.ez))
    off = (cell * (MOTION_CELLS[0] * ex + MOTION_CELLS[1] * ey + MOTION_CELLS[2] * ez)).to(torch.float32).cuda()
    cloud = (cloud - off).contiguous()                                    # it has to move by +MOTION_CELLS to lie on the reference
    moving = capi.dsm_rasterize(cloud, frame, capi.DSM_MAX, False, False)[0]
    gen = torch.Generator("cuda").manual_seed(7)
    holes = moving.clone()
    holes.view(torch.int32)[torch.rand((h, w), device="cuda", generator=gen) < 0.3] = INVALID
    scale = float(np.float32(64.0 / cell))
    valid = lambda m: int((m.view(torch.int32) != INVALID).sum())  # noqa: E731
    say("scene: %d x %d cells of %.4f, %d valid in the reference, %d in the moving map, %d with the holes; %d points" % (
        w, h, cell, valid(reference), valid(moving), valid(holes), cloud.shape[0]))

    a, b = capi.dev_bytes(8 * w * h), capi.dev_bytes(8 * w * h)
    copy = summary(timed(lambda: b.copy_(a), repeats))
    say("  copy of both maps (8 B a cell read, 8 B written)   %8.4f ms (%.4f .. %.4f)" % (copy["ms"], copy["min_ms"], copy["max_ms"]))
    del a, b
    reg = summary(timed(lambda: pipeline.surface_register(cloud, reference, frame, iterations=1, gate=3.0), repeats))
    say("  one iteration of surface_register, gate 3.0        %8.4f ms (%.4f .. %.4f)" % (reg["ms"], reg["min_ms"], reg["max_ms"]))
    res.update(w=w, h=h, copy=copy, register_iteration=reg)

    ws = capi.dev_bytes(int(LIB.ssrlcv_hip_shift_search_workspace_bytes(u32(w), u32(h), ctypes.byref(capi.ShiftParams(scale, 1, 0, 0, 0, 0, 0)))))
    table = torch.empty(int(LIB.ssrlcv_shift_table_bytes(u32(32))) // 8, dtype=torch.int64, device="cuda")

    def search_row(name, m, radius, center=(0, 0), center_q=0, gate_q=capi.SHIFT_NO_GATE):
        p = capi.ShiftParams(scale, 1, center[0], center[1], radius, center_q, gate_q)
        call = lambda: capi.check(LIB.ssrlcv_hip_shift_search(capi.ptr(m), capi.ptr(reference), u32(w), u32(h), ctypes.byref(p), capi.ptr(table), capi.ptr(ws),  # noqa: E731
                                                              capi.c_sz(ws.numel()), capi.stream_ptr()))
        t = summary(timed(call, repeats))
        pairs = pairs_of(w, h, radius, center)
        t.update(name=name, radius=radius, pairs=pairs, pairs_per_s=round(pairs / (t["ms"] * 1e-3), 1) if pairs else 0.0, over_copy=round(t["ms"] / copy["ms"], 2),
                 over_register=round(t["ms"] / reg["ms"], 3), over_match=round(t["ms"] / MATCH_MS, 2))
        res["rows"].append(t)
        say("  %-22s S %2d %9.4f ms (%.4f .. %.4f); %.3e pairs, %.3e a second; %7.2f x the copy, %6.3f x the registration iteration, %6.2f x the matching call"
            % (name, radius, t["ms"], t["min_ms"], t["max_ms"], pairs, t["pairs_per_s"], t["over_copy"], t["over_register"], t["over_match"]))
        return t

    for radius in RADII:
        search_row("search", moving, radius)
    search_row("search, 30 % holes", holes, 16)
    # the gate of pipeline.surface_shift_search at shift 0
    diff = capi.dsm_subtract(moving, reference)
    signed = capi.difference_stats(diff, quantiles=(5000,))
    mad = float(capi.difference_stats(diff, center=float(signed.quantile[0]), absolute=True, quantiles=(5000,)).quantile[0])
    center_q, gate_q = int(np.rint(float(signed.quantile[0]) * scale)), int(np.floor(3.0 * 1.4826 * mad * scale))
    del diff
    search_row("search, gated %d +- %d" % (center_q, gate_q), moving, 16, center_q=max(-(1 << 18), min(1 << 18, center_q)), gate_q=gate_q)
    search_row("quantise (no shift met)", moving, 0, center=(1 << 24, 0))

    whole = summary(timed(lambda: pipeline.surface_shift_search(cloud, reference, frame, radius=8, strides=(4, 1), gate=3.0), repeats))
    found = pipeline.surface_shift_search(cloud, reference, frame, radius=8, strides=(4, 1), gate=3.0)
    whole.update(shift=list(found["shift"]), bias_cells=found["bias"] / cell, over_copy=round(whole["ms"] / copy["ms"], 2),
                 over_register=round(whole["ms"] / reg["ms"], 3), over_match=round(whole["ms"] / MATCH_MS, 2))
    res["surface_shift_search"] = whole
    say("  surface_shift_search, strides (4, 1), radius 8, gate 3.0: %8.4f ms (%.4f .. %.4f), allocations and read-backs included; %.2f x the copy, %.3f x the "
        "registration iteration, %.2f x the matching call; found (%.3f, %.3f) cells and a bias of %.3f cells for a motion of %s"
        % (whole["ms"], whole["min_ms"], whole["max_ms"], whole["over_copy"], whole["over_register"], whole["over_match"], found["shift"][0], found["shift"][1],
           whole["bias_cells"], MOTION_CELLS))

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
