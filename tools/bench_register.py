#!/usr/bin/env python
"""Developer tool: surface registration (include/ssrlcv_hip.h "surface registration") on the library ssrlcv_amd/_lib.py loads
(release by default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: the MESH difference call of
surface accuracy and plain device copies of the same run are the yardsticks, the spread of identical repeats is the noise.

The reference is the terrain of tools/scene.py's scene at the centres of a size^2 grid (4096 by default); the subject is that
terrain plus noise of a twentieth of a cell with 5 % holes, its valid cells as points through ssrlcv_hip_dsm_points (about 15.9 M
points in raster order), and the same points shuffled, the unorganised case.  Every buffer is allocated beforehand, one warm-up and
`repeats` timed runs between stream events, medians with min and max.
  register_terms     on the raster and on the shuffled cloud, under a pose a third of a cell off the identity; beside it the MESH
                     difference call on the same posed cloud and a device copy of 12 B a point, both timed before AND after the
                     terms call in the same job
  transform_points   against a device copy of 24 B a point (12 read, 12 written)
  surface_register   8 iterations on the raster cloud, with a gate of 3 NMAD and without one: host wall time around a
                     synchronise, read-backs, host steps and the gate's statistics calls included

usage: bench_register.py [repeats] [--size N] [--out FILE]   (defaults 9, 4096, profiles/register_bench.txt)"""
import ctypes
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ssrlcv_amd import _lib, capi, pipeline  # noqa: E402
from bench_stereo import commit, take, timed  # noqa: E402


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "register_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    repeats = max(3, int(args[0])) if args else 9
    assert torch.cuda.is_available(), "bench_register.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    w = h = size
    res = dict(tool="bench_register", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_register %s commit %s library %s on %s: %d^2, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, repeats))

    # the scene's terrain over the patch, a cell of one world unit (tools/bench_accuracy.py's inputs)
    import scene
    gsd = scene.PATCH_KM / size
    jj, ii = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    terrain = scene.Scene(64, gsd, torch.device("cuda")).height((ii + 0.5 - w / 2) * gsd, (jj + 0.5 - h / 2) * gsd)
    truth = (terrain / gsd).contiguous()                                 # heights in cells
    del terrain, ii, jj
    gen = torch.Generator("cuda").manual_seed(1)
    subject = truth + 0.05 * torch.randn((h, w), device="cuda", generator=gen)
    subject.view(torch.int32)[torch.rand((h, w), device="cuda", generator=gen) < 0.05] = capi.STEREO_INVALID_BITS
    fr = capi.DsmFrame.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1.0, w, h)
    raster, n = capi.dsm_points(subject, fr)
    raster = raster.contiguous()
    shuffled = raster[torch.randperm(n, device="cuda", generator=gen)].contiguous()
    cells = capi.disparity_mesh(truth, 1, float("inf"))[1]
    del subject
    say("reference: %d x %d terrain, relief %.1f cells; subject: %d points, noise 0.05 cells" % (w, h, float(truth.max() - truth.min()), n))
    res["points"] = n

    angle = 1e-4
    pose = capi.RegisterPose.make([[np.cos(angle), -np.sin(angle), 0], [np.sin(angle), np.cos(angle), 0], [0, 0, 1]], (0.3, -0.2, 0.1), (w / 2, h / 2, 0))
    params = capi.RegisterParams(0.0, float("inf"))
    ws = capi.dev_bytes(int(LIB.ssrlcv_hip_register_terms_workspace_bytes(u32(n))))
    record = torch.empty(304, dtype=torch.uint8, device="cuda")
    diff = torch.empty((n,), dtype=torch.float32, device="cuda")
    posed = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    half12, other12 = capi.dev_bytes(6 * n), capi.dev_bytes(6 * n)      # a copy that moves 12 B a point: 6 read, 6 written
    half24, other24 = capi.dev_bytes(12 * n), capi.dev_bytes(12 * n)

    def show(key, label, s, extra=""):
        res[key] = s
        say("  %-46s %9.4f ms (%.4f .. %.4f)%s" % (label, s["ms"], s["min_ms"], s["max_ms"], extra))

    for cloud_name, cloud in (("raster", raster), ("shuffled", shuffled)):
        capi.transform_points(cloud, pose, out=posed)
        mesh = lambda: capi.check(LIB.ssrlcv_hip_dsm_difference(capi.ptr(posed), u32(n), capi.ptr(truth), ctypes.byref(fr), capi.ptr(cells),  # noqa: E731
                                                                capi.ptr(diff), capi.stream_ptr()))
        terms = lambda: capi.check(LIB.ssrlcv_hip_register_terms(capi.ptr(cloud), u32(n), ctypes.byref(pose), capi.ptr(truth), ctypes.byref(fr),  # noqa: E731
                                                                 capi.ptr(cells), ctypes.byref(params), capi.ptr(record), capi.ptr(ws), capi.c_sz(ws.numel()),
                                                                 capi.stream_ptr()))
        before_mesh, before_copy = summary(timed(mesh, repeats)), summary(timed(lambda: other12.copy_(half12), repeats))
        t = summary(timed(terms, repeats))
        after_mesh, after_copy = summary(timed(mesh, repeats)), summary(timed(lambda: other12.copy_(half12), repeats))
        rec = capi.RegisterTerms.from_buffer_copy(record.cpu().numpy().tobytes())
        mesh_ms, copy_ms = 0.5 * (before_mesh["ms"] + after_mesh["ms"]), 0.5 * (before_copy["ms"] + after_copy["ms"])
        t.update(used=int(rec.used), inside=int(rec.inside), over_mesh_difference=round(t["ms"] / mesh_ms, 2), over_copy_12B=round(t["ms"] / copy_ms, 2))
        show("mesh_difference/%s/before" % cloud_name, "MESH difference, %s, before" % cloud_name, before_mesh)
        show("copy12/%s/before" % cloud_name, "copy of 12 B a point, before", before_copy)
        show("terms/%s" % cloud_name, "register_terms, %s (used %d of %d)" % (cloud_name, rec.used, n), t,
             ": %.2f x the MESH difference, %.2f x the copy" % (t["over_mesh_difference"], t["over_copy_12B"]))
        show("mesh_difference/%s/after" % cloud_name, "MESH difference, %s, after" % cloud_name, after_mesh)
        show("copy12/%s/after" % cloud_name, "copy of 12 B a point, after", after_copy)

    c24 = summary(timed(lambda: other24.copy_(half24), repeats))
    tr = summary(timed(lambda: capi.transform_points(raster, pose, out=posed), repeats))
    tr.update(over_copy_24B=round(tr["ms"] / c24["ms"], 2))
    show("copy24", "copy of 24 B a point", c24)
    show("transform", "transform_points", tr, ": %.2f x the copy" % tr["over_copy_24B"])
    del half12, other12, half24, other24, shuffled

    start = capi.RegisterPose.make(None, (0.8, -0.6, 0.5))
    for gate in (3.0, None):
        times = []
        for k in range(3):   # the first is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = pipeline.surface_register(raster, truth, fr, dof="rigid", iterations=8, gate=gate, initial=start)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        s = summary(times[1:])
        s.update(iterations=len(got["history"]), converged=bool(got["converged"]), rms=[round(x["rms"], 5) for x in got["history"]])
        show("surface_register/%s" % ("gate3" if gate else "no_gate"), "surface_register, 8 iterations, %s" % ("gate 3 NMAD" if gate else "no gate"), s,
             ": %d iterations, rms %.4f -> %.4f cells" % (s["iterations"], got["history"][0]["rms"], got["history"][-1]["rms"]))

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
