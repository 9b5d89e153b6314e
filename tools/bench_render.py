#!/usr/bin/env python
"""Developer tool: the mesh render (include/ssrlcv_hip.h "mesh render") on the library ssrlcv_amd/_lib.py loads (release by
default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: a plain device copy of the bytes a call
must move at least and the block-matching call of the same run are the yardsticks, the spread of identical repeats is the noise.

The model is the terrain of tools/scene.py's scene at the centres of a size^2 grid (4096 by default: 16.8 M vertices, 33.5 M
triangles at step 1), one grey a vertex, joined everywhere; the view has size^2 pixels.  Every buffer is allocated beforehand, one
warm-up and `repeats` timed runs between stream events, medians with min and max.
  nadir          the camera above the centre, a cell a pixel on the ground plane: about one pixel centre a triangle pair
  oblique 30     the same camera 30 degrees off the vertical, aimed at the centre
  zoom 4         the nadir camera with a quarter of the field of view, 4 pixels a cell, at maxExtent 8 and 64
  step 4         the map sampled at every fourth cell (a sixteenth of the vertices, 4 pixels a cell) under the nadir camera
  residual       ssrlcv_hip_image_residual of the nadir render against an image, beside a copy of its 10 B a pixel
The bytes of a render are what it must read and write once: 12 + 1 B a vertex, 4 B a node, 1 B a cell, 4 + 4 + 1 B a pixel; the
accumulators and the projected vertices in the workspace come on top and are not counted.

usage: bench_render.py [repeats] [--size N] [--out FILE] [--append]   (defaults 9, 4096, profiles/render_bench.txt)"""
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
from bench_ortho import D, RADIUS, camera  # noqa: E402
from bench_stereo import commit, make_pair, take, timed  # noqa: E402


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "render_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    append = "--append" in args
    args = [a for a in args if a != "--append"]
    repeats = max(3, int(args[0])) if args else 9
    assert torch.cuda.is_available(), "bench_render.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    w = h = size
    res = dict(tool="bench_render", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_render %s commit %s library %s on %s: a %d^2 map into a %d^2 view, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, size, repeats))

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

    # the scene's terrain over the patch, a cell of one world unit (tools/bench_register.py's reference)
    import scene
    gsd = scene.PATCH_KM / size
    jj, ii = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    terrain = (scene.Scene(64, gsd, torch.device("cuda")).height((ii + 0.5 - w / 2) * gsd, (jj + 0.5 - h / 2) * gsd) / gsd).contiguous()
    del ii, jj
    gen = torch.Generator("cuda").manual_seed(1)
    image = torch.randint(0, 256, (size, size), dtype=torch.uint8, device="cuda", generator=gen)
    say("model: %d x %d terrain, relief %.1f cells, joined everywhere" % (w, h, float(terrain.max() - terrain.min())))

    def model(step):
        sub = terrain[::step, ::step].contiguous()
        fr = capi.DsmFrame.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), float(step), sub.shape[1], sub.shape[0])
        pts, n = capi.dsm_points(sub, fr)
        vi, cells, _ = capi.disparity_mesh(sub, 1, float("inf"))
        grey = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
        return dict(points=pts.contiguous(), n=n, vertex_index=vi, cells=cells, grey=grey, frame=fr)

    centre, up = np.array([w / 2.0, h / 2.0, 0.0]), 5.0 * size
    one_to_one = 2.0 * math.atan(0.5 * size / up)       # a cell a pixel on the ground plane
    lean = up * math.tan(math.radians(30))
    rows = [("nadir", 1, centre + (0.0, 0.0, up), one_to_one, 8), ("oblique 30", 1, centre + (lean, 0.0, up), one_to_one, 8),
            ("zoom 4, maxExtent 8", 1, centre + (0.0, 0.0, up), 2.0 * math.atan(0.125 * size / up), 8),
            ("zoom 4, maxExtent 64", 1, centre + (0.0, 0.0, up), 2.0 * math.atan(0.125 * size / up), 64),
            ("step 4", 4, centre + (0.0, 0.0, up), one_to_one, 8)]

    depth = torch.empty((h, w), dtype=torch.float32, device="cuda")
    triangle = torch.empty((h, w), dtype=torch.int32, device="cuda")
    shade = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")

    def copy_of(nbytes):
        a, b = capi.dev_bytes(nbytes // 2), capi.dev_bytes(nbytes // 2)
        return summary(timed(lambda: b.copy_(a), repeats))

    models = {}
    for name, step, pos, fov, extent in rows:
        if step not in models:
            models.clear()          # one model at a time on the device
            models[step] = model(step)
        m = models[step]
        gh, gw = m["vertex_index"].shape
        view = capi.dsm_ortho_view(camera(pos, centre, (size, size), fov), m["frame"])
        params = capi.RenderParams(extent)
        ws = capi.dev_bytes(int(LIB.ssrlcv_hip_mesh_render_workspace_bytes(u32(m["n"]), u32(w), u32(h))))
        call = lambda: capi.check(LIB.ssrlcv_hip_mesh_render(capi.ptr(m["points"]), u32(m["n"]), capi.ptr(m["grey"]), capi.ptr(m["vertex_index"]),  # noqa: E731
                                                             capi.ptr(m["cells"]), u32(gw), u32(gh), ctypes.byref(view), ctypes.byref(params), capi.ptr(depth),
                                                             capi.ptr(triangle), capi.ptr(shade), capi.ptr(counts), capi.ptr(ws), capi.c_sz(ws.numel()),
                                                             capi.stream_ptr()))
        s = summary(timed(call, repeats))
        drawn, large, unusable = (int(c) for c in counts.cpu().tolist())
        covered = int((triangle != -1).sum().item())
        check = "%08x" % ((int(shade.to(torch.int64).sum().item()) * 31 + int(triangle.to(torch.int64).sum().item()) * 7 +
                           int(depth.view(torch.int32).to(torch.int64).sum().item())) & 0xFFFFFFFF)
        nbytes = 13 * m["n"] + 4 * gw * gh + (gw - 1) * (gh - 1) + 9 * w * h
        del ws
        c = copy_of(nbytes)
        s.update(vertices=m["n"], drawn=drawn, too_large=large, unusable=unusable, covered=covered, bytes=nbytes, copy_ms=c["ms"],
                 over_copy=round(s["ms"] / c["ms"], 2), over_block_matching=round(s["ms"] / sad["ms"], 4), checksum=check)
        res[name] = s
        say("  %-22s %9.4f ms (%.4f .. %.4f); %8d drawn, %d too large, %d unusable, %5.1f %% of the view covered; at least %6.1f MB, whose copy "
            "takes %.4f ms: %6.2f x the copy, %.4f x block matching; checksum %s" % (name, s["ms"], s["min_ms"], s["max_ms"], drawn, large, unusable,
                                                                                     100.0 * covered / (w * h), nbytes / 1e6, c["ms"], s["over_copy"],
                                                                                     s["over_block_matching"], check))
        if name == "nadir":
            out = torch.empty((h, w), dtype=torch.float32, device="cuda")
            r = summary(timed(lambda: capi.image_residual(image, shade, depth, out=out), repeats))
            c = copy_of(10 * w * h)
            r.update(copy_ms=c["ms"], over_copy=round(r["ms"] / c["ms"], 2))
            res["residual"] = r
            say("  %-22s %9.4f ms (%.4f .. %.4f); 10 B a pixel, whose copy takes %.4f ms: %.2f x the copy" % (
                "residual of nadir", r["ms"], r["min_ms"], r["max_ms"], c["ms"], r["over_copy"]))
            del out

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a" if append else "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
