"""Developer tool: dense SIFT (ssrlcv_hip_sift_dense_u8) next to the chain of per-kernel exports that defines its result
(tests/dense_ref.py: u8_to_f32, minmax, normalize, pixel_gradients, compute_thetas, compact_thetas, compact_addresses,
expand_keypoints, fill_descriptors), in one process, on the library ssrlcv_amd/_lib.py loads (release by default).

Two shapes: 1024^2 at stride 1 and 4096^2 at stride 4 (about a million grid points each), sigma 1.6, two orientations.  Per
shape and path one warm-up and `repeats` timed calls between stream events, every buffer allocated beforehand; the chain's
one read-back of the compacted count is part of it, as it is for any caller of the exports.  Prints median / min / max of
both, their ratio, the new path's nanoseconds per feature beside the sparse k_descriptors figure (1.34 ms for
294 041 features, about 4.6 ns), and whether the slowest repeat of the new path beat the fastest of the chain.

usage: bench_dense.py [repeats] [--out FILE]      (default 5)"""
import ctypes
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import dense_ref  # noqa: E402
import helpers as H  # noqa: E402
from ssrlcv_amd import _lib, capi  # noqa: E402

SHAPES = [(1024, 1024, 1), (4096, 4096, 4)]
SPARSE_NS_PER_FEATURE = 1.34e6 / 294041


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
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    repeats = max(5, int(args[0])) if args else 5
    torch.cuda.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("dense SIFT: new entry point vs composed exports; %s; commit %s; %s library; %s" %
        (datetime.date.today().isoformat(), commit(), _lib.flavour(), torch.cuda.get_device_name(0)))
    say("sigma 1.6, maxOrientations 2, one warm-up + %d timed repeats per path, stream events, ms" % repeats)
    verdicts = []
    for w, h, stride in SHAPES:
        img = H.synthetic_image(w, h, seed=17)
        pix = torch.from_numpy(img).cuda()
        p = capi.DenseParams(stride, 1.6, 2, 0.8, 1.5, 6.0)
        _, nx, ny = capi.dense_grid(w, h, p)
        cap = nx * ny * 2
        ws = capi.dense_workspace(w, h, p)
        feats = capi.dev_bytes(cap * 152)
        count = torch.zeros(1, dtype=torch.int32, device="cuda")

        def new_path():
            capi.check(capi.LIB.ssrlcv_hip_sift_dense_u8(capi.ptr(pix), capi.c_u32(w), capi.c_u32(h), ctypes.byref(p), capi.ptr(ws),
                                                         capi.c_sz(ws.numel()), capi.ptr(feats), capi.c_u32(cap), capi.ptr(count),
                                                         capi.stream_ptr()))

        t_new = timed(new_path, repeats)
        n_new = int(count.item())
        chain = dense_ref.Chain(capi, img, stride=stride, sigma=1.6, max_orientations=2)
        n_ref = [0]

        def composed():
            n_ref[0] = chain.run()

        t_ref = timed(composed, repeats)
        same = n_new == n_ref[0] and torch.equal(feats[: n_new * 152].view(-1, 152)[:, 8:], chain.features[: n_new * 152].view(-1, 152)[:, 8:])
        ok = max(t_new) < min(t_ref)
        verdicts.append(ok)
        say("%d x %d, stride %d: %d x %d grid points, %d features (composed: %d, records %s)" %
            (w, h, stride, nx, ny, n_new, n_ref[0], "equal" if same else "DIFFER"))
        say("  new       median %9.3f  min %9.3f  max %9.3f" % (float(np.median(t_new)), min(t_new), max(t_new)))
        say("  composed  median %9.3f  min %9.3f  max %9.3f" % (float(np.median(t_ref)), min(t_ref), max(t_ref)))
        say("  composed / new (medians) %.2f; new path %.2f ns per feature (sparse k_descriptors: %.1f ns)" %
            (float(np.median(t_ref)) / float(np.median(t_new)), 1e6 * float(np.median(t_new)) / max(n_new, 1), SPARSE_NS_PER_FEATURE))
        say("  slowest new repeat %s fastest composed repeat: condition %s" % ("<" if ok else ">=", "met" if ok else "NOT met"))
        del chain, feats, ws
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
