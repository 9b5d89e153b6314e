"""Developer tool: the two-nearest matcher next to the one-nearest one, n x n descriptors of bench.py's matcher leg, one
process, the library ssrlcv_amd/_lib.py loads (release by default).  Median of `iters` timed calls each:

  match_knn2                       pack + k_match2_i8 + merge + decode
  match_ratio                      ... + ratio test / finalise
  match_ratio, mutual              ... + the reverse one-nearest pass
  match (mode 0)                   the existing brute-force call, at bench.py's threshold (200^2) and at an infinite one

usage: bench_knn2.py [n] [iters]     (default 262144, 5).  A fused two-best kernel has to beat running the one-nearest matcher
twice: the last line is knn2 / match and must stay below 2."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from ssrlcv_amd import _lib, capi  # noqa: E402


def median_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def main():
    torch.cuda.set_device(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    q, t = bench.synth_descriptors(n, 1), bench.synth_descriptors(n, 2)
    rng = np.random.default_rng(3)  # bench_matcher's data: 25 % planted near-duplicates (+-3)
    dup, tgt = rng.choice(n, n // 4, replace=False), rng.choice(n, n // 4, replace=False)
    t["values"][tgt] = np.clip(q["values"][dup].astype(np.int32) + rng.integers(-3, 4, (len(dup), 128)), 0, 255)
    q_d, t_d = capi.to_dev(q), capi.to_dev(t)
    ws2, ws1 = capi.match2_workspace(n, n), capi.match_workspace(n, n)
    out = capi.dev_bytes(n * 48)
    inf = 3.0e9
    p_bench = capi.make_match_params(0, 0, 1, 0.0, 0.0, 0.6, 200.0 * 200.0)
    p_inf = capi.make_match_params(0, 0, 1, 0.0, 0.0, 0.6, inf)
    r_plain = capi.make_ratio_params(0, 1, ratio=0.8, absolute=inf, mutual=False)
    r_mutual = capi.make_ratio_params(0, 1, ratio=0.8, absolute=inf, mutual=True)
    rows = [
        ("match_knn2", lambda: capi.match_knn2(q_d, n, t_d, n, workspace=ws2)),
        ("match_ratio (ratio 0.8)", lambda: capi.match_ratio(q_d, n, t_d, n, r_plain, capi.OUT_DMATCH, workspace=ws2, out=out)),
        ("match_ratio (ratio 0.8, mutual)", lambda: capi.match_ratio(q_d, n, t_d, n, r_mutual, capi.OUT_DMATCH, workspace=ws2, out=out)),
        ("match, mode 0, threshold 200^2", lambda: capi.match(q_d, n, t_d, n, p_bench, capi.OUT_DMATCH, workspace=ws1, out=out)),
        ("match, mode 0, no threshold", lambda: capi.match(q_d, n, t_d, n, p_inf, capi.OUT_DMATCH, workspace=ws1, out=out)),
    ]
    print("%d x %d descriptors, %d iterations each, %s library" % (n, n, iters, _lib.flavour()))
    ms = {}
    for name, fn in rows:
        ms[name] = median_ms(fn, iters)
        print("  %-34s %9.3f ms   %.0f TOP/s" % (name, ms[name], 2.0 * 128.0 * n * n / (ms[name] * 1e-3) / 1e12))
    for base in ("match, mode 0, threshold 200^2", "match, mode 0, no threshold"):
        print("  match_knn2 / %-28s %.3f  (must stay below 2)" % (base, ms["match_knn2"] / ms[base]))


if __name__ == "__main__":
    main()
