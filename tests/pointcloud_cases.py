"""The point-cloud leg's cases off the golden fixtures: random camera rigs and MatchSets, the hand-made degenerate tables,
and the exact structure of the kernels' error sums.  Shared by tests/test_pointcloud_cases.py (which proves on the CPU
oracle alone that the cases test something) and tests/test_gpu_pointcloud_edges.py (which holds csrc/pointcloud.hip to
that oracle).  No GPU, no torch.

The sizes are the smallest that cross every seam of csrc/pointcloud.hip: one thread per bundle, a wave of 64 lanes reduces
its errors with a fixed xor butterfly (device_math.h wave_sum: 32, 16, 8, 4, 2, 1) and adds one float atomically per wave,
a block is 256 threads, and ba_sweep2 walks its K parameter sets with a stride of gridDim.y (at most 2048 / blocks, a power
of two).  So: 1, 63 / 64 / 65 (one wave, full, the second one), 255 / 256 / 257 (one block, full, the second one), 1000."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import helpers as H

NCAM = 7                                         # generate_bundles, triangulate2, triangulateN
SWEEP_NCAM = 5                                   # ba_sweep2
GEN_SIZES = (1, 255, 256, 257, 1000)
TRI_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
# (n, K): K = 1300 at four blocks is gridDim.y = 512 -> three passes of the stride loop for k < 276, two above;
# K = 2500 at one block is gridDim.y = 2048 -> two passes for k < 452
SWEEP_CASES = ((1, 612), (63, 1), (64, 7), (65, 612), (257, 64), (1000, 612), (1000, 1300), (65, 2500))
# Seeds of the sweep cases: every case must give K distinct float32 sums, 95 % of them further than 4 bounds from every
# other (tests/test_pointcloud_cases.py).  2500 sums spread over some 10^6 float32 values collide at the birthday rate,
# about two pairs a seed, and 1300 sums of 16 waves are twice as dense as the 612 the 95 % was set for (seeds j = 0..3 gave
# 91.8, 92.5, 93.7 and 94.2 %, j = 4 gives 95.4 %): these two cases take the first seed of the sequence
# 4000 + 7 n + K + 10000 j that meets both conditions.
SWEEP_SEED_STEP = {(1000, 1300): 4, (65, 2500): 7}
EMBED_N, EMBED_AT = 300, (63, 64, 255)           # last lane of a wave, first lane of the next, last thread of a block
POS_SIGMA, ROT_SIGMA = 1.0, 0.05                 # km, rad: the sweep's perturbations of every camera of every set
SENTINEL = 0x5A5A5A5A                            # prefill of output buffers (as a float 1.5e16: never a result here)


# ---- builders ------------------------------------------------------------------------------------------------------------
def rig(ncam, rng):
    """ncam cameras anywhere, looking anywhere, with non-square images"""
    cams = np.zeros(ncam, H.CAMERA)
    cams["cam_pos"] = rng.uniform(-50.0, 50.0, (ncam, 3))
    cams["cam_rot"] = rng.uniform(-np.pi, np.pi, (ncam, 3))
    cams["fov"] = rng.uniform(0.05, 1.2, (ncam, 2))
    cams["foc"] = rng.uniform(0.01, 0.5, ncam)
    size = rng.integers(200, 5001, (ncam, 2))
    eq = size[:, 0] == size[:, 1]
    size[eq, 1] = np.where(size[eq, 1] < 5000, size[eq, 1] + 1, 200)
    cams["size"] = size
    return cams


def matchset(n, ncam, lo, hi, rng):
    """-> (MultiMatch[n], KeyPoint[sum numKeyPoints]): lo..hi key points per bundle from any cameras in any order, some of them
    outside the image, and the bundles' key-point runs laid out in a random order, so that `index` is not monotone"""
    mm = np.zeros(n, H.MULTIMATCH)
    num = rng.integers(lo, hi + 1, n).astype(np.uint32)
    order = rng.permutation(n)                   # order[j]: the bundle whose run comes j-th in the key-point array
    start = np.concatenate([[0], np.cumsum(num[order])[:-1]]).astype(np.int32)
    mm["numKeyPoints"] = num
    mm["index"][order] = start
    nk = int(num.sum())
    kp = np.zeros(nk, H.KEYPOINT)
    kp["parentId"] = rng.integers(0, ncam, nk)
    kp["loc"] = rng.uniform(-100.0, 5100.0, (nk, 2))
    return mm, kp


def bundles_of(index, num):
    b = np.zeros(len(index), H.BUNDLE)
    b["index"], b["numLines"] = index, num
    return b


# ---- the error sums --------------------------------------------------------------------------------------------------------
def wave_partials(err):
    """device_math.h wave_sum in numpy: the float32 value lane 0 of every wave adds to the sum.  err: (..., n) -> (..., W),
    W = ceil(n / 64).  (The idle lanes of the last wave hold 0; a block's waves past n add 0.0f, which changes nothing.)"""
    err = np.ascontiguousarray(err, np.float32)
    n = err.shape[-1]
    W = (n + 63) // 64
    v = np.zeros(err.shape[:-1] + (W * 64,), np.float32)
    v[..., :n] = err
    v = v.reshape(err.shape[:-1] + (W, 64))
    lane = np.arange(64)
    with np.errstate(over="ignore", invalid="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[..., lane ^ o]).astype(np.float32)
    return v[..., 0]


def sum_bound(partials):
    """|float32 sum of the W partials in any order - their exact sum| <= (W - 1) 2^-24 sum |p_w|: each of the W - 1 additions
    rounds a partial sum no larger than sum |p_w| by at most half an ulp.  Zero for one wave: that sum is 0 + p exactly."""
    p = np.asarray(partials, np.float64)
    return (p.shape[-1] - 1) * 2.0 ** -24 * np.abs(p).sum(-1)


def sum_reference(partials):
    with np.errstate(invalid="ignore"):
        return np.asarray(partials, np.float64).sum(-1)


def same(a, b):
    """element-wise: the same bit pattern, or NaN on both sides (x86 gives 0xFFC00000 for 0 / 0 and a GPU need not);
    infinities and zeros must match in bits"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def sum_agrees(got, err):
    """an error sum a kernel returned against the errors it summed -> (ok, text).  One wave: the butterfly's value, bit for
    bit.  More: within sum_bound of the exact sum of the partials.  NaN or inf exactly when the partials' sum is."""
    got = np.float32(got)
    p = wave_partials(err)
    ref, bound = float(sum_reference(p)), float(sum_bound(p))
    text = "got %r, reference %r, bound %g, %d waves" % (float(got), ref, bound, p.shape[-1])
    if not np.isfinite(ref):
        return bool(same(got, np.float32(ref))), text
    if p.shape[-1] == 1:
        return bool(got.view(np.uint32) == p[0].view(np.uint32)), text
    return bool(np.isfinite(got) and abs(float(got) - ref) <= bound), text


def pick_cutoff(err):
    """one bundle's own error with at least one larger error present (where there are two values at all): that bundle
    stays valid under the strict compare, something above it is flagged"""
    u = np.unique(err[np.isfinite(err)])
    return float(u[(len(u) - 1) // 2])


# ---- inputs and oracle results, computed once and never modified ----------------------------------------------------------------
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bundle_input(n):
    """generate_bundles: -> (cameras, MultiMatch, KeyPoint), 7 cameras, 2 to 9 key points per bundle"""
    def make():
        rng = np.random.default_rng(1000 + n)
        cams = rig(NCAM, rng)
        return (cams,) + matchset(n, NCAM, 2, 9, rng)
    return _once(("bundle", n), make)


def two_view_input(lib, n):
    """triangulate2: -> (bundles, lines), the oracle's lines of a random two-key-point MatchSet over 7 cameras"""
    def make():
        rng = np.random.default_rng(2000 + n)
        cams = rig(NCAM, rng)
        mm, kp = matchset(n, NCAM, 2, 2, rng)
        b, l, _ = H.oracle_bundles(lib, mm, kp, cams)
        return b, l
    return _once(("two", n), make)


def n_view_input(lib, n):
    """triangulateN: 2 to 9 lines per bundle, every line's vec scaled by a factor in [0.5, 3] (not unit length)"""
    def make():
        rng = np.random.default_rng(3000 + n)
        cams = rig(NCAM, rng)
        mm, kp = matchset(n, NCAM, 2, 9, rng)
        b, l, _ = H.oracle_bundles(lib, mm, kp, cams)
        l["vec"] = l["vec"] * rng.uniform(0.5, 3.0, (len(l), 1)).astype(np.float32)
        return b, l
    return _once(("nview", n), make)


def triangulate_ref(lib, nview, bundles, lines, cutoff=None, invalid_before=0):
    """the oracle on copies -> dict(points, errors, invalid, sum); points is SENTINEL-filled first, so that a point the
    oracle leaves unwritten (N-view, singular S) shows"""
    n = len(bundles)
    b = bundles.copy()
    b["invalid"] = invalid_before
    pts = np.full((n, 3), SENTINEL, np.uint32).view(np.float32)
    errs = np.zeros(n, np.float32)
    cut = np.array([cutoff], np.float32) if cutoff is not None else None
    f = lib.oracle_n_view_triangulate if nview else lib.oracle_two_view_triangulate
    with np.errstate(all="ignore"):
        total = f(ctypes.c_uint32(n), H.P(lines), H.P(b), H.P(pts), H.P(errs), H.P(cut))
    return {"points": pts, "errors": errs, "invalid": b["invalid"].copy(), "sum": np.float32(total)}


# ---- degenerate tables -----------------------------------------------------------------------------------------------------
# classes: "nan" (0 / 0: point and error NaN), "residue" (parallel lines whose cross product is the rounding residue of
# fma(a, b, -(c d)), not zero: finite), "finite", "inf" (the squared gap overflows; the point is finite),
# "singular" (N-view: det S == 0 exactly, the point is not written), "either" (bit-equal to the oracle whichever it is)
def degenerate_two_view():
    """-> (bundles, lines, classes): rows of two lines (vec, pnt, vec, pnt)"""
    rows = [
        ("nan", (0, 0, 1), (0, 0, 0), (0, 0, 1), (1, 0, 0)),                    # parallel along z through different points
        ("nan", (0, 0, 1), (0, 0, 0), (0, 0, -1), (0, 2, 0)),                   # antiparallel
        ("residue", (0.6, 0.8, 0), (0, 0, 0), (0.6, 0.8, 0), (0, 0, 0)),        # the same oblique line twice
        ("residue", (0.6, 0.8, 0), (0, 0, 0), (0.6, 0.8, 0), (1, 2, 3)),        # oblique parallel, different points
        ("finite", (1, 0, 0), (0, 0, 0), (0, 1, 0), (3, -2, 0)),                # meet exactly in (3, 0, 0)
        ("inf", (1, 0, 0), (0, 0, 0), (0, 1, 0), (0, 0, 3e19)),                 # gap 3e19: its square overflows
    ]
    lines = np.zeros(2 * len(rows), H.LINE)
    for i, (_, v1, p1, v2, p2) in enumerate(rows):
        lines["vec"][2 * i], lines["pnt"][2 * i] = v1, p1
        lines["vec"][2 * i + 1], lines["pnt"][2 * i + 1] = v2, p2
    return bundles_of(2 * np.arange(len(rows)), 2), lines, [r[0] for r in rows]


def degenerate_n_view():
    """-> (bundles, lines, classes); bundles 0 and 2 are ordinary neighbours of the singular one"""
    rows = [
        ("finite", [((1, 0, 0), (0, 0, 0)), ((0, 1, 0), (0, 0, 0))]),
        ("singular", [((0, 0, 1), (0, 0, 0)), ((0, 0, 1), (1, 0, 0))]),          # error 0.5 from the point (0, 0, 0)
        ("finite", [((0, 2, 0), (1, 1, 1)), ((0, 0, 0.5), (1, 0, 2)), ((3, 0, 0), (0, 1, 2))]),
        ("either", [((0.6, 0.8, 0), (0, 0, 0)), ((0.6, 0.8, 0), (1, 2, 3)), ((0.6, 0.8, 0), (-2, 0, 1))]),
        ("finite", [((1, 0, 0), (0, 1, 0)), ((0, 0, 0), (5, 5, 5)), ((0, 1, 0), (1, 0, 2))]),   # a zero vec in the middle
        ("nan", [((1, 0, 0), (0, 1, 0)), ((0, 1, 0), (1, 0, 2)), ((0, 0, 0), (5, 5, 5))]),      # ... last: its error is 0 / 0
    ]
    num = np.array([len(r[1]) for r in rows])
    lines = np.zeros(int(num.sum()), H.LINE)
    i = 0
    for _, ls in rows:
        for v, p in ls:
            lines["vec"][i], lines["pnt"][i] = v, p
            i += 1
    return bundles_of(np.concatenate([[0], np.cumsum(num)[:-1]]), num), lines, [r[0] for r in rows]


def embedded(lib, nview, first):
    """table rows first, first + 1, first + 2 in place of bundles 63, 64 and 255 of a 300-bundle random case
    -> (bundles, lines, {position: class})"""
    def make():
        b, l = (n_view_input if nview else two_view_input)(lib, EMBED_N)
        tb, tl, tc = (degenerate_n_view if nview else degenerate_two_view)()
        b, at = b.copy(), {}
        for j, g in enumerate(EMBED_AT):
            r = (first + j) % len(tb)
            b["index"][g] = len(l) + tb["index"][r]   # the table's lines follow the case's
            b["numLines"][g] = tb["numLines"][r]
            at[g] = tc[r]
        return b, np.concatenate([l, tl]), at
    return _once(("embedded", nview, first), make)


def embedded_firsts(nview):
    return tuple(range(0, len((degenerate_n_view if nview else degenerate_two_view)()[0]), len(EMBED_AT)))


# ---- ba_sweep2 -------------------------------------------------------------------------------------------------------------
def sweep_input(n, K):
    """-> (cameras, MultiMatch, KeyPoint, params[K, 5 * 6]): pairs of key points from any two of 5 cameras in either order;
    set 0 is the rig itself, every other set moves every camera by N(0, 1) km and turns it by N(0, 0.05) rad"""
    def make():
        rng = np.random.default_rng(4000 + 7 * n + K + 10000 * SWEEP_SEED_STEP.get((n, K), 0))
        cams = rig(SWEEP_NCAM, rng)
        mm, kp = matchset(n, SWEEP_NCAM, 2, 2, rng)
        if n == 1:
            kp["parentId"] = [3, 1]                # one bundle: two different cameras, the higher one first
        base = np.concatenate([cams["cam_pos"], cams["cam_rot"]], 1).astype(np.float32)
        params = np.tile(base.reshape(1, SWEEP_NCAM, 6), (K, 1, 1))
        params[1:, :, :3] += rng.normal(0.0, POS_SIGMA, (K - 1, SWEEP_NCAM, 3)).astype(np.float32)
        params[1:, :, 3:] += rng.normal(0.0, ROT_SIGMA, (K - 1, SWEEP_NCAM, 3)).astype(np.float32)
        return cams, mm, kp, np.ascontiguousarray(params.reshape(K, SWEEP_NCAM * 6))
    return _once(("sweep", n, K), make)


def sweep_errors(lib, cams, mm, kp, params):
    """the oracle's per-bundle errors of every parameter set: generate_bundles with that set's cam_pos / cam_rot, then the
    two-view triangulation -> float32 (K, n)"""
    K, n = len(params), len(mm)
    out = np.zeros((K, n), np.float32)

    def run(ks):                                    # the oracle calls release the GIL: a few threads share the K sets
        c = cams.copy()
        bundles, lines = np.zeros(n, H.BUNDLE), np.zeros(len(kp), H.LINE)
        for k in ks:
            p = params[k].reshape(len(cams), 6)
            c["cam_pos"], c["cam_rot"] = p[:, :3], p[:, 3:]
            lib.oracle_generate_bundles(ctypes.c_uint32(n), H.P(mm), H.P(kp), H.P(c), H.P(bundles), H.P(lines))
            lib.oracle_two_view_triangulate(ctypes.c_uint32(n), H.P(lines), H.P(bundles), None, H.P(out[k]), None)

    threads = max(1, min(8, H.cpu_budget(), K * n // 100000))
    if threads == 1:
        run(range(K))
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(run, [range(t, K, threads) for t in range(threads)]))
    return out


def sweep_partials(lib, n, K):
    """the reference of one ba_sweep2 case: wave partials (K, W) of the oracle's errors"""
    def make():
        cams, mm, kp, params = sweep_input(n, K)
        return wave_partials(sweep_errors(lib, cams, mm, kp, params))
    return _once(("sweep_partials", n, K), make)


def fixture_sweep(lib):
    """the 612 parameter sets tests/test_gpu_pointcloud.py::test_ba_sweep_matches_oracle builds on the two-view fixture
    -> (MultiMatch, KeyPoint, cameras, params, partials)"""
    def make():
        v = H.load_view("Pipeline2View")
        mm, kp, cams = v["mm1"], v["kp1"], v["cameras"]
        base = np.concatenate([np.concatenate([c["cam_pos"], c["cam_rot"]]) for c in cams]).astype(np.float32)
        rng = np.random.default_rng(5)
        K = 612
        params = np.tile(base, (K, 1))
        for k in range(1, K):
            i, j = rng.integers(0, 12, 2)
            params[k, i] += np.float32(1e-4 if i % 6 < 3 else 1e-5)
            params[k, j] -= np.float32(1e-4 if j % 6 < 3 else 1e-5)
        return mm, kp, cams, params, wave_partials(sweep_errors(lib, cams, mm, kp, params))
    return _once("fixture_sweep", make)


def sums_within(got, partials):
    """K sums of a sweep against their partials -> indices of the sets that miss: bit-equal for one wave, else within
    sum_bound of the exact sum of the partials"""
    got = np.ascontiguousarray(got, np.float32)
    if partials.shape[-1] == 1:
        return np.flatnonzero(got.view(np.uint32) != np.ascontiguousarray(partials[:, 0]).view(np.uint32))
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(~(np.abs(got.astype(np.float64) - sum_reference(partials)) <= sum_bound(partials)))
