"""The cases that hold the hot SIFT sampling kernels (k_thetas, k_desc_consts, k_descriptors of csrc/keypoints.hip) to the CPU
oracle OFF the default parameters and off the key points a detector happens to find.  Shared by tests/test_sampling_cases.py
(which proves on the oracle alone that the cases reach what they claim) and tests/test_gpu_sampling.py (which holds the kernels
to the oracle).  Nothing here imports torch or the HIP library.

Part 1, PLAN_CASES: plan parameters (maxOrientations, orientationThreshold, orientationContribWidth, descriptorContribWidth)
through the whole key-point stage on two synthetic images.

Part 2, SETS: hand-placed key-point lists, written into a plan's workspace between two stage calls (stages 0..5 run, the
lists and state words of the four octaves are overwritten, stages 6 and 7 run; the "theta" sets carry their own theta and are
written after stage 6, in front of stage 7 alone).  The builder enforces the preconditions
that keep the kernels inside memory; a placement that cannot meet them is dropped HERE, never on the GPU side:
  - blur in {1, 2, 3} (the levels that have polar tables); the list is sorted by blur and idx is its ordered partition;
  - n <= CAPACITY; hasExtrema = (n > 0); discard = 0;
  - sigma / pixelWidth < 8 (the bound ssrlcv_sift_plan_create's window check assumes);
  - every key point passes checkKeyPoints at the plan's descriptor width, evaluated in float32 as the oracle does.
A key point whose ORIENTATION window leaves the level is legal: it gets no orientation on either side."""
from collections import namedtuple
from multiprocessing.pool import ThreadPool

import numpy as np

import helpers as H

f32 = np.float32
CAPACITY = 4096            # max_keypoints_per_octave of every plan the hand-placed lists go into
IMAGES = {"256x192": (256, 192, 5), "384x256": (384, 256, 1)}   # name -> (w, h, seed of H.synthetic_image)
PLACED_IMAGE = (256, 256, 5)

# ---- the window arithmetic, in float32 and in the oracle's operand order (oracle/oracle_sift.c) ---------------------------


def desc_extent(sigma, dw, pw):
    """checkKeyPoints' ww = sigma * lambda / pixelWidth"""
    return (np.asarray(sigma, f32) * f32(dw)) / f32(pw)


def desc_half(sigma, dw, pw):
    """fillDescriptors' windowWidth = ceilf(sigma * lambda / pixelWidth)"""
    return np.ceil(desc_extent(sigma, dw, pw))


def ori_half(sigma, ow, pw):
    """computeThetas' windowWidth = ceilf(sigma * 3 * lambda / pixelWidth)"""
    return np.ceil(((np.asarray(sigma, f32) * f32(3.0)) * f32(ow)) / f32(pw))


def passes_check(x, y, sigma, dw, pw, w, h):
    """checkKeyPoints' predicate (oracle_sift.c check_keypoints): True = kept"""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    ww = desc_extent(sigma, dw, pw)
    return ~((x - ww < f32(0)) | (y - ww < f32(0)) | (x + ww >= f32(w - 1)) | (y + ww >= f32(h - 1)))


def has_orientation_window(x, y, sigma, ow, pw, w, h):
    """computeThetas' early return, negated: the orientation window lies inside the level"""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    wo = ori_half(sigma, ow, pw)
    return ~((x - wo < f32(0)) | (y - wo < f32(0)) | (x + wo >= f32(w - 1)) | (y + wo >= f32(h - 1)))


def llround(v):
    """llroundf of float32 values (halves away from zero), exactly"""
    v = np.asarray(v, f32).astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


# ---- part 1 ----------------------------------------------------------------------------------------------------------------
# features: the oracle's count on the 256 x 192 image; ori / desc: (min, max) half-width of the orientation / descriptor window
# over the key points that pass checkKeyPoints at the case's dw (None: not pinned for this row)
PlanCase = namedtuple("PlanCase", "maxo thr ow dw features ori desc why")
PLAN_CASES = {
    "maxo3": PlanCase(3, 0.8, 1.5, 6.0, 1194, (9, 22), (11, 29), "k_thetas<3>"),
    "thr0.5": PlanCase(4, 0.5, 1.5, 6.0, 1997, (9, 22), (11, 29), "third and fourth slots filled"),
    "thr0.05": PlanCase(4, 0.05, 1.5, 6.0, 3334, (9, 22), (11, 29), "nearly every local peak kept"),
    "thr1.0": PlanCase(2, 1.0, 1.5, 6.0, 838, (9, 22), (11, 29), "only the maximum survives (= the stage-5 count)"),
    "ow0.1": PlanCase(2, 0.8, 0.1, 6.0, 841, (1, 2), (11, 29), "orientation half-window 1..2, minx below one chunk"),
    "ow0.4": PlanCase(2, 0.8, 0.4, 6.0, 1109, (3, 6), (11, 29), "orientation half-window 3..6"),
    "ow5": PlanCase(2, 0.8, 5.0, 6.0, 967, (27, 72), (11, 29), "orientation half-window 27..72, rows of many chunks"),
    "dw0.2": PlanCase(2, 0.8, 1.5, 0.2, 1200, (9, 22), (1, 1), "descriptor window 1 for every key point"),
    "dw0.5": PlanCase(2, 0.8, 1.5, 0.5, 1200, (9, 22), (1, 3), "descriptor windows 1..3"),
    "dw1": PlanCase(2, 0.8, 1.5, 1.0, 1200, (9, 22), (2, 5), "descriptor windows 2..5"),
    "dw12": PlanCase(2, 0.8, 1.5, 12.0, 905, None, (22, 58), "descriptor windows 22..58"),
    "dw30": PlanCase(2, 0.8, 1.5, 30.0, 408, None, (58, 141), "descriptor windows 58..141; checkKeyPoints empties octaves 2-3"),
    "both_max": PlanCase(4, 0.3, 5.0, 30.0, 1196, None, (58, 141), "both extremes together"),
    "both_min": PlanCase(1, 1.0, 0.1, 0.2, 1004, (1, 2), (1, 1), "both minima together"),
}
# the rows that also run on the 384 x 256 image (other per-octave counts, more key points at the left edge)
WIDE_IMAGE_CASES = [n for n, c in PLAN_CASES.items() if c.dw in (0.2, 30.0) or c.ow in (0.1, 5.0) or c.maxo == 3]
ENTRY_POINT_CASES = ["dw0.2", "dw30", "ow5"]          # build_dog + describe and stages 0..7, next to extract
SCHEDULE_CASES = ["ow0.1", "ow5", "dw0.2", "dw30"]    # the rows every developer schedule runs in a child process
EXPORT_CASES = {"exports_small": (4, 0.8, 0.4, 1.0), "exports_max": (4, 0.8, 5.0, 30.0)}   # maxo, thr, ow, dw


def image(name):
    w, h, seed = IMAGES[name]
    return H.synthetic_image(w, h, seed=seed)


_SIFT = {}


def oracle_scale_space(key):
    """one OracleSift per image (an IMAGES name or "placed"), created once and shared"""
    if key not in _SIFT:
        w, h, seed = PLACED_IMAGE if key == "placed" else IMAGES[key]
        _SIFT[key] = H.OracleSift(H.oracle(), H.synthetic_image(w, h, seed=seed))
    return _SIFT[key]


_FEATURES = {}


def oracle_features(image_name, maxo, thr, ow, dw):
    """OracleSift.features of one parameter set, computed once and shared; never modified"""
    key = (image_name, maxo, thr, ow, dw)
    if key not in _FEATURES:
        _FEATURES[key] = oracle_scale_space(image_name).features(maxo, thr, ow, dw)
    return _FEATURES[key]


_STAGE4 = {}


def checked_lists(image_name, dw):
    """The oracle's stage-4 list (after removeEdges) filtered by checkKeyPoints at `dw` -> per octave (SSKEYPOINT[], idx[5]):
    what stage 5 leaves at that descriptor width."""
    if image_name not in _STAGE4:
        _STAGE4[image_name] = oracle_scale_space(image_name).keypoints(4)
    kps, idx = _STAGE4[image_name]
    s = oracle_scale_space(image_name)
    out, pos = [], 0
    for o in range(4):
        w, h, pw, _ = s.octave_info(o)
        lst = kps[pos:pos + int(idx[o][5])]
        pos += int(idx[o][5])
        keep = passes_check(lst["loc"][:, 0], lst["loc"][:, 1], lst["sigma"], dw, pw, w, h) if len(lst) else np.zeros(0, bool)
        lst = lst[keep].copy()
        out.append((lst, partition_by_blur(lst)))
    return out


def partition_by_blur(lst):
    """extremaBlurIndices of a list sorted by blur: idx[b] = the number of key points with a smaller blur"""
    assert np.all(np.diff(lst["blur"]) >= 0)
    return np.array([int((lst["blur"] < b).sum()) for b in range(5)], np.int32)


def window_ranges(image_name, ow, dw):
    """-> ((min, max) orientation half-width, (min, max) descriptor half-width, key points) over checked_lists"""
    s = oracle_scale_space(image_name)
    wo, wd = [], []
    for o, (lst, _) in enumerate(checked_lists(image_name, dw)):
        pw = s.octave_info(o)[2]
        wo.append(ori_half(lst["sigma"], ow, pw))
        wd.append(desc_half(lst["sigma"], dw, pw))
    wo, wd = np.concatenate(wo), np.concatenate(wd)
    return (int(wo.min()), int(wo.max())), (int(wd.min()), int(wd.max())), len(wo)


# ---- the per-key-point reference chain (parts 1 and 2) ------------------------------------------------------------------------
def chain_reference(levels, geoms, lists, maxo, thr, ow, dw, oriented=False):
    """The oracle's computeThetas / expansion / fillDescriptors, one key point at a time, over per-octave lists:
    levels[o][b]: the twice-normalised DoG level; geoms[o] = (w, h, pixelWidth); lists[o] = SSKEYPOINT[] sorted by blur.
    oriented: the lists already carry their theta (no orientation step).
    -> {"expanded": [SSKEYPOINT[] per octave], "idx": [int32[5] per octave], "norient": [int[] per octave],
        "features": FEATURE[] (octaves concatenated)}"""
    lib = H.oracle()
    pool = ThreadPool(H.cpu_budget())      # (ctypes calls release the GIL; the per-key-point oracle calls share nothing)
    expanded, idxs, norient, feats = [], [], [], []
    for o, lst in enumerate(lists):
        pw = geoms[o][2]
        out, cnt = [], []
        if oriented:
            per_kp = [[kp["theta"]] for kp in lst]
        else:
            per_kp = pool.map(lambda kp: H.oracle_thetas(lib, levels[o][int(kp["blur"])], pw, ow, kp, maxo, thr), lst)
        for kp, thetas in zip(lst, per_kp):
            cnt.append(len(thetas))
            for t in thetas:
                e = kp.copy()
                e["theta"] = t
                out.append(e)
        exp = np.array(out, H.SSKEYPOINT) if out else np.zeros(0, H.SSKEYPOINT)
        expanded.append(exp)
        idxs.append(partition_by_blur(exp))
        norient.append(np.array(cnt, np.int64))
        feats += pool.map(lambda e: H.oracle_descriptor(lib, levels[o][int(e["blur"])], pw, dw, e), exp)
    pool.close()
    return {"expanded": expanded, "idx": idxs, "norient": norient,
            "features": np.concatenate(feats) if feats else np.zeros(0, H.FEATURE)}


# ---- part 2: hand-placed key points -------------------------------------------------------------------------------------------
PAIRS = {"default": (1.5, 6.0), "small": (0.4, 1.0), "max": (5.0, 30.0), "min": (0.1, 0.2)}    # (ow, dw)
SEGMENT_SIZES = {"1_0_1": (1, 0, 1), "63_64_65": (63, 64, 65), "15_16_17": (15, 16, 17)}      # key points of blur 1, 2, 3
FRACTIONS = (0.0, 0.5, 0.25, 0.75)
PLACED_MAXO, PLACED_THR = 4, 0.5     # several orientations per key point where the histogram has them
Geometry = namedtuple("Geometry", "w h pw sigma")


def geometry(o):
    """octave o of a 256 x 256 plan, as ssrlcv_sift_plan_create lays it out (float32 sigma ladder)"""
    sig = [f32(np.sqrt(f32(2.0))) / f32(2.0)]
    for _ in range(5):
        sig.append(f32(sig[-1] * f32(np.sqrt(f32(2.0)))))
    side = (2 * PLACED_IMAGE[0]) >> o
    return Geometry(side, (2 * PLACED_IMAGE[1]) >> o, f32(0.5 * 2 ** o), np.array(sig, f32) * f32(2 ** o))


def record(o, b, x, y, sigma, theta=-1.0):
    kp = np.zeros(1, H.SSKEYPOINT)
    kp["octave"], kp["blur"], kp["loc"], kp["sigma"], kp["theta"] = o, b, (f32(x), f32(y)), f32(sigma), f32(theta)
    kp["intensity"] = f32(0.25)
    return kp


def integer_extent_sigmas(own, dw, pw):
    """-> [sigma with sigma * dw / pw an exact integer, sigma with it just above that integer] near `own`, each only if
    sigma / pw < 8 keeps holding.  "Just above" is the smallest float32 quotient above the integer that a sigma reaches: one
    ulp wherever sigma's own spacing, scaled by dw / pw, does not step over it."""
    k = max(1.0, float(np.rint(desc_extent(own, dw, pw))))
    s = f32(f32(k) * f32(pw) / f32(dw))
    for _ in range(64):                     # walk onto the integer (the quotient is monotone in sigma)
        q = desc_extent(s, dw, pw)
        if q == f32(k):
            break
        s = np.nextafter(s, f32(np.inf) if q < f32(k) else f32(0))
    out = []
    if desc_extent(s, dw, pw) == f32(k):
        out.append(s)
        a = s
        while desc_extent(a, dw, pw) == f32(k):
            a = np.nextafter(a, f32(np.inf))
        out.append(a)
    return [v for v in out if v / f32(pw) < f32(8.0)]


def placements(pair, o, b):
    """the hand-placed key points of blur b of octave o at the parameter pair, BEFORE the preconditions -> [(x, y, sigma)]"""
    ow, dw = PAIRS[pair]
    g = geometry(o)
    W1, H1 = f32(g.w - 1), f32(g.h - 1)
    cx, cy = f32(g.w // 2), f32(g.h // 2)
    inf, zero = f32(np.inf), f32(0)
    own = g.sigma[b]
    sigmas = [own] + integer_extent_sigmas(own, dw, g.pw)
    if pair == "max" and o == 0 and b == 3:
        sigmas.append(f32(3.99))     # descriptor half-width 240 (57 840 orbit indices), orientation half-width 120 (241 columns)
    out = []
    for n, s in enumerate(sigmas):
        m = np.maximum(desc_extent(s, dw, g.pw), ori_half(s, ow, g.pw))   # the larger of ww and the orientation half-width
        # corners: the window touches the level's border exactly; one ulp inward; one ulp outward (kept where it passes)
        lo, hi_x, hi_y = m, np.nextafter(W1 - m, zero), np.nextafter(H1 - m, zero)
        for (x, xin), (y, yin) in (((lo, inf), (lo, inf)), ((hi_x, zero), (lo, inf)), ((lo, inf), (hi_y, zero))):
            xout, yout = (zero if xin == inf else inf), (zero if yin == inf else inf)
            out.append((x, y, s))
            out.append((np.nextafter(x, xin), np.nextafter(y, yin), s))
            out.append((np.nextafter(x, xout), np.nextafter(y, yout), s))
        out.append((cx, cy, s))
        if pair == "max" and s == f32(3.99):
            continue
        # rounding ties on the window's first column: x - windowWidth on a half-integer (orientation, then descriptor window)
        out.append((ori_half(s, ow, g.pw) + f32(2.5), cy, s))
        out.append((desc_half(s, dw, g.pw) + f32(1.5), cy + f32(0.5), s))
        if n:
            continue
        # fractions, at the centre and a few columns off the left edge (either side of the orientation kernel's chunk widths)
        for k in (None, 0.5, 31.5, 32.0, 33.0):
            px = cx if k is None else f32(np.ceil(m) + f32(k))
            for fx in FRACTIONS:
                for fy in FRACTIONS:
                    if pair == "max" and fx != fy:     # (the widest windows cost the oracle 10 ms each: the diagonal only)
                        continue
                    out.append((f32(px + f32(fx)), f32(cy + f32(fy)), s))
    return out


def enforce(o, dw, kps):
    """the preconditions (module docstring) on one octave's candidate list -> (SSKEYPOINT[] sorted by blur, idx[5])"""
    g = geometry(o)
    if len(kps):
        keep = passes_check(kps["loc"][:, 0], kps["loc"][:, 1], kps["sigma"], dw, g.pw, g.w, g.h)
        keep &= (kps["blur"] >= 1) & (kps["blur"] <= 3) & (kps["sigma"] / g.pw < f32(8.0)) & (kps["sigma"] > 0)
        keep &= np.isfinite(kps["loc"]).all(1)
        kps = kps[keep]
        kps = kps[np.argsort(kps["blur"], kind="stable")]
    kps = kps[:CAPACITY].copy()
    kps["discard"], kps["pad"], kps["octave"] = 0, 0, o
    return kps, partition_by_blur(kps)


def check_preconditions(o, dw, kps, idx):
    """asserts what enforce() promises (tests/test_sampling_cases.py runs it on every set)"""
    g = geometry(o)
    assert len(kps) <= CAPACITY and (kps["discard"] == 0).all() and (kps["octave"] == o).all()
    assert np.isin(kps["blur"], (1, 2, 3)).all() and np.all(np.diff(kps["blur"]) >= 0)
    assert np.array_equal(idx, partition_by_blur(kps)) and idx[0] == 0 and idx[1] == 0 and idx[4] == len(kps)
    assert (kps["sigma"] / g.pw < f32(8.0)).all()
    assert passes_check(kps["loc"][:, 0], kps["loc"][:, 1], kps["sigma"], dw, g.pw, g.w, g.h).all()


PlacedSet = namedtuple("PlacedSet", "kind pair oriented")   # kind: "place", "theta", "segments"
SETS = {}
for _p in PAIRS:
    SETS["place_" + _p] = PlacedSet("place", _p, False)
    SETS["theta_" + _p] = PlacedSet("theta", _p, True)
for _n in SEGMENT_SIZES:
    SETS["segments_" + _n] = PlacedSet("segments", "default", False)
SETS["segments_63_64_65_min"] = PlacedSet("segments", "min", False)


BORDER_THETAS = (f32(0), f32(np.pi / 4), f32(1.0), f32(4.0))


def forced_thetas():
    """0, k pi / 4 (k = 1..7) as float32, each with its two float32 neighbours, and the float below 2 pi"""
    base = [f32(0)] + [f32(k * np.pi / 4) for k in range(1, 8)]
    out = []
    for t in base:
        out += [t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf))]
    out.append(np.nextafter(f32(2 * np.pi), f32(0)))
    return out


def strongest_gradient_near_centre(o, b, dw):
    """the legal pixel within 8 of the level's centre with the largest central-difference gradient: a 3 x 3 descriptor window (the
    smallest width) on a flat spot of the level would collect no vote at all, and a descriptor without votes is 0 / 0"""
    lvl = placed_levels()[o][b]
    cy, cx = lvl.shape[0] // 2, lvl.shape[1] // 2
    sub = lvl[cy - 9:cy + 10, cx - 9:cx + 10].astype(np.float64)
    mag = np.hypot(sub[1:-1, 2:] - sub[1:-1, :-2], sub[2:, 1:-1] - sub[:-2, 1:-1])
    g = geometry(o)
    xs, ys = np.meshgrid(np.arange(cx - 8, cx + 9), np.arange(cy - 8, cy + 9))
    mag = np.where(passes_check(xs, ys, g.sigma[b], dw, g.pw, g.w, g.h), mag, -1.0)   # (only where a key point is legal)
    # ... at which every forced theta collects votes: the reference drops a sample whose direction relative to theta comes
    # out below -45 degrees (fmodf keeps the sign), and the nine samples of a 3 x 3 window can all point that way
    for flat in np.argsort(-mag, axis=None):
        iy, ix = np.unravel_index(int(flat), mag.shape)
        if mag[iy, ix] < 0:
            break
        x, y = cx - 8 + int(ix), cy - 8 + int(iy)
        if all(has_votes(o, dw, record(o, b, x, y, g.sigma[b], t)[0]) for t in forced_thetas()):
            return x, y
    return None     # (dw = 30 in octave 2: no blur-2 or blur-3 window fits the level)


_BUILT = {}


def build_set(name):
    """-> [(SSKEYPOINT[], idx[5]) per octave 0..3]; octave 3 is always empty (built once and shared; never modified)"""
    if name not in _BUILT:
        _BUILT[name] = _build_set(name)
    return _BUILT[name]


def has_votes(o, dw, kp):
    """the oracle's descriptor of an oriented key point collects at least one vote (without any its bytes are 0 / 0)"""
    return bool(H.oracle_descriptor(H.oracle(), placed_levels()[o][int(kp["blur"])], geometry(o).pw, dw, kp)["values"].any())


def _build_set(name):
    spec = SETS[name]
    ow, dw = PAIRS[spec.pair]
    lists = []
    for o in range(3):
        g = geometry(o)
        recs = []
        for b in (1, 2, 3):
            if spec.kind == "place":
                recs += [record(o, b, x, y, s) for (x, y, s) in placements(spec.pair, o, b)]
            elif spec.kind == "theta":
                at = strongest_gradient_near_centre(o, b, dw)
                if at is not None:
                    recs += [record(o, b, at[0], at[1], g.sigma[b], t) for t in forced_thetas()]
                # Descriptor windows that touch the level's border exactly.  An oriented list needs no orientation window, so
                # this is the one way to the table's padding where the orientation half-width is the wider margin (3 ow > dw).
                for s in [g.sigma[b]] + integer_extent_sigmas(g.sigma[b], dw, g.pw):
                    ww = desc_extent(s, dw, g.pw)
                    far_x, far_y = np.nextafter(f32(g.w - 1) - ww, f32(0)), np.nextafter(f32(g.h - 1) - ww, f32(0))
                    for cxy in ((ww, ww), (far_x, ww), (ww, far_y), (far_x, far_y)):
                        border = [record(o, b, cxy[0], cxy[1], s, t) for t in BORDER_THETAS]
                        # (the smallest windows, 3 x 3 samples in a level's flat corner, collect no vote: dropped here)
                        recs += [r for r in border if passes_check(cxy[0], cxy[1], s, dw, g.pw, g.w, g.h) and has_votes(o, dw, r[0])]
            else:
                sizes = SEGMENT_SIZES[name.split("segments_")[1].replace("_min", "")]
                # copies of the centre key point, moved by whole pixels so that the windows differ
                recs += [record(o, b, g.w // 2 + (i % 9) - 4, g.h // 2 + ((i // 9) % 9) - 4, g.sigma[b]) for i in range(sizes[b - 1])]
        cand = np.concatenate(recs) if recs else np.zeros(0, H.SSKEYPOINT)
        lists.append(enforce(o, dw, cand))
    lists.append(enforce(3, dw, np.zeros(0, H.SSKEYPOINT)))
    return lists


_LEVELS = {}


def placed_levels():
    """levels[o][b] of the placed image: the oracle's twice-normalised DoG (bit-equal to the plan's, test_dog_pyramid_bit_exact)"""
    if not _LEVELS:
        s = oracle_scale_space("placed")
        for o in range(4):
            _LEVELS[o] = [s.level(2, o, b) for b in range(5)]
    return _LEVELS


_REFERENCE = {}


def reference(name):
    """chain_reference of one set, computed once and shared; never modified"""
    if name not in _REFERENCE:
        spec = SETS[name]
        ow, dw = PAIRS[spec.pair]
        lists = build_set(name)
        geoms = [tuple(geometry(o)[:3]) for o in range(4)]
        _REFERENCE[name] = chain_reference(placed_levels(), geoms, [l for l, _ in lists], PLACED_MAXO, PLACED_THR, ow, dw,
                                           oriented=spec.oriented)
    return _REFERENCE[name]


def descriptor_window_reach(kp, dw, pw):
    """-> (min x, max x, min y, max y) of the rounded sample coordinates of an oriented key point's descriptor window, as
    fill_descriptor walks it (the oracle's own sinf / cosf)"""
    lib = H.oracle()
    theta = np.array([-kp["theta"]], f32)
    c, s = np.zeros(1, f32), np.zeros(1, f32)
    lib.oracle_math_eval(3, H.P(theta), None, H.P(c), 1)
    lib.oracle_math_eval(2, H.P(theta), None, H.P(s), 1)
    c, s = c[0], s[0]
    wc = desc_half(kp["sigma"], dw, pw)
    r = np.arange(-int(wc), int(wc) + 1).astype(f32)
    x, y = np.meshgrid(r, r)
    cxx = (x * c) + (y * s)
    cyy = ((-x) * s) + (y * c)
    ok = ~((np.abs(cxx) > wc) | (np.abs(cyy) > wc))
    px, py = llround(cxx + f32(kp["loc"][0]))[ok], llround(cyy + f32(kp["loc"][1]))[ok]
    return int(px.min()), int(px.max()), int(py.min()), int(py.max())
