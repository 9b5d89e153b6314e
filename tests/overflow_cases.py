"""The cases that hold the key-point lists' OVERFLOW to its contract (include/ssrlcv_hip.h above ssrlcv_sift_plan_overflow): a
list that outgrows the plan's capacity is truncated AT the capacity in the reference's order (blur 1, 2, 3, raster order inside a
blur), the octave's bit is set in the mask, the call returns SSRLCV_ERR_CAPACITY.  Shared by tests/test_overflow_cases.py (which
proves on the oracle alone that every capacity falls where it is claimed to fall) and tests/test_gpu_overflow.py (which holds the
device code to the truncated reference, bit for bit).  Nothing here imports torch or the HIP library.

Truncation, restated: the reference's list of an octave (unbounded), cut after `cap` records; the blur indices clamped to `cap`.
The two places a list can outgrow the capacity:
  extrema     the first list of the key-point stage.  The fused calls (extract, describe) compact the extrema behind the first
              removeNoise, so THEIR first list is the oracle's stage-1 list; the stage call and a describe stopped at stage 0
              produce the raw stage-0 list.
  expansion   computeKeyPointOrientations writes one record per orientation: the stage-6 list can be up to maxOrientations
              times the stage-5 list.

References are computed once per process and never modified.  With SSRLCV_OVERFLOW_CACHE set to a directory they are also kept
there as .npz files: the child processes of the schedule test load what the parent computed."""
import os
from collections import namedtuple

import numpy as np

import helpers as H
import sampling_cases as C

FLOOR = 4096          # ssrlcv_sift_plan_create raises a smaller maxKeyPointsPerOctave to this
OK, ERR_CAPACITY = 0, -2


# ---- the images ---------------------------------------------------------------------------------------------------------------
def _noise(w, h):
    return np.random.default_rng(1).integers(0, 256, (h, w), dtype=np.uint8)


def _sparse512():
    """512 x 512 with few extrema in octave 0: the 256 x 256 synthetic image, every pixel doubled, under a 3 x 3 box filter"""
    up = np.kron(H.synthetic_image(256, 256, seed=4), np.ones((2, 2), np.uint8)).astype(np.int64)
    a = np.pad(up, 1, mode="reflect")
    s = sum(a[dy:dy + 512, dx:dx + 512] for dy in range(3) for dx in range(3))
    return ((2 * s + 9) // 18).astype(np.uint8)      # (the sum of nine over 9, halves up, in integers)


IMAGES = {
    "noise256": lambda: _noise(256, 256),
    "syn512": lambda: H.synthetic_image(512, 512, seed=4),
    "noise768": lambda: _noise(768, 768),       # raw blur-1 count of octave 0 above 4096: a cut inside blur 1
    "noise512": lambda: _noise(512, 512),       # the host mirror's two re-runs
    "sparse512": _sparse512,                    # fits 4096 at every stage of both paths
}
_IMG = {}


def image(name):
    if name not in _IMG:
        _IMG[name] = IMAGES[name]()
    return _IMG[name]


# ---- the oracle, once per process (and per cache directory) ----------------------------------------------------------------------
_MEM, _SIFT = {}, {}


def _cached(key, compute):
    """compute() -> a tuple of numpy arrays; kept in memory, and under SSRLCV_OVERFLOW_CACHE when that is set"""
    d = os.environ.get("SSRLCV_OVERFLOW_CACHE")
    path = os.path.join(d, key + ".npz") if d else None
    if key not in _MEM:
        if path and os.path.exists(path):
            with np.load(path) as z:
                _MEM[key] = tuple(z["a%d" % i] for i in range(len(z.files)))
        else:
            _MEM[key] = tuple(compute())
    if path and not os.path.exists(path):
        np.savez(path + ".tmp.npz", **{"a%d" % i: a for i, a in enumerate(_MEM[key])})
        os.replace(path + ".tmp.npz", path)
    return _MEM[key]


def scale_space(name):
    """one OracleSift per image, created once and shared"""
    if name not in _SIFT:
        _SIFT[name] = H.OracleSift(H.oracle(), image(name))
    return _SIFT[name]


def _split(kps, idx):
    out, pos = [], 0
    for o in range(4):
        n = int(idx[o][5])
        out.append((kps[pos:pos + n], np.array(idx[o][:5], np.int32)))
        pos += n
    return out


def lists(name, stage):
    """the oracle's lists after `stage` (0 raw extrema .. 5 checkKeyPoints, 6 orientations at maxOrientations 2, threshold 0.8)
    -> [(SSKEYPOINT[], idx int32[5]) per octave]"""
    kps, idx = _cached("%s_stage%d" % (name, stage), lambda: scale_space(name).keypoints(stage))
    return _split(kps, idx)


def counts(name, stage):
    """-> [[idx0..idx4, n] per octave]"""
    return [[int(v) for v in idx] + [len(l)] for l, idx in lists(name, stage)]


def features(name, maxo=2, thr=0.8):
    """OracleSift.features at the default widths -> FEATURE[] (octaves concatenated, list order)"""
    return _cached("%s_features_%d_%g" % (name, maxo, thr), lambda: (scale_space(name).features(maxo, thr, 1.5, 6.0),))[0]


def chain(name, maxo, thr):
    """sampling_cases.chain_reference on the oracle's stage-5 lists: the stage-6 lists and the features at any maxOrientations /
    threshold -> ([(SSKEYPOINT[], idx[5]) per octave], [FEATURE[] per octave])"""
    def compute():
        s = scale_space(name)
        levels = {o: [s.level(2, o, b) for b in range(5)] for o in range(4)}
        geoms = [s.octave_info(o)[:3] for o in range(4)]
        r = C.chain_reference(levels, geoms, [l for l, _ in lists(name, 5)], maxo, thr, 1.5, 6.0)
        return _pack(r)
    return _unpack(_cached("%s_chain_%d_%g" % (name, maxo, thr), compute))


def _pack(r):
    """chain_reference's result -> (expanded, counts[4], idx[4, 5], features)"""
    n = np.array([len(e) for e in r["expanded"]], np.int64)
    return np.concatenate(r["expanded"]), n, np.array(r["idx"], np.int32), r["features"]


def _unpack(packed):
    exp, n, idx, feats = packed
    ends = np.cumsum(n)
    return ([(exp[e - k:e], idx[o]) for o, (e, k) in enumerate(zip(ends, n))],
            [feats[e - k:e] for e, k in zip(ends, n)])


def features_per_octave(name):
    """features(name) split by the stage-6 counts -> [FEATURE[] per octave]"""
    f, out, pos = features(name), [], 0
    for l, _ in lists(name, 6):
        out.append(f[pos:pos + len(l)])
        pos += len(l)
    assert pos == len(f)
    return out


# ---- truncation ------------------------------------------------------------------------------------------------------------------
def state_words(idx, n, overflow):
    """the eight state words of ssrlcv_sift_plan_keypoints: idx[0..4], n, hasExtrema, overflow"""
    return np.array([int(v) for v in idx] + [n, 1 if n else 0, overflow], np.int32)


def truncate_extrema(lst, idx, cap):
    """the first list of the key-point stage under capacity `cap` -> (SSKEYPOINT[], state words[8])"""
    if len(lst) <= cap:
        return lst, state_words(idx, len(lst), 0)
    c1, c12 = int(idx[2]), int(idx[3])     # blur-1 records, blur-1 and blur-2 records
    return lst[:cap], state_words([0, 0, min(c1, cap), min(c12, cap), cap], cap, 1)


def truncate_expanded(expanded, idx, cap):
    """the stage-6 list under capacity `cap` -> (SSKEYPOINT[], state words[8])"""
    if len(expanded) <= cap:
        return expanded, state_words(idx, len(expanded), 0)
    return expanded[:cap], state_words([min(int(v), cap) for v in idx], cap, 1)


def truncated_features(per_octave, kept):
    """stage 7 books from the state words: the reference features of the first kept[o] expanded key points of every octave, one
    octave behind the other"""
    return np.concatenate([f[:n] for f, n in zip(per_octave, kept)])


def mask_of(states):
    return sum(int(st[7]) << o for o, st in enumerate(states))


def where(idx, n, cap):
    """where capacity `cap` falls in a list of n records with blur indices idx -> a set of labels"""
    if n <= cap:
        return {"fits"} | ({"exact fit"} if n == cap else set())
    out = {"one too many"} if n == cap + 1 else set()
    assert int(idx[4]) == n
    for b in (1, 2, 3):
        first, last = int(idx[b]), int(idx[b + 1])      # blur b's segment
        if first < cap < last:
            out.add("inside blur %d" % b)
        if b > 1 and cap == first < last and first > int(idx[b - 1]):
            out.add("on the blur %d/%d boundary" % (b - 1, b))
    return out


# ---- the capacity tables ---------------------------------------------------------------------------------------------------------
# (image, capacity) -> what the capacity does to octave 0's list (labels of where())
Case = namedtuple("Case", "image cap claim")
# set_stop_stage(0) + describe and build_dog + stage(0): the raw stage-0 list
STAGED_EXTREMA = [
    Case("noise256", 4096, {"inside blur 2"}),
    Case("noise256", 4134, {"on the blur 2/3 boundary"}),
    Case("noise256", 4135, {"inside blur 3"}),              # one blur-3 record is left
    Case("noise256", 6470, {"inside blur 3", "one too many"}),
    Case("noise256", 6471, {"exact fit"}),
    Case("syn512", 4096, {"inside blur 2"}),
    Case("noise768", 4096, {"inside blur 1"}),              # book_extrema's c1 clamp: idx = [0, 0, 4096, 4096, 4096]
]
# extract and build_dog + describe stopped at stage 1: the stage-1 list
FUSED_EXTREMA = [
    Case("syn512", 4096, {"inside blur 3"}),
    Case("syn512", 4755, {"inside blur 3", "one too many"}),
    Case("syn512", 4756, {"exact fit"}),
    Case("noise256", 4096, {"inside blur 2"}),
    Case("noise256", 6459, {"exact fit"}),
]
# the full fused extract at the defaults: the extrema fit, the claim is about the stage-6 list
EXPANSION = [
    Case("syn512", 5413, {"exact fit"}),
    Case("syn512", 5412, {"inside blur 3", "one too many"}),
    Case("syn512", 4756, {"inside blur 3"}),
]
# ... and at four orientations per key point: e / maxOrientations across the cut (reference: chain())
EXPANSION_MAXO4 = Case("noise256", 6459, {"inside blur 2"})
MAXO4, THR4 = 4, 0.5
# octaves 1-3 fit every capacity of every case, with ONE exception: noise768's octave 1 has 5184 raw extrema (a second bit of the mask)
ALSO_OVERFLOWS = {("noise768", 4096): {1: {"inside blur 2"}}}
# the image that fits 4096 in both paths (the re-arm test runs it between two overflowing runs of syn512)
FITS = "sparse512"
# the host mirror's re-run loop from 4096: (image, capacities tried, oracle features)
RERUNS = [("syn512", (4096, 8192), 6301), ("noise512", (4096, 8192, 16384), 20037)]


def capacity_fits(name, cap):
    """the fused path at the defaults runs through at this capacity: stage-1 and stage-6 lists of every octave fit"""
    return all(c[5] <= cap for st in (1, 6) for c in counts(name, st))


# ---- hand-placed lists whose EXPANSION overflows (capacity 4096, sampling_cases' image, parameters and preconditions) --------------
PLACED_PAIR = "default"
PLACED_CUTS = {
    # name -> expanded records of (blur 1, blur 2 up to the straddling key point, more blur-2 key points, blur-3 key points)
    "mid_keypoint": "the cut falls behind the first orientation of a blur-2 key point; the blur-3 segment is dropped whole",
    "segment_start": "blur 1 and blur 2 expand to exactly 4096 records: the blur-3 segment starts on the cut",
    "blur1_only": "blur 1 alone expands past 4096: both later segments are dropped whole, idx = [0, 0, cap, cap, cap]",
}
_PLACED = {}


def _walk(cands, norient, target, exact):
    """key points (indices into the octave's list) taken cyclically from `cands` until they expand to `target` records (exact) or
    to at least `target` -> (indices, expanded records)"""
    out, total, k = [], 0, 0
    while (target - total > 12) if exact else (total < target):      # (a key point has at most four orientations)
        i = cands[k % len(cands)]
        out.append(i)
        total += int(norient[i])
        k += 1
    if exact:       # the rest in twos, one three where it is odd
        two = [i for i in cands if norient[i] == 2][0]
        three = [i for i in cands if norient[i] == 3][0]
        rest = target - total
        assert rest >= 2
        if rest % 2:
            out.append(three)
            rest -= 3
        out += [two] * (rest // 2)
        total = target
    return out, total


def placed_lists(name):
    """-> [(SSKEYPOINT[], idx[5]) per octave]: octave 0 built from sampling_cases' "place_default" placements that have at least two
    orientations (repeated: the list stays sorted by blur), a short octave-1 list that fits, octaves 2-3 empty"""
    if name in _PLACED:
        return _PLACED[name]
    base, ref = C.build_set("place_" + PLACED_PAIR), C.reference("place_" + PLACED_PAIR)
    kps, _ = base[0]
    norient = ref["norient"][0]
    cands = {b: [i for i in range(len(kps)) if kps["blur"][i] == b and norient[i] >= 2] for b in (1, 2, 3)}
    if name == "mid_keypoint":
        pick = _walk(cands[1], norient, 1000, True)[0] + _walk(cands[2], norient, 3095, True)[0] + cands[2][:5] + cands[3][:5]
    elif name == "segment_start":
        pick = _walk(cands[1], norient, 1000, True)[0] + _walk(cands[2], norient, 3096, True)[0] + cands[3][:10]
    else:
        pick = _walk(cands[1], norient, 4200, False)[0] + cands[2][:5] + cands[3][:5]
    lst0 = kps[np.array(pick)].copy()
    short, _ = base[1]
    lst1 = short[::8].copy()
    empty = np.zeros(0, H.SSKEYPOINT)
    _PLACED[name] = [(lst0, C.partition_by_blur(lst0)), (lst1, C.partition_by_blur(lst1)),
                     (empty, C.partition_by_blur(empty)), (empty.copy(), C.partition_by_blur(empty))]
    return _PLACED[name]


def placed_reference(name):
    """chain_reference of placed_lists(name) -> ([(expanded SSKEYPOINT[], idx[5]) per octave], [FEATURE[] per octave], norient of
    octave 0)"""
    def compute():
        ow, dw = C.PAIRS[PLACED_PAIR]
        geoms = [tuple(C.geometry(o)[:3]) for o in range(4)]
        r = C.chain_reference(C.placed_levels(), geoms, [l for l, _ in placed_lists(name)], C.PLACED_MAXO, C.PLACED_THR, ow, dw)
        return _pack(r) + (r["norient"][0],)
    packed = _cached("placed_" + name, compute)
    return _unpack(packed[:4]) + (packed[4],)
