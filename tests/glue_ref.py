"""Plain numpy restatements of the header contracts of the MatchSet glue (include/ssrlcv_hip.h: ssrlcv_hip_compact_matches[_async],
_matchset_from_matches, _keypoints_from_members, _filter_matchset, _select_pair_bundles, _dog_normalised_sub), written from the
header's sentences and not from the kernels: Python loops where the input is small, cumsum / repeat where it has millions of
records (tests/test_glue_cases.py holds the two forms of the filter to each other and to the oracle).  Nothing here calls the
library or the oracle.

Records travel as the bytes they are: a structured array or a uint8 array of `n x size` bytes goes in, uint8 [n, size] comes
out, padding included, so that a comparison of the bytes is a comparison of everything."""
import numpy as np

SIZE = {"dmatch": 48, "match": 40, "pair": 16}
KEYPOINT_BYTES, MULTIMATCH_BYTES, BUNDLE_BYTES, FEATURE_BYTES = 16, 8, 12, 152


def rows(records, size):
    """the records as uint8 [n, size]"""
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
    assert raw.size % size == 0, (raw.size, size)
    return raw.reshape(-1, size)


def words(raw):
    """uint8 [n, 4 k] -> the little-endian uint32 words [n, k]"""
    return np.ascontiguousarray(raw).view("<u4").reshape(len(raw), -1)


# ---- ssrlcv_hip_compact_matches[_async]
def kept_mask(records, kind):
    """A DMatch or Match is kept iff its `invalid` byte (byte 0) is 0: any non-zero byte is invalid, 2 and 255 included.  A
    uint2_pair is kept iff not (a.x == b.x and a.y == b.y)."""
    raw = rows(records, SIZE[kind])
    if kind == "pair":
        w = words(raw)
        return ~((w[:, 0] == w[:, 2]) & (w[:, 1] == w[:, 3]))
    return raw[:, 0] == 0


def compact_ref(records, kind):
    """-> the kept records in input order, uint8 [count, size]"""
    raw = rows(records, SIZE[kind])
    keep = kept_mask(raw, kind)
    out = np.zeros((int(keep.sum()), SIZE[kind]), np.uint8)
    at = np.cumsum(keep) - keep            # the slot of every kept record: how many were kept before it
    out[at[keep]] = raw[keep]
    return out


def compact_ref_loop(records, kind):
    """the same, one record at a time"""
    raw = rows(records, SIZE[kind])
    out = []
    for r in raw:
        if kind == "pair":
            a_x, a_y, b_x, b_y = [int(v) for v in r.view("<u4")]
            if a_x == b_x and a_y == b_y:
                continue
        elif r[0] != 0:
            continue
        out.append(r)
    return np.array(out, np.uint8).reshape(-1, SIZE[kind])


# ---- ssrlcv_hip_matchset_from_matches
def matchset_ref(records, kind):
    """keyPoints[2 i], [2 i + 1] = the end points of match i (bytes 8..23 and 24..39 of the record, as they lie there),
    multiMatches[i] = {2, 2 i}; max(0, max_i distance_i) for DMatch input (None for Match).
    -> (uint8 [2 n, 16], uint8 [n, 8], float32 or None)"""
    raw = rows(records, SIZE[kind])
    n = len(raw)
    kp = np.zeros((2 * n, KEYPOINT_BYTES), np.uint8)
    kp[0::2] = raw[:, 8:24]
    kp[1::2] = raw[:, 24:40]
    mm = np.zeros((n, 2), "<u4")
    mm[:, 0] = 2
    mm[:, 1] = 2 * np.arange(n)
    peak = None
    if kind == "dmatch":
        peak = np.float32(0.0)
        if n:
            peak = max(peak, np.ascontiguousarray(raw[:, 40:44]).view("<f4").max())
    return kp, mm.view(np.uint8).reshape(n, MULTIMATCH_BYTES), peak


# ---- ssrlcv_hip_keypoints_from_members
def members_ref(members, feature_arrays, num_images):
    """KeyPoint{parentId = image, 4 zero bytes, loc = that feature's location} for every member {image, feature}.  A member
    that names no image (x >= num_images), no feature of its image (y >= that image's count) or an image without an array
    (None) keeps its parentId and gets the location (0, 0).  feature_arrays: per image None or uint8 [count, 152].
    -> uint8 [n, 16]"""
    mem = np.ascontiguousarray(members).view("<u4").reshape(-1, 2)
    out = np.zeros((len(mem), 4), "<u4")
    for i, (x, y) in enumerate(mem.tolist()):
        out[i, 0] = x
        if x < num_images and feature_arrays[x] is not None and y < len(feature_arrays[x]):
            out[i, 2:4] = rows(feature_arrays[x], FEATURE_BYTES)[y, 8:16].view("<u4")   # Feature::loc sits at byte 8
    return out.view(np.uint8).reshape(len(mem), KEYPOINT_BYTES)


# ---- ssrlcv_hip_filter_matchset
def _bundle_fields(bundles):
    raw = rows(bundles, BUNDLE_BYTES)
    return np.ascontiguousarray(raw[:, 0:4]).view("<u4").reshape(-1).astype(np.int64), raw[:, 8] == 0


def filter_ref(bundles, kp):
    """The MatchSet without the bundles whose `invalid` byte is non-zero, order kept: matchesOut[j] = {numLines, running
    index}, keyPointsOut = the kept bundles' key points; the source offset of a bundle's key points is the running sum of ALL
    bundles' numLines (the bundles' own `index` is not read).  -> (uint8 [kept, 8], uint8 [kept lines, 16], uint32 [3] =
    {bundles kept, key points kept, key points in})"""
    lines, keep = _bundle_fields(bundles)
    kpr = rows(kp, KEYPOINT_BYTES)
    src = np.cumsum(lines) - lines                 # where each bundle's key points begin in the input
    lk = lines[keep]                               # numLines of the kept bundles
    dst = np.cumsum(lk) - lk                       # ... and where they begin in the output
    total = int(lk.sum())
    take = np.repeat(src[keep], lk) + (np.arange(total) - np.repeat(dst, lk))
    mm = np.zeros((len(lk), 2), "<u4")
    mm[:, 0] = lk
    mm[:, 1] = dst
    counts = np.array([len(lk), total, int(lines.sum())], np.uint32)
    return mm.view(np.uint8).reshape(len(lk), MULTIMATCH_BYTES), kpr[take], counts


def filter_ref_loop(bundles, kp):
    """the same as the host loop the header cites (src/PointCloudFactory.cu:3253-3268), one bundle at a time"""
    lines, keep = _bundle_fields(bundles)
    kpr = rows(kp, KEYPOINT_BYTES)
    mm, out, k_keypnt = [], [], 0
    for n, ok in zip(lines.tolist(), keep.tolist()):
        if ok:
            mm.append((n, len(out)))
            out.extend(kpr[k_keypnt + l] for l in range(n))
        k_keypnt += n
    counts = np.array([len(mm), len(out), k_keypnt], np.uint32)
    return (np.array(mm, "<u4").reshape(-1, 2).view(np.uint8).reshape(len(mm), MULTIMATCH_BYTES),
            np.array(out, np.uint8).reshape(-1, KEYPOINT_BYTES), counts)


# ---- ssrlcv_hip_select_pair_bundles
REASONS = ("taken", "not_two", "negative_index", "past_the_end", "wrong_first", "wrong_second")


def select_pair_reasons(mm, kp, a, b):
    """why each multi-match is taken or not, as indices into REASONS (the first test that fails, in the header's order: two key
    points; an index that names two key points of the array; parentIds a then b)"""
    m = np.ascontiguousarray(rows(mm, MULTIMATCH_BYTES))
    num = m[:, 0:4].copy().view("<u4").reshape(-1).astype(np.int64)
    idx = m[:, 4:8].copy().view("<i4").reshape(-1).astype(np.int64)
    parent = np.ascontiguousarray(rows(kp, KEYPOINT_BYTES)[:, 0:4]).view("<i4").reshape(-1)
    nk = len(parent)
    why = np.zeros(len(num), np.int64)
    inside = (idx >= 0) & (idx + 1 < nk)
    safe = np.where(inside, idx, 0)
    first = parent[safe] if nk else np.zeros(len(num), np.int32)
    second = parent[np.minimum(safe + 1, max(nk - 1, 0))] if nk else np.zeros(len(num), np.int32)
    why[:] = REASONS.index("taken")
    # later assignments win: the first failing test is assigned last
    why[second != b] = REASONS.index("wrong_second")
    why[first != a] = REASONS.index("wrong_first")
    why[idx + 1 >= nk] = REASONS.index("past_the_end")
    why[idx < 0] = REASONS.index("negative_index")
    why[num != 2] = REASONS.index("not_two")
    return why


def select_pair_ref(mm, kp, a, b):
    """A multi-match is taken when numKeyPoints == 2, its index names two key points of the array (0 <= index and
    index + 1 < numKeyPoints of the array) and their parentIds are a, b in that order; output j = {2, 2 j} with the pair
    re-labelled parentId 0 / 1, everything else of the two key points as it was.  -> (uint8 [count, 8], uint8 [2 count, 16])"""
    taken = np.flatnonzero(select_pair_reasons(mm, kp, a, b) == 0)
    idx = np.ascontiguousarray(rows(mm, MULTIMATCH_BYTES)[:, 4:8]).view("<i4").reshape(-1).astype(np.int64)[taken]
    kpr = rows(kp, KEYPOINT_BYTES)
    out = np.zeros((2 * len(taken), KEYPOINT_BYTES), np.uint8)
    if len(taken):
        out[0::2] = kpr[idx]
        out[1::2] = kpr[idx + 1]
        out[0::2, 0:4] = np.array([0], "<i4").view(np.uint8)
        out[1::2, 0:4] = np.array([1], "<i4").view(np.uint8)
    m = np.zeros((len(taken), 2), "<u4")
    m[:, 0] = 2
    m[:, 1] = 2 * np.arange(len(taken))
    return m.view(np.uint8).reshape(len(taken), MULTIMATCH_BYTES), out


def select_pair_ref_loop(mm, kp, a, b):
    """the same, one multi-match at a time"""
    m = words(rows(mm, MULTIMATCH_BYTES))
    kpr = rows(kp, KEYPOINT_BYTES)
    parent = [int(v) for v in np.ascontiguousarray(kpr[:, 0:4]).view("<i4").reshape(-1)]
    mm_out, kp_out = [], []
    for num, index in m.tolist():
        index = index - (1 << 32) if index >= (1 << 31) else index
        if num != 2 or index < 0 or index + 1 >= len(parent):
            continue
        if parent[index] != a or parent[index + 1] != b:
            continue
        mm_out.append((2, len(kp_out)))
        for label, k in ((0, kpr[index]), (1, kpr[index + 1])):
            k = k.copy()
            k[0:4] = np.array([label], "<i4").view(np.uint8)
            kp_out.append(k)
    return (np.array(mm_out, "<u4").reshape(-1, 2).view(np.uint8).reshape(len(mm_out), MULTIMATCH_BYTES),
            np.array(kp_out, np.uint8).reshape(-1, KEYPOINT_BYTES))


# ---- ssrlcv_hip_dog_normalised_sub
def dog_ref(levels, level_minmax):
    """dog[b] = N(level[b + 1]) - N(level[b]), b = 0 .. 4, with N(x) = (x - min_b) / (max_b - min_b): every operation one
    float32 operation, in that order.  -> (float32 [5, n], float32 [5, 2] = the {min, max} of each DoG level)"""
    lv = np.ascontiguousarray(levels, np.float32)
    mmx = np.ascontiguousarray(level_minmax, np.float32).reshape(6, 2)
    norm = np.zeros_like(lv)
    for b in range(6):
        mn, mx = mmx[b]
        norm[b] = (lv[b] - mn) / np.float32(mx - mn)
    dog = np.zeros((5, lv.shape[1]), np.float32)
    for b in range(5):
        dog[b] = norm[b + 1] - norm[b]
    assert norm.dtype == np.float32 and dog.dtype == np.float32
    return dog, np.stack([dog.min(1), dog.max(1)], 1).astype(np.float32)
