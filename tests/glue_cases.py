"""Seeded, deterministic inputs for the MatchSet glue (tests/test_gpu_glue.py runs them on the device against tests/glue_ref.py;
tests/test_glue_cases.py shows without a GPU that they sit where they claim).  Every size is derived from a named constant of
the code it crosses; tests/test_glue_cases.py reads the constants back out of the sources, so a retuned kernel fails there
first instead of leaving these sizes beside the seams."""
import functools

import numpy as np

import glue_ref as R
import helpers as H

WAVE = 64

# ---- csrc/compact.h, as csrc/matcher.hip instantiates it for ssrlcv_hip_compact_matches[_async]
SVC_THREADS = 256                      # svc::kThreads
PER_THREAD = 8                         # svc::partition<1, 8>
RUN = WAVE * PER_THREAD                # 512: the elements a wave owns (one entry of the count table)
BLOCK = SVC_THREADS * PER_THREAD       # 2048: the elements a block owns
SCAN_ITEMS = 4                         # k_scan: four consecutive table entries per thread and round
SCAN256_ROUND = 256 * SCAN_ITEMS       # 1024 entries per round of k_scan<1, 256>
SCAN_SWITCH = 16384                    # more table entries than this: k_scan<1, 1024>
COPY_BLOCKS, COPY_THREADS = 2048, 256  # k_copy_counted: grid cap x block, one 16-byte word per thread and sweep
COPY_SWEEP = COPY_BLOCKS * COPY_THREADS

# ---- csrc/scan_lookback.h, csrc/filter.hip
SVS_THREADS = 256                      # svs::kThreads
K_ITEMS = 4                            # filter.hip kItems
TILE = SVS_THREADS * K_ITEMS           # 1024 bundles / multi-matches per tile (scan_lookback.h for_each_tile<NSUM, kItems>)
GRID_CAP = 2048                        # scan_lookback.h kMaxBlocks: blocks of k_filter_matchset / k_select_pair at most
LOOKBACK_WINDOW = 64                   # aggregates one look-back step reads (tile_prefix: at -= 64); not forced, see DESIGN.md
K_CHUNK = 1024                         # filter.hip kChunk: samples per half of k_sample_cutoff's double buffer

# ---- csrc/matcher.hip
MAX_GATHER_IMAGES = 64                 # kMaxGatherImages: one launch of k_keypoints_from_members per 64 images
MATCHSET_BLOCK = 256                   # k_matchset: one thread per match

# ---- csrc/pyramid.hip, launch_dog without partials
DOG_BLOCKS, DOG_THREADS, DOG_PX = 1024, 256, 4


def table_entries(n):
    """entries of the partition's count table: four wave runs for every block, whole blocks"""
    return (SVC_THREADS // WAVE) * -(-n // BLOCK)


def compact_workspace_bytes(n, kind):
    """what ssrlcv_hip_compact_matches[_async] need: the scratch copy of the list, 256 bytes of slack for its alignment, the
    count table and NKEYS + 2 = 3 words of totals"""
    return n * R.SIZE[kind] + 256 + 4 * (table_entries(n) + 3)


COMPACT_SMALL = (1, WAVE - 1, WAVE, WAVE + 1, RUN - 1, RUN, RUN + 1, BLOCK - 1, BLOCK, BLOCK + 1)
N_SCAN_ROUND2 = SCAN256_ROUND * RUN + RUN + 1          # 524 288 + 513: 1028 entries, a second round of k_scan<1, 256>
N_SCAN_1024 = SCAN_SWITCH * RUN + BLOCK + 1            # 8 388 608 + 2049: 16 392 entries, k_scan<1, 1024>
assert COMPACT_SMALL == (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049)
assert (N_SCAN_ROUND2, N_SCAN_1024) == (524288 + 513, 8388608 + 2049)

PATTERNS = ("none", "all", "first", "last", "alternate", "runs", "p02", "p50", "p98")


def keep_pattern(n, name, seed=0):
    """-> bool [n]: which records are kept"""
    i = np.arange(n)
    if name == "none":
        return np.zeros(n, bool)
    if name == "all":
        return np.ones(n, bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == n - 1
    if name == "alternate":
        return i % 2 == 0
    if name == "runs":                 # whole runs of a wave kept and dropped in turn: every second table entry is 0
        return (i // RUN) % 2 == 0
    p = {"p02": 0.02, "p50": 0.5, "p98": 0.98}[name]
    rng = np.random.default_rng([n, int(p * 100), seed])
    keep = rng.random(n) < p
    if n >= 2 and keep.all():
        keep[int(rng.integers(n))] = False
    if n >= 2 and not keep.any():
        keep[int(rng.integers(n))] = True
    return keep


def nontrivial(n, name):
    """the (size, pattern) combinations that must keep some records and drop some"""
    if name in ("none", "all") or n < 2:
        return False
    return n > RUN if name == "runs" else True


INVALID_BYTES = np.array([1, 2, 255], np.uint8)


def compact_records(kind, keep, seed=0):
    """-> uint8 [n, size]: records of random bytes (so that order and content are both checked) that compact to `keep`.
    DMatch / Match: invalid byte 0 where kept and 1, 2 or 255 in turn where not; the padding bytes are zero, as every producer of
    the library leaves them.  uint2_pair: b = a where dropped; a kept pair has a.x == b.x with a.y != b.y, or a.y == b.y with
    a.x != b.x, or differs in both, in turn."""
    n, size = len(keep), R.SIZE[kind]
    rng = np.random.default_rng([n, size, seed])
    raw = rng.integers(0, 256, (n, size), dtype=np.uint8)
    if kind == "pair":
        w = raw.view("<u4")
        turn = np.arange(n) % 3
        w[:, 2] = np.where(turn == 0, w[:, 0], np.where(w[:, 2] == w[:, 0], w[:, 0] ^ 1, w[:, 2]))
        w[:, 3] = np.where(turn == 1, w[:, 1], np.where(w[:, 3] == w[:, 1], w[:, 1] ^ 1, w[:, 3]))
        w[~keep, 2:4] = w[~keep, 0:2]
        return raw
    raw[:, 1:8] = 0
    raw[:, 12:16] = 0
    raw[:, 28:32] = 0
    if kind == "dmatch":
        raw[:, 44:48] = 0
    raw[:, 0] = np.where(keep, 0, INVALID_BYTES[(np.cumsum(~keep) - 1) % 3])
    return raw


@functools.lru_cache(maxsize=1)
def compact_case(kind, n, pattern):
    """-> (records, the compacted records), left unchanged; only the last case is kept (the largest is 134 MB and its
    reference as much again: the test that builds it lets go of it with compact_case.cache_clear())"""
    raw = compact_records(kind, keep_pattern(n, pattern))
    raw.setflags(write=False)
    return raw, R.compact_ref(raw, kind)


# ---- ssrlcv_hip_matchset_from_matches
MATCHSET_SIZES = (MATCHSET_BLOCK - 1, MATCHSET_BLOCK, MATCHSET_BLOCK + 1, (1 << 20) + 3)
PEAKS = ("first", "last", "nowhere")


def matchset_records(kind, n, peak, seed=0):
    """valid records with random end points; DMatch distances below 40 000 but for the one maximum of 50 000.5 in the first
    lane of the first wave or in the last lane of the last (partial) wave, or all 0 ("nowhere": the result is 0)"""
    raw = compact_records(kind, np.ones(n, bool), seed + 1).copy()
    if kind == "dmatch":
        d = np.random.default_rng([n, seed]).integers(0, 40000, n).astype("<f4")
        if peak == "nowhere":
            d[:] = 0.0
        else:
            d[0 if peak == "first" else n - 1] = 50000.5
        raw[:, 40:44] = d.view(np.uint8).reshape(n, 4)
    return raw


# ---- ssrlcv_hip_filter_matchset, ssrlcv_hip_select_pair_bundles
TILE_SIZES = (1, TILE - 1, TILE, TILE + 1, 4 * TILE + 1, GRID_CAP * TILE + TILE + 1)
assert TILE_SIZES == (1, 1023, 1024, 1025, 4097, 2097152 + 1025)
FILTER_PATTERNS = ("mixed", "tiles", "all", "none")
LINES = np.array([0, 1, 2, 3, 8], np.uint32)
FLAGS = np.array([0, 0, 0, 1, 2, 255], np.uint8)


def tiles_of(n):
    return -(-n // TILE)


@functools.lru_cache(maxsize=2)
def filter_case(n, pattern):
    """-> (BUNDLE [n], KEYPOINT [sum of numLines]).  numLines from {0, 1, 2, 3, 8}; `index` and the padding are garbage (the
    contract reads neither); key points with random bits for locations (NaN patterns among them), zero padding.
    mixed: invalid bytes from {0, 1, 2, 255}, half of the bundles kept.  tiles: every second tile invalid as a whole, the
    others valid as a whole (an invalid tile adds 0 to the kept bundles and kept lines and its lines to the third sum)."""
    rng = np.random.default_rng([n, FILTER_PATTERNS.index(pattern)])
    b = np.zeros(n, H.BUNDLE)
    b["numLines"] = LINES[rng.integers(0, len(LINES), n)]
    b["index"] = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    b["pad"] = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    if pattern == "mixed":
        b["invalid"] = FLAGS[rng.integers(0, len(FLAGS), n)]
        if n >= TILE - 1:      # ... and a bundle without lines and one with a single line among the kept, whatever the draw
            b["numLines"][[5, n - 6]] = [0, 1]
            b["invalid"][[5, n - 6]] = 0
        elif n == 1:
            b["numLines"], b["invalid"] = 1, 0
    elif pattern == "tiles":
        b["invalid"] = INVALID_BYTES[np.arange(n) % 3] * ((np.arange(n) // TILE) % 2 == 1)
    elif pattern == "none":
        b["invalid"] = INVALID_BYTES[np.arange(n) % 3]
    nk = int(b["numLines"].sum())
    kp = np.zeros(nk, H.KEYPOINT)
    kp["parentId"] = rng.integers(0, 8, nk)
    kp["loc"] = rng.integers(0, 2 ** 32, (nk, 2), dtype=np.uint64).astype(np.uint32).view(np.float32)
    for a in (b, kp):
        a.setflags(write=False)
    return b, kp


SELECT_A, SELECT_B, SELECT_C = 3, 5, 6
# what a multi-match of the select-pair case is: its own key points' parentIds, then how its index is formed
SELECT_KINDS = (("ab", (SELECT_A, SELECT_B)), ("ba", (SELECT_B, SELECT_A)), ("aa", (SELECT_A, SELECT_A)), ("ac", (SELECT_A, SELECT_C)),
                ("one", (SELECT_A,)), ("three", (SELECT_A, SELECT_B, SELECT_C)), ("negative", (SELECT_A, SELECT_B)),
                ("past_the_end", ()), ("shared", ()))


@functools.lru_cache(maxsize=2)
def select_case(n):
    """-> (MULTIMATCH [n], KEYPOINT [nk]) for images (a, b, c) = (3, 5, 6).  Multi-matches of 1, 2 and 3 key points with
    parentIds (a, b), (b, a), (a, a), (a, c); indices that are negative (-1, -2, -3, INT_MIN); indices at and past the end
    (nk - 1 -- the last key point belongs to image a, so only the bound refuses it --, nk, nk + 7, INT_MAX); multi-matches
    that share the key points of another one (taken twice, or looking at the seam between two others)."""
    rng = np.random.default_rng([n, 77])
    kind = rng.integers(0, len(SELECT_KINDS), n)
    if n == 1:
        kind[:] = 0
    own = np.array([len(p) for _, p in SELECT_KINDS])[kind]
    start = np.cumsum(own) - own
    total = int(own.sum())
    nk = total + 1                                  # one more key point of image a, so that index nk - 1 begins with a
    kp = np.zeros(nk, H.KEYPOINT)
    kp["loc"] = rng.integers(0, 2 ** 32, (nk, 2), dtype=np.uint64).astype(np.uint32).view(np.float32)
    kp["parentId"][total] = SELECT_A
    for k, (_, parents) in enumerate(SELECT_KINDS):
        for j, p in enumerate(parents):
            kp["parentId"][start[kind == k] + j] = p
    mm = np.zeros(n, H.MULTIMATCH)
    mm["numKeyPoints"] = np.where(own == 0, 2, own)
    index = start.astype(np.int64)
    i = np.arange(n)
    names = [s for s, _ in SELECT_KINDS]
    neg = kind == names.index("negative")
    index[neg] = np.array([-1, -2, -3, -2 ** 31])[i[neg] % 4]
    end = kind == names.index("past_the_end")
    index[end] = np.array([nk - 1, nk, nk + 7, 2 ** 31 - 1])[i[end] % 4]
    sh = kind == names.index("shared")
    index[sh] = start[rng.integers(0, n, int(sh.sum()))] + (i[sh] % 5 == 0)   # another one's key points, or one further
    mm["index"] = index.astype(np.int32)
    for a in (mm, kp):
        a.setflags(write=False)
    return mm, kp


# ---- ssrlcv_hip_keypoints_from_members
MEMBER_IMAGES = (1, MAX_GATHER_IMAGES, MAX_GATHER_IMAGES + 1, 2 * MAX_GATHER_IMAGES + 1)
assert MEMBER_IMAGES == (1, 64, 65, 129)
EDGE_KINDS = ("no_image", "no_feature", "null_array")


@functools.lru_cache(maxsize=4)
def members_case(num_images):
    """-> (members uint32 [n, 2], feature arrays: FEATURE [3..40] per image or None, edge kind per member (-1: none)).
    At least 300 members (more than one block of 256), three and more per image, shuffled; image 1 has no array where there
    is more than one image; members that name no image (numImages, numImages + 5, numImages + 64, UINT32_MAX), no feature
    (count, count + 1, UINT32_MAX) or the image without an array."""
    rng = np.random.default_rng([num_images, 5])
    feats = []
    for v in range(num_images):
        f = np.zeros(int(rng.integers(3, 41)), H.FEATURE)
        f["loc"] = rng.uniform(0, 4096, (len(f), 2)).astype(np.float32)
        f["values"] = rng.integers(0, 256, (len(f), 128), dtype=np.uint8)
        f["parent"], f["pad"], f["sigma"], f["theta"] = v, 0x5A5A5A5A, 1.5, 0.25
        feats.append(f)
    null = 1 if num_images > 1 else None
    per = max(3, -(-300 // num_images))
    mem, edge = [], []
    for v in range(num_images):
        n = len(feats[v])
        for y in [0, n - 1] + [int(t) for t in rng.integers(0, n, per - 2)]:
            mem.append((v, y))
            edge.append(EDGE_KINDS.index("null_array") if v == null else -1)
        for y in (n, n + 1, 0xFFFFFFFF):
            mem.append((v, y))
            edge.append(EDGE_KINDS.index("null_array") if v == null else EDGE_KINDS.index("no_feature"))
    for x in (num_images, num_images + 5, num_images + MAX_GATHER_IMAGES, 0xFFFFFFFF):
        for y in (0, 2, 0xFFFFFFFF):
            mem.append((x, y))
            edge.append(EDGE_KINDS.index("no_image"))
    order = rng.permutation(len(mem))
    members = np.array(mem, np.uint32)[order]
    if null is not None:
        feats[null] = None
    members.setflags(write=False)
    return members, feats, np.array(edge)[order]


# ---- ssrlcv_hip_dog_normalised_sub
DOG_SIZES = ((2, 2), (36, 20), (1032, 1020))
assert DOG_SIZES[2][0] * DOG_SIZES[2][1] > DOG_BLOCKS * DOG_THREADS * DOG_PX     # the grid-stride loop takes a second step


@functools.lru_cache(maxsize=1)
def dog_case(w, h):
    """-> (six float32 levels [6, w h] with ranges like blurred grey levels, their true {min, max} [6, 2])"""
    rng = np.random.default_rng([w, h])
    lv = np.stack([rng.uniform(3.0 + b, 250.0 - 7.0 * b, w * h).astype(np.float32) for b in range(6)])
    mmx = np.stack([lv.min(1), lv.max(1)], 1).astype(np.float32)
    lv.setflags(write=False)
    return lv, mmx


# ---- ssrlcv_hip_error_sample_cutoff: sample counts either side of the float4 body / scalar tail and of the chunks
SAMPLE_COUNTS = (1, 2, 3, 4, 5, K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 2 * K_CHUNK - 1, 2 * K_CHUNK, 2 * K_CHUNK + 1, 3 * K_CHUNK + 3)
assert SAMPLE_COUNTS == (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 3075)
SAMPLE_JUMP = 7


def cutoff_params():
    """(numErrors, jump): every sample count at jump 1 and at jump 7 with numErrors % 7 != 0"""
    return [(s, 1) for s in SAMPLE_COUNTS] + [(SAMPLE_JUMP * s + 1 + s % (SAMPLE_JUMP - 1), SAMPLE_JUMP) for s in SAMPLE_COUNTS]
