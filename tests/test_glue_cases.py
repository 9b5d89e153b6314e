"""The cases of tests/glue_cases.py test something, shown without a GPU: every named size lies on the side of its seam that it
claims (computed from the constants, and the constants are read back out of the kernels' sources), the patterns keep some
records and drop some, the tile-aligned filter case has tiles without a survivor, the select-pair case is refused for every
reason there is, the members case reaches every launch and every edge, and the plain references (tests/glue_ref.py) agree with
their own loop forms, with answers written out by hand and, for the filter, with the oracle.  tests/test_gpu_glue.py then holds
the kernels to the same references on the same cases."""
import ctypes
import os
import re

import numpy as np
import pytest

import glue_cases as C
import glue_ref as R
import helpers as H

CSRC = os.path.join(H.ROOT, "ssrlcv_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


@pytest.mark.parametrize("name,pattern,value", [
    ("compact.h", r"constexpr int kThreads = (\d+);", C.SVC_THREADS),
    ("compact.h", r"start \+= THREADS \* (\d+)\)", C.SCAN_ITEMS),
    ("compact.h", r"if \(!live && \(size_t\)NKEYS \* runs > (\d+)\)\s+hipLaunchKernelGGL\(\(k_scan<NKEYS, 1024>\)", C.SCAN_SWITCH),
    ("compact.h", r"else\s+hipLaunchKernelGGL\(\(k_scan<NKEYS, (\d+)>\), dim3\(1\), dim3\(256\)", 256),
    ("compact.h", r"const uint32_t base = run \* \((\d+)u \* PER_THREAD\);", C.WAVE),
    ("scan_lookback.h", r"constexpr int kThreads = (\d+);", C.SVS_THREADS),
    ("scan_lookback.h", r"at -= (\d+);", C.LOOKBACK_WINDOW),
    ("filter.hip", r"constexpr int kItems = (\d+);", C.K_ITEMS),
    ("filter.hip", r"constexpr int kChunk = (\d+);", C.K_CHUNK),
    ("scan_lookback.h", r"constexpr uint32_t kTile = kThreads \* ITEMS;", None),
    ("scan_lookback.h", r"constexpr uint32_t kMaxBlocks = (\d+);", C.GRID_CAP),
    ("matcher.hip", r"constexpr int kMaxGatherImages = (\d+);", C.MAX_GATHER_IMAGES),
    ("matcher.hip", r"blocks = blocks > (\d+)u \? 2048u : blocks;\s+hipLaunchKernelGGL\(k_copy_counted, dim3\(blocks\), dim3\(256\)", C.COPY_BLOCKS),
    ("matcher.hip", r"i \+= \(size_t\)gridDim\.x \* (\d+)\) dst\[i\] = src\[i\];", C.COPY_THREADS),
    ("matcher.hip", r"const uint32_t i = blockIdx\.x \* (\d+) \+ threadIdx\.x;\s+float d = 0\.0f;", C.MATCHSET_BLOCK),
    ("pyramid.hip", r"if \(blocks > (\d+)\) blocks = 1024;", C.DOG_BLOCKS),
    ("pyramid.hip", r"size_t stride = \(size_t\)gridDim\.x \* (\d+) \* 4;", C.DOG_THREADS),
])
def test_the_constants_are_the_sources(name, pattern, value):
    found = re.findall(pattern, source(name))
    assert found, (name, pattern)
    if value is not None:
        assert all(int(f) == value for f in found), (name, pattern, found, value)


def test_the_instantiations_are_the_sources():
    """partition<1, 8> at all five call sites of the two compactions, the one walk of the look-back kernels (its tile, its grid
    cap, its last-tile condition) with both filter kernels instantiating it at kItems, and the workspace formula the exact-size
    tests restate"""
    m = source("matcher.hip")
    body = m[m.index("int ssrlcv_hip_compact_matches("): m.index("int ssrlcv_hip_keypoints_from_members(")]
    assert len(re.findall(r"svc::partition<1, %d>\(numMatches" % C.PER_THREAD, body)) == 5 == len(re.findall(r"svc::partition<", body))
    assert len(re.findall(r"\(size_t\)numMatches \* elem \+ 256 \+ svc::workspace_words<1, %d>\(numMatches\) \* 4;" % C.PER_THREAD, body)) == 2
    assert "return (size_t)NKEYS * kWavesPerBlock * num_chunks(n, PER_THREAD) + NKEYS + 2;" in source("compact.h")
    h, f = source("scan_lookback.h"), source("filter.hip")
    # one walk: a tile of kThreads * ITEMS from `base` on, tiles handed out up to ts.numTiles, the last one's thread 0 reports
    assert len(re.findall(r"const uint32_t base = tile \* kTile \+ threadIdx\.x \* ITEMS;", h)) == 1
    assert len(re.findall(r"if \(tile == ts\.numTiles - 1 && threadIdx\.x == 0\)", h)) == 1
    assert len(re.findall(r"for \(uint32_t tile = next_tile\(ts\.counter\); tile < ts\.numTiles; tile = next_tile\(ts\.counter\)\)", h)) == 1
    # one launch: the grid cap, and the tile count the filters ask for is that of their kItems
    assert len(re.findall(r"dim3\(tiles < kMaxBlocks \? tiles : kMaxBlocks\), dim3\(kThreads\)", h)) == 1
    assert "inline uint32_t scan_tiles(uint32_t n) { return (n + kThreads * ITEMS - 1) / (kThreads * ITEMS); }" in h
    assert len(re.findall(r"svs::for_each_tile<3, kItems>\(", f)) == 1 == len(re.findall(r"svs::for_each_tile<1, kItems>\(", f))
    assert len(re.findall(r"svs::launch_tiles<3>\(k_filter_matchset, tiles,", f)) == 1 == len(re.findall(r"svs::launch_tiles<1>\(k_select_pair, tiles,", f))
    assert len(re.findall(r"const uint32_t tiles = svs::scan_tiles<kItems>\(", f)) == 2 and "next_tile" not in f and "hipLaunchKernelGGL(k_filter" not in f
    assert "for (uint32_t base = 0; base < numImages; base += (uint32_t)kMaxGatherImages)" in m


def test_compact_sizes_sit_beside_their_seams():
    assert C.RUN == 512 and C.BLOCK == 2048 and C.SCAN256_ROUND == 1024 and C.COPY_SWEEP == 524288
    for seam in (C.WAVE, C.RUN, C.BLOCK):
        assert {seam - 1, seam, seam + 1} <= set(C.COMPACT_SMALL)
    assert C.table_entries(C.BLOCK) == 4 and C.table_entries(C.BLOCK + 1) == 8
    # one round of the 256-thread scan up to 524 288 elements, two from there
    assert C.table_entries(C.N_SCAN_ROUND2 - C.RUN - 1) == C.SCAN256_ROUND < C.table_entries(C.N_SCAN_ROUND2) <= 2 * C.SCAN256_ROUND
    assert C.table_entries(C.N_SCAN_ROUND2) <= C.SCAN_SWITCH                     # ... and still the 256-thread scan
    assert C.table_entries(C.N_SCAN_1024 - C.BLOCK - 1) == C.SCAN_SWITCH < C.table_entries(C.N_SCAN_1024)
    # the counted copy: a second sweep of the grid needs more than 2048 x 256 16-byte words
    assert C.N_SCAN_ROUND2 * (R.SIZE["dmatch"] // 16) > C.COPY_SWEEP > C.N_SCAN_ROUND2 * (R.SIZE["pair"] // 16) // 2
    assert -(-C.COPY_SWEEP // 3) == 174763 and C.N_SCAN_ROUND2 > 174763
    assert int(C.keep_pattern(C.N_SCAN_1024, "p50").sum()) > C.COPY_SWEEP         # uint2_pair: the random pattern sweeps twice too
    assert C.N_SCAN_1024 * (R.SIZE["pair"] // 16) > C.COPY_SWEEP * 16            # all kept: seventeen sweeps


@pytest.mark.parametrize("n", C.COMPACT_SMALL + (C.N_SCAN_ROUND2,))
def test_every_nontrivial_pattern_keeps_some_and_drops_some(n):
    for name in C.PATTERNS:
        keep = C.keep_pattern(n, name)
        assert len(keep) == n
        if C.nontrivial(n, name):
            assert 0 < int(keep.sum()) < n, (n, name)
    if n > C.RUN:     # whole runs without a survivor, and the patterns differ
        runs = C.keep_pattern(n, "runs")
        per_run = np.add.reduceat(runs.astype(np.int64), np.arange(0, n, C.RUN))
        assert (per_run == 0).any() and (per_run == np.minimum(C.RUN, n - np.arange(0, n, C.RUN)))[0]


@pytest.mark.parametrize("kind", sorted(R.SIZE))
def test_compact_records_compact_to_their_pattern(kind):
    for n, name in ((C.BLOCK + 1, "p50"), (C.RUN + 1, "runs"), (C.WAVE, "alternate"), (C.RUN, "p98")):
        keep = C.keep_pattern(n, name)
        raw = C.compact_records(kind, keep)
        assert np.array_equal(R.kept_mask(raw, kind), keep)
        assert np.array_equal(R.compact_ref(raw, kind), R.compact_ref_loop(raw, kind))
        assert np.array_equal(R.compact_ref(raw, kind), raw[keep])
        if kind == "pair":   # kept pairs that share x, kept pairs that share y
            w = R.words(raw)[keep]
            assert ((w[:, 0] == w[:, 2]) & (w[:, 1] != w[:, 3])).sum() > 5 and ((w[:, 1] == w[:, 3]) & (w[:, 0] != w[:, 2])).sum() > 5
        else:
            assert set(raw[~keep, 0].tolist()) == set([1, 2, 255][:int((~keep).sum())])
            assert len(np.unique(raw[keep], axis=0)) == int(keep.sum())          # distinct records: the order is checked


def test_compact_ref_on_a_list_written_out_by_hand():
    m = np.zeros(10, H.MATCH)
    m["invalid"] = [0, 1, 0, 2, 255, 0, 0, 128, 0, 1]
    m["kp0_parent"] = np.arange(10)
    assert np.ascontiguousarray(R.compact_ref(m, "match")).view(H.MATCH)["kp0_parent"].reshape(-1).tolist() == [0, 2, 5, 6, 8]
    d = np.zeros(10, H.DMATCH)
    d["invalid"], d["distance"] = m["invalid"], np.arange(10)
    assert np.ascontiguousarray(R.compact_ref(d, "dmatch")).view(H.DMATCH)["distance"].reshape(-1).tolist() == [0, 2, 5, 6, 8]
    p = np.zeros(10, H.UINT2_PAIR)
    p["a"] = [[0, 0], [1, 7], [2, 9], [3, 3], [0, 0], [5, 6], [7, 7], [4, 4], [9, 1], [0, 1]]
    p["b"] = [[0, 0], [1, 8], [2, 9], [4, 3], [0, 1], [5, 6], [7, 7], [3, 3], [9, 1], [1, 0]]
    want = [1, 3, 4, 7, 9]   # (1,7)-(1,8) shares x, (3,3)-(4,3) shares y, (0,0)-(0,1), (4,4)-(3,3), (0,1)-(1,0)
    got = np.ascontiguousarray(R.compact_ref(p, "pair")).view(H.UINT2_PAIR).reshape(-1)
    assert np.array_equal(got, p[want]) and np.array_equal(R.compact_ref_loop(p, "pair"), R.compact_ref(p, "pair"))


def test_tile_sizes_sit_beside_their_seams():
    assert C.TILE == 1024
    assert [C.tiles_of(n) for n in C.TILE_SIZES] == [1, 1, 1, 2, 5, C.GRID_CAP + 2]
    assert C.tiles_of(C.TILE_SIZES[-1]) > C.GRID_CAP >= C.tiles_of(C.TILE_SIZES[-2])   # only there a block takes a second tile
    assert C.TILE_SIZES[-1] % C.TILE == 1                                               # ... and the last tile holds one element
    assert C.tiles_of(C.TILE_SIZES[-1]) > C.LOOKBACK_WINDOW


@pytest.mark.parametrize("n", C.TILE_SIZES[:-1])
def test_filter_cases_hold_what_they_claim(oracle_lib, n):
    for pattern in C.FILTER_PATTERNS:
        b, kp = C.filter_case(n, pattern)
        mm_r, kp_r, cnt = R.filter_ref(b, kp)
        mm_l, kp_l, cnt_l = R.filter_ref_loop(b, kp)
        assert np.array_equal(mm_r, mm_l) and np.array_equal(kp_r, kp_l) and np.array_equal(cnt, cnt_l)
        assert cnt[2] == len(kp) and len(mm_r) == cnt[0] and len(kp_r) == cnt[1]
        # the oracle's restatement of the host loop (it does not read `index` either)
        mm_o, kp_o, cnt_o = np.zeros(n, H.MULTIMATCH), np.zeros(max(len(kp), 1), H.KEYPOINT), np.zeros(3, np.uint32)
        oracle_lib.oracle_filter_matchset(ctypes.c_uint32(n), H.P(np.ascontiguousarray(b)), H.P(np.ascontiguousarray(kp) if len(kp) else np.zeros(1, H.KEYPOINT)),
                                          H.P(mm_o), H.P(kp_o), H.P(cnt_o))
        assert np.array_equal(cnt_o, cnt)
        assert np.array_equal(R.rows(mm_o[:cnt[0]], 8), mm_r) and np.array_equal(R.rows(kp_o[:cnt[1]], 16), kp_r)
        kept = b["invalid"] == 0
        if pattern == "all":
            assert kept.all()
        if pattern == "none":
            assert not kept.any() and cnt[0] == 0 and cnt[2] > 0
        if pattern == "mixed" and n >= C.TILE - 1:
            assert 0 < kept.sum() < n and {0, 1, 2, 3, 8} == set(b["numLines"][kept].tolist())
            assert {1, 2, 255} == set(b["invalid"][~kept].tolist())
            assert not np.array_equal(b["index"], np.cumsum(b["numLines"]) - b["numLines"])   # `index` is garbage
        if pattern == "tiles" and n > C.TILE:
            per_tile = np.add.reduceat(kept.astype(np.int64), np.arange(0, n, C.TILE))
            size = np.minimum(C.TILE, n - np.arange(0, n, C.TILE))
            lines = np.add.reduceat(b["numLines"].astype(np.int64), np.arange(0, n, C.TILE))
            assert ((per_tile == 0) & (lines > 0)).any() and (per_tile == size).any() and set(per_tile) <= {0} | set(size)


def test_the_large_filter_case_has_whole_tiles_of_each_kind():
    b, _ = C.filter_case(C.TILE_SIZES[-1], "tiles")
    kept = b["invalid"] == 0
    per_tile = np.add.reduceat(kept.astype(np.int64), np.arange(0, len(b), C.TILE))
    assert (per_tile[0::2][:-1] == C.TILE).all() and (per_tile[1::2] == 0).all() and len(per_tile) == C.GRID_CAP + 2


@pytest.mark.parametrize("n", C.TILE_SIZES[:-1])
def test_select_cases_hold_what_they_claim(n):
    mm, kp = C.select_case(n)
    for a, b in ((C.SELECT_A, C.SELECT_B), (C.SELECT_A, C.SELECT_A), (C.SELECT_B, C.SELECT_A)):
        mm_r, kp_r = R.select_pair_ref(mm, kp, a, b)
        mm_l, kp_l = R.select_pair_ref_loop(mm, kp, a, b)
        assert np.array_equal(mm_r, mm_l) and np.array_equal(kp_r, kp_l)
        why = R.select_pair_reasons(mm, kp, a, b)
        assert (why == 0).sum() == len(mm_r)
        if n >= C.TILE - 1:   # taken, and refused for every reason there is
            assert set(why.tolist()) == set(range(len(R.REASONS))), (a, b, np.bincount(why))
    assert set(mm["numKeyPoints"].tolist()) == ({1, 2, 3} if n > 1 else {2})
    if n >= C.TILE - 1:
        idx = mm["index"].astype(np.int64)
        assert (idx + 1 == len(kp)).any() and kp["parentId"][-1] == C.SELECT_A     # index + 1 == numKeyPoints, refused by the bound alone
        assert (idx == -2 ** 31).any() and (idx == 2 ** 31 - 1).any()
        two = idx[(mm["numKeyPoints"] == 2) & (idx >= 0)]
        assert len(np.unique(two)) < len(two)                                       # multi-matches that share key points
        taken = idx[R.select_pair_reasons(mm, kp, C.SELECT_A, C.SELECT_B) == 0]
        assert len(np.unique(taken)) < len(taken)                                   # ... and are both taken


@pytest.mark.parametrize("num_images", C.MEMBER_IMAGES)
def test_members_cases_hold_what_they_claim(num_images):
    mem, feats, edge = C.members_case(num_images)
    assert len(mem) > 256 and len(feats) == num_images
    assert all(f is None or 3 <= len(f) <= 40 for f in feats)
    named = mem[mem[:, 0] < num_images, 0]
    assert set(named.tolist()) == set(range(num_images))                          # every image, so the ends of every chunk of 64
    chunks = -(-num_images // C.MAX_GATHER_IMAGES)
    assert set((named // C.MAX_GATHER_IMAGES).tolist()) == set(range(chunks))
    assert chunks == {1: 1, 64: 1, 65: 2, 129: 3}[num_images]
    want = {-1, 0, 1} | ({2} if num_images > 1 else set())
    assert set(edge.tolist()) == want
    out = R.members_ref(mem, [None if f is None else R.rows(f, 152) for f in feats], num_images)
    kp = np.ascontiguousarray(out).view(H.KEYPOINT).reshape(-1)
    assert np.array_equal(kp["parentId"].view(np.uint32), mem[:, 0]) and (kp["pad"] == 0).all()
    assert (kp["loc"][edge >= 0] == 0).all() and (kp["loc"][edge < 0] > 0).all()
    i = int(np.flatnonzero(edge < 0)[0])
    assert np.array_equal(kp["loc"][i], feats[mem[i, 0]]["loc"][mem[i, 1]])


def test_matchset_records_put_the_peak_where_they_claim():
    for n in C.MATCHSET_SIZES[:3]:
        assert n % C.WAVE != 0 or n == C.MATCHSET_BLOCK
        for peak in C.PEAKS:
            raw = C.matchset_records("dmatch", n, peak)
            d = np.ascontiguousarray(raw[:, 40:44]).view("<f4").reshape(-1)
            kp, mm, top = R.matchset_ref(raw, "dmatch")
            assert (raw[:, 0] == 0).all() and len(kp) == 2 * n and len(mm) == n
            if peak == "nowhere":
                assert top == 0 and (d == 0).all()
            else:
                assert top == np.float32(50000.5) and int(np.argmax(d)) == (0 if peak == "first" else n - 1) and (np.sort(d)[-2] < 40000)
    assert R.matchset_ref(C.matchset_records("match", 5, "first"), "match")[2] is None
    assert C.MATCHSET_SIZES[-1] % C.MATCHSET_BLOCK == 3


def test_dog_and_cutoff_cases():
    for w, h in C.DOG_SIZES:
        assert (w * h) % 4 == 0
    lv, mmx = C.dog_case(36, 20)
    dog, dmm = R.dog_ref(lv, mmx)
    assert dog.shape == (5, 720) and dog.dtype == np.float32 and (dmm[:, 0] < 0).all() and (dmm[:, 1] > 0).all()
    x = ((lv[1].astype(np.float64) - mmx[1, 0]) / (float(mmx[1, 1]) - float(mmx[1, 0]))
         - (lv[0].astype(np.float64) - mmx[0, 0]) / (float(mmx[0, 1]) - float(mmx[0, 0])))
    assert np.abs(dog[0] - x).max() < 4e-7                                         # three float32 roundings of values in [0, 1]
    params = C.cutoff_params()
    assert len(params) == 24 == len(set(params))
    assert sorted({(n - n % j) // j for n, j in params}) == sorted(C.SAMPLE_COUNTS)
    assert all(n % j != 0 for n, j in params if j != 1) and {j for _, j in params} == {1, C.SAMPLE_JUMP}
