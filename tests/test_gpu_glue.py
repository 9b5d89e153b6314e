"""The MatchSet glue on the GPU -- ssrlcv_hip_compact_matches[_async], _filter_matchset, _select_pair_bundles,
_keypoints_from_members, _matchset_from_matches, _dog_normalised_sub -- against the numpy restatement of their header contracts
(tests/glue_ref.py) on the cases of tests/glue_cases.py, which sit either side of the seams the kernels define: wave runs, blocks,
scan rounds, tiles handed out to a capped grid, launches per 64 images (tests/test_glue_cases.py proves that without a GPU).
Every comparison is exact: record bytes (padding included) and float bit patterns, nothing left out.  Every buffer the library
writes lies between two 0xA5 guards that must come back intact, the workspaces included (given at their exact size), and the
inputs must come back as they went in."""
import ctypes

import numpy as np
import pytest
import torch

import glue_cases as C
import glue_ref as R
import helpers as H

pytestmark = pytest.mark.gpu

u32, vp, sz, ci = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
GUARD = 256
KIND_ID = {"dmatch": 0, "pair": 1, "match": 2}        # SSRLCV_OUT_DMATCH, _UINT2_PAIR, _MATCH


class Guarded:
    """`nbytes` of device memory (holding `content`, or 0xA5) between two guards of 0xA5, 256-byte aligned"""

    def __init__(self, nbytes, content=None):
        self.n = int(nbytes)
        self.buf = torch.full((2 * GUARD + self.n,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        if content is not None:
            flat = np.array(content, copy=True).view(np.uint8).reshape(-1)
            assert flat.size == self.n, (flat.size, self.n)
            if self.n:
                self.buf[GUARD:GUARD + self.n] = torch.from_numpy(flat).cuda()

    @property
    def addr(self):
        return self.buf.data_ptr() + GUARD

    @property
    def ptr(self):
        return vp(self.addr)

    def guards_intact(self):
        """without copying what lies between them"""
        return bool((self.buf[:GUARD] == 0xA5).all().item() and (self.buf[GUARD + self.n:] == 0xA5).all().item())

    def host(self):
        """-> (the bytes between the guards, both guards intact)"""
        h = self.buf.cpu().numpy()
        return h[GUARD:GUARD + self.n], bool((h[:GUARD] == 0xA5).all() and (h[GUARD + self.n:] == 0xA5).all())


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.size == want.size, (what, got.size, want.size)
    ne = got != want
    assert not ne.any(), (what, "%d of %d bytes differ, first at byte %d: got %s want %s" % (
        int(ne.sum()), ne.size, int(np.argmax(ne)), got[ne][:8], want[ne][:8]))


def intact(g, content, what):
    body, guards = g.host()
    assert guards, (what, "bytes outside the buffer were written")
    same_bytes(body, content, what)


# ---- 1. ssrlcv_hip_compact_matches and _async
def compact(capi, kind, mode, matches_addr, n, ws, ws_bytes):
    """-> (status, count): the synchronous call's host count or the asynchronous call's device count (a guarded word)"""
    if mode == "sync":
        cnt = u32(0xDEADBEEF)
        rc = capi.LIB.ssrlcv_hip_compact_matches(ci(KIND_ID[kind]), vp(matches_addr), u32(n), ctypes.byref(cnt), ws.ptr, sz(ws_bytes),
                                                 capi.stream_ptr())
        torch.cuda.synchronize()
        return rc, cnt.value
    cnt = Guarded(4)
    rc = capi.LIB.ssrlcv_hip_compact_matches_async(ci(KIND_ID[kind]), vp(matches_addr), u32(n), cnt.ptr, ws.ptr, sz(ws_bytes),
                                                   capi.stream_ptr())
    torch.cuda.synchronize()
    word, guards = cnt.host()
    assert guards, "bytes around the device count were written"
    return rc, int(word.view("<u4")[0])


def check_compact(capi, kind, mode, raw, want, ws, ws_bytes, what):
    n, size = len(raw), R.SIZE[kind]
    g = Guarded(n * size, raw)
    rc, count = compact(capi, kind, mode, g.addr, n, ws, ws_bytes)
    assert rc == OK, (what, rc)
    assert count == len(want), (what, count, len(want))
    body, guards = g.host()
    assert guards, (what, "bytes outside the list were written")
    same_bytes(body[:count * size], want, (what, "survivors"))
    same_bytes(body[count * size:], raw[count:], (what, "the records behind the survivors are left as they were"))
    assert ws.guards_intact(), (what, "bytes outside the workspace were written")


@pytest.mark.parametrize("kind,mode", [("dmatch", "sync"), ("match", "sync"), ("pair", "sync"), ("dmatch", "async"), ("pair", "async")])
def test_compact_equals_the_reference_around_runs_and_blocks(capi, kind, mode):
    for n in C.COMPACT_SMALL:
        need = C.compact_workspace_bytes(n, kind)
        ws = Guarded(need)                                  # the exact size, reused dirty from pattern to pattern
        for pattern in C.PATTERNS:
            raw, want = C.compact_case(kind, n, pattern)
            check_compact(capi, kind, mode, raw, want, ws, need, (kind, mode, n, pattern))
        g = Guarded(n * R.SIZE[kind], raw)
        rc, _ = compact(capi, kind, mode, g.addr, n, ws, need - 1)
        assert rc == WORKSPACE, (kind, mode, n, rc)
        intact(g, raw, (kind, mode, n, "a refused call leaves the list alone"))


LARGE = [(kind, C.N_SCAN_ROUND2, p) for kind in ("dmatch", "match", "pair") for p in ("all", "p50")] + \
        [("pair", C.N_SCAN_1024, p) for p in ("all", "p50")]


@pytest.mark.parametrize("kind,n,pattern", LARGE)
def test_compact_equals_the_reference_past_a_scan_round_and_a_copy_sweep(capi, kind, n, pattern):
    """524 801 records: the 256-thread scan carries its sum into a second round; DMatch (all kept) and uint2_pair beyond 524 288
    survivors take a second sweep of the counted copy.  8 390 657 uint2_pairs: the 1024-thread scan."""
    raw, want = C.compact_case(kind, n, pattern)
    need = C.compact_workspace_bytes(n, kind)
    ws = Guarded(need)
    for mode in ("sync",) if kind == "match" else ("sync", "async"):
        check_compact(capi, kind, mode, raw, want, ws, need, (kind, mode, n, pattern))
    C.compact_case.cache_clear()


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_compact_in_a_workspace_that_served_a_larger_call(capi, mode):
    big = C.compact_workspace_bytes(C.BLOCK + 1, "dmatch")
    ws = Guarded(big)
    for kind, n, pattern in (("dmatch", C.BLOCK + 1, "p50"), ("dmatch", C.RUN + 1, "p50"), ("pair", C.WAVE + 1, "alternate"),
                             ("dmatch", C.BLOCK + 1, "p98"), ("pair", 1, "all"), ("dmatch", C.RUN, "runs")):
        raw, want = C.compact_case(kind, n, pattern)
        check_compact(capi, kind, mode, raw, want, ws, big, (kind, mode, n, pattern, "workspace reused"))


@pytest.mark.parametrize("kind,mode", [("dmatch", "sync"), ("match", "sync"), ("pair", "sync"), ("dmatch", "async"), ("pair", "async"),
                                       ("match", "async")])
def test_compact_of_an_empty_list(capi, kind, mode):
    """numMatches == 0: SSRLCV_OK and a count of 0 before anything else is looked at -- the workspace size, and for _async the
    kind and the alignment of the list -- and neither the list nor the workspace is touched"""
    ws = Guarded(64)
    g = Guarded(R.SIZE[kind] + 8, np.full(R.SIZE[kind] + 8, 0x11, np.uint8))
    for off, ws_bytes in ((0, 64), (8, 0)):
        rc, count = compact(capi, kind, mode, g.addr + off, 0, ws, ws_bytes)
        assert (rc, count) == (OK, 0), (kind, mode, off, rc, count)
    intact(g, np.full(g.n, 0x11, np.uint8), "the list")
    intact(ws, np.full(64, 0xA5, np.uint8), "the workspace")


def test_compact_async_refuses_what_its_copy_cannot_move(capi):
    """the 40-byte Match, and a list that begins 8 bytes off a 16-byte boundary: SSRLCV_ERR_UNSUPPORTED, nothing touched"""
    n = C.RUN + 1
    ws = Guarded(C.compact_workspace_bytes(n, "dmatch"))
    raw, _ = C.compact_case("match", n, "p50")
    g = Guarded(n * 40, raw)
    assert compact(capi, "match", "async", g.addr, n, ws, ws.n)[0] == UNSUPPORTED
    intact(g, raw, "Match through _async")
    for kind in ("pair", "dmatch"):
        raw, _ = C.compact_case(kind, n, "p50")
        g = Guarded(n * R.SIZE[kind] + 8, np.concatenate([np.full(8, 0x11, np.uint8), raw.reshape(-1)]))
        assert compact(capi, kind, "async", g.addr + 8, n, ws, ws.n)[0] == UNSUPPORTED, kind
        intact(g, np.concatenate([np.full(8, 0x11, np.uint8), raw.reshape(-1)]), (kind, "a list 8 bytes off"))
    # the synchronous call moves any list
    raw, want = C.compact_case("pair", n, "p50")
    g = Guarded(n * 16 + 8, np.concatenate([np.full(8, 0x11, np.uint8), raw.reshape(-1)]))
    rc, count = compact(capi, "pair", "sync", g.addr + 8, n, ws, ws.n)
    assert rc == OK and count == len(want)
    same_bytes(g.host()[0][8:8 + 16 * count], want, "a list 8 bytes off through the synchronous call")


# ---- 2. ssrlcv_hip_filter_matchset and ssrlcv_hip_select_pair_bundles
def filter_on_device(capi, b, kp, short=0):
    capi.LIB.ssrlcv_hip_filter_workspace_bytes.restype = ctypes.c_size_t
    need = int(capi.LIB.ssrlcv_hip_filter_workspace_bytes(u32(len(b))))
    io = dict(b=Guarded(12 * len(b), b), kp=Guarded(16 * len(kp), kp), mm=Guarded(8 * len(b)), out=Guarded(16 * len(kp)),
              counts=Guarded(12), ws=Guarded(need))
    rc = capi.LIB.ssrlcv_hip_filter_matchset(io["b"].ptr, io["kp"].ptr, u32(len(b)), io["mm"].ptr, io["out"].ptr, io["counts"].ptr,
                                             io["ws"].ptr, sz(need - short), capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, io


def check_filter(capi, n, pattern):
    b, kp = C.filter_case(n, pattern)
    mm_r, kp_r, cnt_r = R.filter_ref(b, kp)
    rc, io = filter_on_device(capi, b, kp)
    what = (n, pattern)
    assert rc == OK, (what, rc)
    host = {k: g.host() for k, g in io.items()}
    assert all(guards for _, guards in host.values()), (what, [k for k, (_, guards) in host.items() if not guards])
    cnt = host["counts"][0].view("<u4")
    assert np.array_equal(cnt, cnt_r), (what, cnt, cnt_r)
    same_bytes(host["mm"][0][:8 * cnt[0]], mm_r, (what, "MultiMatch"))
    same_bytes(host["out"][0][:16 * cnt[1]], kp_r, (what, "KeyPoint"))
    same_bytes(host["b"][0], b, (what, "the bundles are read only"))
    same_bytes(host["kp"][0], kp, (what, "the key points are read only"))


@pytest.mark.parametrize("n", C.TILE_SIZES[:-1])
def test_filter_equals_the_reference_around_a_tile(capi, n):
    for pattern in C.FILTER_PATTERNS:
        check_filter(capi, n, pattern)
    b, kp = C.filter_case(n, "mixed")
    rc, io = filter_on_device(capi, b, kp, short=1)
    assert rc == WORKSPACE
    for k in ("mm", "out", "counts", "ws"):
        intact(io[k], np.full(io[k].n, 0xA5, np.uint8), (n, k, "a refused call writes nothing"))


@pytest.mark.parametrize("pattern", ["mixed", "tiles"])
def test_filter_equals_the_reference_where_blocks_take_a_second_tile(capi, pattern):
    """2050 tiles on a grid of 2048 blocks: two blocks come back for a tile (svs::next_tile), and the counts are written by
    whichever block owns tile 2049, not by the last block.  config[4] runs this path with 3.1 M multi-matches."""
    check_filter(capi, C.TILE_SIZES[-1], pattern)


PAIRS = ((C.SELECT_A, C.SELECT_B), (C.SELECT_A, C.SELECT_A), (C.SELECT_B, C.SELECT_A))


def select_on_device(capi, mm, kp, a, b, short=0):
    capi.LIB.ssrlcv_hip_select_pair_workspace_bytes.restype = ctypes.c_size_t
    need = int(capi.LIB.ssrlcv_hip_select_pair_workspace_bytes(u32(len(mm))))
    io = dict(mm=Guarded(8 * len(mm), mm), kp=Guarded(16 * len(kp), kp), mmo=Guarded(8 * len(mm)), kpo=Guarded(32 * len(mm)),
              count=Guarded(4), ws=Guarded(need))
    rc = capi.LIB.ssrlcv_hip_select_pair_bundles(io["mm"].ptr, io["kp"].ptr, u32(len(mm)), u32(len(kp)), ci(a), ci(b), io["mmo"].ptr,
                                                 io["kpo"].ptr, io["count"].ptr, io["ws"].ptr, sz(need - short), capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, io


def check_select(capi, n, a, b):
    mm, kp = C.select_case(n)
    mm_r, kp_r = R.select_pair_ref(mm, kp, a, b)
    rc, io = select_on_device(capi, mm, kp, a, b)
    what = (n, a, b)
    assert rc == OK, (what, rc)
    host = {k: g.host() for k, g in io.items()}
    assert all(guards for _, guards in host.values()), (what, [k for k, (_, guards) in host.items() if not guards])
    count = int(host["count"][0].view("<u4")[0])
    assert count == len(mm_r), (what, count, len(mm_r))
    same_bytes(host["mmo"][0][:8 * count], mm_r, (what, "MultiMatch"))
    same_bytes(host["kpo"][0][:32 * count], kp_r, (what, "KeyPoint"))
    same_bytes(host["mm"][0], mm, (what, "the multi-matches are read only"))
    same_bytes(host["kp"][0], kp, (what, "the key points are read only"))


@pytest.mark.parametrize("n", C.TILE_SIZES[:-1])
def test_select_pair_equals_the_reference_around_a_tile(capi, n):
    for a, b in PAIRS:                                  # (a, b), imageA == imageB, and the pair the other way round
        check_select(capi, n, a, b)
    mm, kp = C.select_case(n)
    rc, io = select_on_device(capi, mm, kp, C.SELECT_A, C.SELECT_B, short=1)
    assert rc == WORKSPACE
    for k in ("mmo", "kpo", "count", "ws"):
        intact(io[k], np.full(io[k].n, 0xA5, np.uint8), (n, k, "a refused call writes nothing"))


def test_select_pair_equals_the_reference_where_blocks_take_a_second_tile(capi):
    check_select(capi, C.TILE_SIZES[-1], C.SELECT_A, C.SELECT_B)


# ---- 4. ssrlcv_hip_keypoints_from_members
def members_on_device(capi, mem, feats, out_addr, null_count=7):
    dev = [None if f is None else capi.to_dev(f) for f in feats]
    ptrs = (vp * len(feats))(*[0 if t is None else t.data_ptr() for t in dev])
    counts = (u32 * len(feats))(*[null_count if f is None else len(f) for f in feats])   # an image without an array: its count is not believed
    mem_d = Guarded(8 * len(mem), mem)
    rc = capi.LIB.ssrlcv_hip_keypoints_from_members(mem_d.ptr if len(mem) else vp(0), u32(len(mem)), ptrs, counts, u32(len(feats)),
                                                    vp(out_addr), capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, mem_d, dev


@pytest.mark.parametrize("num_images", C.MEMBER_IMAGES)
def test_keypoints_from_members_equal_the_reference(capi, num_images):
    """one launch per 64 images: 1, 1, 2 and 3 launches over the same member list, every element written by exactly one of them
    -- members that name no image by the first"""
    mem, feats, _ = C.members_case(num_images)
    want = R.members_ref(mem, [None if f is None else R.rows(f, 152) for f in feats], num_images)
    out = Guarded(16 * len(mem))
    rc, mem_d, _ = members_on_device(capi, mem, feats, out.addr)
    assert rc == OK
    body, guards = out.host()
    assert guards, "bytes outside keyPoints were written"
    same_bytes(body, want, (num_images, "KeyPoint, padding included"))
    intact(mem_d, mem, "the members are read only")


def test_keypoints_from_members_arguments(capi):
    mem, feats, _ = C.members_case(C.MAX_GATHER_IMAGES + 1)
    out = Guarded(16 * len(mem) + 8)
    rc, _, _ = members_on_device(capi, mem, feats, out.addr + 8)                  # 8 bytes off a 16-byte boundary
    assert rc == INVALID_ARG
    intact(out, np.full(out.n, 0xA5, np.uint8), "a refused call writes nothing")
    rc, _, _ = members_on_device(capi, mem[:0], feats, out.addr)                  # no members: nothing to do
    assert rc == OK
    intact(out, np.full(out.n, 0xA5, np.uint8), "numMembers 0 touches nothing")


# ---- 5. ssrlcv_hip_matchset_from_matches
@pytest.mark.parametrize("n", C.MATCHSET_SIZES)
@pytest.mark.parametrize("kind", ["dmatch", "match"])
def test_matchset_from_matches_equals_the_reference(capi, kind, n):
    for peak in C.PEAKS if kind == "dmatch" and n < (1 << 20) else C.PEAKS[1:2]:
        raw = C.matchset_records(kind, n, peak)
        kp_r, mm_r, top = R.matchset_ref(raw, kind)
        io = dict(m=Guarded(len(raw) * R.SIZE[kind], raw), kp=Guarded(32 * n), mm=Guarded(8 * n), top=Guarded(4))
        rc = capi.LIB.ssrlcv_hip_matchset_from_matches(ci(KIND_ID[kind]), io["m"].ptr, u32(n), io["kp"].ptr, io["mm"].ptr,
                                                       io["top"].ptr if kind == "dmatch" else vp(0), capi.stream_ptr())
        torch.cuda.synchronize()
        what = (kind, n, peak)
        assert rc == OK, (what, rc)
        host = {k: g.host() for k, g in io.items()}
        assert all(guards for _, guards in host.values()), (what, [k for k, (_, guards) in host.items() if not guards])
        same_bytes(host["kp"][0], kp_r, (what, "KeyPoint"))
        same_bytes(host["mm"][0], mm_r, (what, "MultiMatch"))
        same_bytes(host["m"][0], raw, (what, "the matches are read only"))
        if kind == "dmatch":
            got = host["top"][0].view("<u4")[0]
            assert got == np.float32(top).view(np.uint32), (what, host["top"][0].view("<f4")[0], top)
        else:
            same_bytes(host["top"][0], np.full(4, 0xA5, np.uint8), (what, "no maxDistance asked for"))


def test_matchset_from_matches_refuses_a_max_distance_of_match_records(capi):
    raw = C.matchset_records("match", 5, "first")
    io = dict(m=Guarded(200, raw), kp=Guarded(160), mm=Guarded(40), top=Guarded(4))
    rc = capi.LIB.ssrlcv_hip_matchset_from_matches(ci(KIND_ID["match"]), io["m"].ptr, u32(5), io["kp"].ptr, io["mm"].ptr, io["top"].ptr,
                                                   capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == INVALID_ARG
    for k in ("kp", "mm", "top"):
        intact(io[k], np.full(io[k].n, 0xA5, np.uint8), (k, "a refused call writes nothing"))


# ---- 6. ssrlcv_hip_dog_normalised_sub
FLT_MAX = np.float32(3.4028234663852886e38)


def dog_on_device(capi, lv, mmx, w, h, want_minmax=True):
    n = w * h
    lv_d = [Guarded(4 * n, lv[b]) for b in range(6)]
    dog_d = [Guarded(4 * n) for _ in range(5)]
    mmx_d = Guarded(48, mmx)
    dmm_d = Guarded(40, np.array([FLT_MAX, -FLT_MAX] * 5, np.float32))
    LV = (vp * 6)(*[g.addr for g in lv_d])
    DG = (vp * 5)(*[g.addr for g in dog_d])
    rc = capi.LIB.ssrlcv_hip_dog_normalised_sub(LV, mmx_d.ptr, u32(w), u32(h), DG, dmm_d.ptr if want_minmax else vp(0), capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, lv_d, dog_d, dmm_d


@pytest.mark.parametrize("w,h", C.DOG_SIZES)
def test_dog_levels_and_their_minmax_equal_the_reference(capi, w, h):
    """k_dog<false>, the materialising form with its min / max atomics: one lane, a part of a block, and more than 1024 blocks
    x 256 lanes x 4 pixels (the grid-stride loop)."""
    lv, mmx = C.dog_case(w, h)
    dog_r, dmm_r = R.dog_ref(lv, mmx)
    for want_minmax in (True, False):
        rc, lv_d, dog_d, dmm_d = dog_on_device(capi, lv, mmx, w, h, want_minmax)
        assert rc == OK
        for b in range(5):
            body, guards = dog_d[b].host()
            assert guards, (w, h, b, "bytes outside the DoG level were written")
            ne = body.view("<u4") != H.bits(dog_r[b])
            assert not ne.any(), (w, h, b, want_minmax, "%d of %d differ, first at %d: got %r want %r" % (
                int(ne.sum()), ne.size, int(np.argmax(ne)), body.view("<f4")[ne][:4], dog_r[b][ne][:4]))
        for b in range(6):
            intact(lv_d[b], lv[b], (w, h, b, "the levels are read only"))
        body, guards = dmm_d.host()
        assert guards
        if want_minmax:
            assert np.array_equal(body.view("<u4"), H.bits(dmm_r).reshape(-1)), (w, h, body.view("<f4"), dmm_r)
        else:
            same_bytes(body, np.array([FLT_MAX, -FLT_MAX] * 5, np.float32), "dogMinMax NULL: nothing accumulated")


def test_dog_refuses_a_pixel_count_that_is_no_multiple_of_four(capi):
    lv = np.ones((6, 9), np.float32)
    rc, _, dog_d, dmm_d = dog_on_device(capi, lv, np.array([[0, 2]] * 6, np.float32), 3, 3)
    assert rc == INVALID_ARG
    for g in dog_d:
        intact(g, np.full(g.n, 0xA5, np.uint8), "a refused call writes nothing")
