"""The device merge (csrc/merge.hip, ssrlcv_hip_merge_matches) against the plain Python reference of tests/merge_ref.py --
not against the host walk, whose walk() / for_each_cleared() / commit() are the device's text -- on the cases of
tests/merge_cases.py: tracks that make walks of up to 29 hops, every grid shape of the persistent kernel, every
configuration of four small models packed into one call, conflict chains on either side of the round limit and in the
single-thread tail, hand-made orderings.  Every comparison is exact.  Every call goes through the raw entry point with the
outputs prefilled, so each case also shows that nothing is written past numMatches records and numMembers members."""
import ctypes

import numpy as np
import pytest
import torch

import merge_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64           # records beyond the capacity the header asks for (totalPairs MultiMatch, 2 x totalPairs members)
MAX_ROUNDS = 48      # kMaxRounds of csrc/merge.hip: a seed image takes at most that many rounds, then the in-order tail
INVALID_ARG = -1     # SSRLCV_ERR_INVALID_ARG


def workspace_bytes(capi, nf, total):
    capi.LIB.ssrlcv_hip_merge_workspace_bytes.restype = ctypes.c_size_t
    arr = (ctypes.c_uint32 * len(nf))(*nf)
    return int(capi.LIB.ssrlcv_hip_merge_workspace_bytes(ctypes.c_uint32(len(nf)), arr, ctypes.c_uint32(total)))


class RawCall:
    """One ssrlcv_hip_merge_matches on the current stream, outputs and counts prefilled; nothing is read back before
    result()."""

    def __init__(self, capi, nf, blocks, workspace=None):
        counts = [len(b) for b in blocks]
        self.total = total = int(sum(counts))
        allp = np.concatenate(blocks) if total else np.zeros(0, C.PAIR)
        self.pairs_d = capi.to_dev(allp) if total else torch.zeros(16, dtype=torch.uint8, device="cuda")
        need = workspace_bytes(capi, nf, total)
        self.workspace = workspace if workspace is not None and workspace.numel() >= max(need, 1) else capi.dev_bytes(max(need, 256))
        self.mm_d = torch.full((8 * (total + GUARD),), SENTINEL, dtype=torch.uint8, device="cuda")
        self.mem_d = torch.full((8 * (2 * total + GUARD),), SENTINEL, dtype=torch.uint8, device="cuda")
        self.counts_d = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.launch = lambda: capi.LIB.ssrlcv_hip_merge_matches(
            ctypes.c_uint32(len(nf)), (ctypes.c_uint32 * len(nf))(*nf), ctypes.c_uint32(len(counts)),
            (ctypes.c_uint32 * max(len(counts), 1))(*counts), capi.ptr(self.pairs_d), capi.ptr(self.workspace),
            ctypes.c_size_t(self.workspace.numel()), capi.ptr(self.mm_d), capi.ptr(self.mem_d), capi.ptr(self.counts_d), capi.stream_ptr())

    def result(self):
        """-> (mm [n, 2], members [m, 2], counts[4]) after the bytes past the counts were found untouched"""
        counts = [int(x) & 0xffffffff for x in self.counts_d.cpu().tolist()]
        mm_b, mem_b = self.mm_d.cpu().numpy(), self.mem_d.cpu().numpy()
        n_mm, n_mem = (counts[0], counts[1]) if counts[0] != 0xffffffff else (0, 0)
        assert n_mm <= self.total and n_mem <= 2 * self.total, counts
        assert (mm_b[8 * n_mm:] == SENTINEL).all(), "MultiMatch records written past numMatches"
        assert (mem_b[8 * n_mem:] == SENTINEL).all(), "members written past numMembers"
        return mm_b[: 8 * n_mm].view("<u4").reshape(-1, 2), mem_b[: 8 * n_mem].view("<u4").reshape(-1, 2), counts


def assert_is_reference(name, got):
    mm, mem, counts = got
    mm_r, mem_r, stats = C.reference(name)
    assert counts[2] == 0, counts
    assert counts[0] == len(mm_r) and counts[1] == len(mem_r), (name, counts, len(mm_r), len(mem_r))
    assert np.array_equal(mm, mm_r), (name, np.nonzero((mm != mm_r).any(1))[0][:5])
    assert np.array_equal(mem, mem_r), (name, np.nonzero((mem != mem_r).any(1))[0][:5])
    # rounds: an image with a live seed takes at least one, none more than the limit
    assert stats["live_images"] <= counts[3] <= MAX_ROUNDS * max(len(C.case(name)[0]) - 2, 0), (name, counts[3])


@pytest.mark.parametrize("name", C.DEVICE_CASES)
def test_device_merge_equals_the_plain_reference(capi, name):
    nf, blocks = C.case(name)
    call = RawCall(capi, nf, blocks)
    assert call.launch() == 0
    got = call.result()
    print("%s: %d multi-matches, %d members, %d rounds" % (name, got[2][0], got[2][1], got[2][3]))
    assert_is_reference(name, got)
    if name in C.TAIL_ROUNDS:  # the chain outlasts the rounds: the rest was walked in order by one thread
        assert got[2][3] >= C.TAIL_ROUNDS[name], got[2]


def test_through_the_python_wrapper(capi):
    """capi.merge_matches_device (what the flow calls) slices the same arrays"""
    name = "tracks_v5_mixed"
    nf, blocks = C.case(name)
    mm_r, mem_r, _ = C.reference(name)
    mm_d, mem_d, n_mm, n_mem, rounds, _ = capi.merge_matches_device(nf, [len(b) for b in blocks], capi.to_dev(np.concatenate(blocks)))
    assert (n_mm, n_mem) == (len(mm_r), len(mem_r)) and rounds >= 3
    assert np.array_equal(mm_d.cpu().numpy().view("<u4").reshape(-1, 2), mm_r)
    assert np.array_equal(mem_d.cpu().numpy().view("<u4").reshape(-1, 2), mem_r)


REUSE = ("small_model_2221_packed", "grid_70000", "tracks_v32_mixed", "tracks_v8_mixed", "tail_mixed", "chain_49",
         "hand_empty_image_in_the_middle", "grid_1")


def test_one_workspace_through_calls_of_every_size(capi):
    """as pipeline.build_match_set keeps its workspace: largest problem first, down, and up again -- what a call left in
    the workspace (marks, barrier counters, scan descriptors, unresolved counts) must not reach the next"""
    sizes = {n: workspace_bytes(capi, C.case(n)[0], sum(len(b) for b in C.case(n)[1])) for n in REUSE}
    order = sorted(REUSE, key=lambda n: -sizes[n])
    assert order[0] == "small_model_2221_packed" and sizes[order[-1]] < sizes[order[0]] // 100
    ws = capi.dev_bytes(sizes[order[0]])
    for name in order + order[::-1]:
        call = RawCall(capi, *C.case(name), workspace=ws)
        assert call.workspace is ws and call.launch() == 0
        assert_is_reference(name, call.result())


def test_two_calls_back_to_back_on_a_side_stream(capi):
    """nothing between them but the stream's order: the second call's memsets and kernels must wait for the first's
    persistent kernel, sharing one workspace"""
    names = ("tracks_v6_collide", "tail_two_images")
    ws = capi.dev_bytes(max(workspace_bytes(capi, C.case(n)[0], sum(len(b) for b in C.case(n)[1])) for n in names))
    side = torch.cuda.Stream()
    calls = [RawCall(capi, *C.case(n), workspace=ws) for n in names]
    torch.cuda.synchronize()  # inputs and prefilled outputs are in place
    with torch.cuda.stream(side):
        rcs = [c.launch() for c in calls]
    side.synchronize()
    assert rcs == [0, 0]
    for n, c in zip(names, calls):
        assert_is_reference(n, c.result())


def _one(a, b):
    blk = np.zeros(1, C.PAIR)
    blk["a"][0], blk["b"][0] = a, b
    return blk


def _malformed():
    good = C.case("hand_reads_what_a_lower_seed_clears")  # [2, 2, 2]: valid entries around the bad one
    nf, blocks = good
    dup = _one((0, 1), (1, 1))  # (0,1) is matched into image 1 already
    return [
        ("a.x is the last image", nf, [blocks[0], blocks[1], np.concatenate([blocks[2], _one((2, 0), (2, 1))])], 1),
        ("a.x past the images", nf, [np.concatenate([_one((7, 0), (8, 0)), blocks[0]]), blocks[1], blocks[2]], 1),
        ("b.x equals a.x", nf, [blocks[0], blocks[1], np.concatenate([blocks[2], _one((1, 1), (1, 0))])], 1),
        ("b.x below a.x", nf, [blocks[0], blocks[1], np.concatenate([blocks[2], _one((1, 1), (0, 0))])], 1),
        ("a.y past its feature array", nf, [np.concatenate([blocks[0], _one((0, 2), (1, 0))]), blocks[1], blocks[2]], 1),
        ("b.y past its feature array", nf, [blocks[0], np.concatenate([blocks[1], _one((0, 0), (2, 2))]), blocks[2]], 1),
        ("b.y far past its feature array", [10, 10, 10], [_one((0, 5), (1, 0xfffffff0)), np.zeros(0, C.PAIR), np.zeros(0, C.PAIR)], 1),
        ("a query twice in one pair", nf, [np.concatenate([blocks[0], dup]), blocks[1], blocks[2]], 2),
        ("an entry out of range and a query twice", nf, [np.concatenate([blocks[0], dup]), blocks[1], np.concatenate([blocks[2], _one((1, 0), (2, 9))])], 3),
    ] + [(n,) + C.case(n) + (2,) for n in C.HOST_ONLY]


@pytest.mark.parametrize("what,nf,blocks,status", _malformed(), ids=[m[0].replace(" ", "_") for m in _malformed()])
def test_malformed_input_is_reported_and_nothing_is_written(capi, what, nf, blocks, status):
    call = RawCall(capi, nf, blocks)
    assert call.launch() == 0  # the host cannot see it: the status word says so
    mm, mem, counts = call.result()  # (asserts that every output byte still holds the sentinel)
    assert counts[:3] == [0, 0, status], (what, counts)
    assert len(mm) == 0 and len(mem) == 0
    with pytest.raises(capi.MalformedPairList):
        capi.merge_matches_device(nf, [len(b) for b in blocks], call.pairs_d)


@pytest.mark.parametrize("V", [1, 33])
def test_one_image_and_33_images_are_refused_by_the_host_check(capi, V):
    """2..32 images: refused before anything is queued -- counts and outputs keep their prefill"""
    nf = [4] * V
    assert workspace_bytes(capi, nf, 0) == 0
    call = RawCall(capi, nf, [np.zeros(0, C.PAIR)] * (V * (V - 1) // 2))
    assert call.launch() == INVALID_ARG
    torch.cuda.synchronize()
    assert call.counts_d.cpu().tolist() == [-1] * 4
    assert (call.mm_d.cpu().numpy() == SENTINEL).all() and (call.mem_d.cpu().numpy() == SENTINEL).all()
    with pytest.raises(ValueError):
        capi.merge_matches_device(nf, [], torch.zeros(16, dtype=torch.uint8, device="cuda"))


def test_match_set_of_the_flow_is_the_reference_s(capi, monkeypatch):
    """pipeline.build_match_set (device merge + device KeyPoint gather, no host merge anywhere) on the 8-view tracks: the
    MultiMatch array is the reference's, every KeyPoint is {image, loc of that feature} by a numpy lookup"""
    import helpers as H
    from ssrlcv_amd import pipeline
    monkeypatch.delenv("SSRLCV_MERGE_HOST", raising=False)
    name = "tracks_v8_mixed"
    nf, blocks = C.case(name)
    mm_r, mem_r, _ = C.reference(name)
    rng = np.random.default_rng(8)
    locs, feats = [], []
    for n in nf:
        f = np.zeros(n, H.FEATURE)
        f["loc"] = rng.random((n, 2), dtype=np.float32) * 1000
        locs.append(f["loc"].copy())
        feats.append(capi.to_dev(f))
    pair_tensors = [capi.to_dev(b) if len(b) else torch.zeros(0, dtype=torch.uint8, device="cuda") for b in blocks]
    dev = {}
    mm, kp = pipeline.build_match_set(feats, pair_tensors, dev)
    assert np.array_equal(mm["numKeyPoints"], mm_r[:, 0]) and np.array_equal(mm["index"], mm_r[:, 1].astype(np.int32))
    assert len(kp) == len(mem_r) and np.array_equal(kp["parentId"], mem_r[:, 0].astype(np.int32))
    want = np.stack([locs[i][f] for i, f in mem_r.tolist()])
    assert np.array_equal(np.ascontiguousarray(kp["loc"]).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dev["matches"].cpu().numpy().view("<u4").reshape(-1, 2), mm_r)
