"""The cases of tests/band_cases.py reach what they claim, shown without a GPU: the constants, the query padding, the split
rule and the two loops of the walk are read back out of csrc/matcher.hip and csrc/matcher_i8.inc; every case gets the split
count and the groups per split it names, the splits that straddle a super-group seam are named, the one-split cases put more
than / exactly a hit list of groups into one walk; and on the oracle alone the narrow cases have accepted targets in every
cluster and no candidate across clusters, the wide cases make every target a candidate of every query.
tests/test_gpu_match_band.py then holds the kernels to the oracle on the same cases."""
import os
import re

import numpy as np
import pytest

import band_cases as C
import helpers as H

CSRC = os.path.join(H.ROOT, "ssrlcv_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_the_constants_are_the_sources():
    m, i8 = source("matcher.hip"), source("matcher_i8.inc")
    assert int(one(r"constexpr int kWaves = (\d+);", m)) == C.WAVES
    assert int(one(r"#define SSRLCV_MATCH_QT (\d+)\n", m)) == C.QT
    assert int(one(r"#define SSRLCV_MATCH_QT8 (\d+)\n", i8)) == C.QT8
    assert int(one(r"#define SSRLCV_MATCH_QT8_BAND (\d+)\n", i8)) == C.QT8_BAND           # kQT8Band's default
    one(r"constexpr int kQT = SSRLCV_MATCH_QT;", m)
    one(r"constexpr int kQT8Brute = SSRLCV_MATCH_QT8, kQT8Band = SSRLCV_MATCH_QT8_BAND;", i8)
    one(r"constexpr int kQPerBlock = kWaves \* kQT \* 32;", m)
    one(r"constexpr int kQPerBlock8 = kWaves \* kQT8Brute \* 32;", i8)
    one(r"constexpr int kQPerBlock8Band = kWaves \* kQT8Band \* 32;", i8)
    # no build of the library retunes them from the command line
    assert not re.search(r"SSRLCV_MATCH_QT|kWaves", source("Makefile"))
    assert (C.Q_PER_BLOCK, C.Q_PER_BLOCK8, C.Q_PER_BLOCK8_BAND, C.Q_PAD) == (512, 512, 128, 512)
    assert (C.TILE, C.GROUP, C.SUPER, C.HIT_LIST) == (32, 1024, 32768, 64)


def test_the_padding_and_the_split_rule_are_the_sources():
    m = source("matcher.hip")
    one(r"L\.nq_pad = round_up\(nq \? nq : 1, lcm_u32\(kQPerBlock, lcm_u32\(kQPerBlock8, kQPerBlock8Band\)\)\);", m)
    one(r"L\.nt_pad = round_up\(nt \? nt : 1, 32\);", m)
    one(r"uint32_t qblocks = L\.nq_pad / \(useF16 \? kQPerBlock : kQPerBlock8\);", m)
    one(r"uint32_t numTiles = L\.nt_pad / 32;", m)
    body = m[m.index("int run_match("):m.index("struct Layout2")]
    band = body[body.index("  if (band) {\n    Box* tileBox"):body.index("  } else {\n    // split the target range")]
    one(r"const uint32_t numGroups = \(numTiles \+ 31\) / 32;", band)
    one(r"const uint32_t numSuper = \(numGroups \+ 31\) / 32;", band)
    one(r"const uint32_t qbBand = useF16 \? qblocks : L\.nq_pad / kQPerBlock8Band;", band)
    assert int(one(r"uint32_t splits = 1;\s+while \(qbBand \* splits < (\d+) && splits \* 2 <= numGroups\) splits \*= 2;", band)) == C.SPLIT_GRID
    one(r"uint32_t tilesPerSplit = \(\(numGroups \+ splits - 1\) / splits\) \* 32;", band)
    # the two kernels of the branch, on a grid of (qbBand or qblocks, splits); the super boxes behind the group boxes
    one(r"hipLaunchKernelGGL\(\(k_match_i8<true, kQT8Band>\), dim3\(qbBand, splits\), dim3\(256\)", band)
    one(r"hipLaunchKernelGGL\(k_match<true>, dim3\(qblocks, splits\), dim3\(256\)", band)
    one(r"hipLaunchKernelGGL\(k_group_boxes, dim3\(\(numSuper \+ 255\) / 256\), dim3\(256\), 0, st, \(const Box\*\)groupBox, numGroups, numSuper,\s+groupBox \+ numGroups\);", band)
    # a box of the next level is the union of 32 children
    boxes = m[m.index("void k_group_boxes("):m.index("__device__ __forceinline__ bool band_hits_box(")]
    one(r"for \(uint32_t j = 0; j < (32); \+\+j\) \{\s+uint32_t t = g \* 32 \+ j;", boxes)


def test_the_walk_is_the_source():
    i8 = source("matcher_i8.inc")
    walk = i8[i8.index("  if constexpr (BAND) {"):i8.index("    if (pend) visit(pendTile, pendPar, pendNeed);")]
    one(r"const Box\* superBox = groupBox \+ numGroups;", walk)
    one(r"const uint32_t grEnd = \(tile1 \+ 31\) / 32 < numGroups \? \(tile1 \+ 31\) / 32 : numGroups;", walk)
    one(r"uint32_t gr = tile0 / 32, curSuper = ~0u;", walk)
    assert int(one(r"while \(gr < grEnd\) \{\s+uint32_t n = 0;\s+while \(gr < grEnd && n < (\d+)\) \{", walk)) == C.HIT_LIST
    one(r"if \(gr / 32 != curSuper\) \{\s+curSuper = gr / 32;", walk)
    one(r"band_hits_box\(gr_\[qt\], superBox\[curSuper\]\);", walk)
    one(r"if \(!__any\(sh\)\) \{ gr = \(curSuper \+ 1\) \* 32; continue; \}", walk)
    one(r"if \(__any\(gh\)\) \{ glist = lane == n \? \(int\)gr : glist; \+\+n; \}\s+\+\+gr;", walk)
    # visited from the middle of the list outwards; a lane of the wave per entry, hence the 64
    one(r"const uint32_t mid = n \? \(n - 1\) / 2 : 0;", walk)
    one(r"const uint32_t j = \(k & 1u\) \? mid \+ \(k \+ 1\) / 2 : mid - k / 2;", walk)


def test_padding_and_blocks_of_the_query_sets():
    assert [C.nq_pad(n) for n in (0, 1, 512, 513, 700, 3000, 65536)] == [512, 512, 512, 1024, 1024, 3072, 65536]
    assert [C.band_blocks(C.NQ[q], "i8") for q in ("q700", "q3000", "q65536")] == [8, 24, 512]
    assert [C.band_blocks(C.NQ[q], "f16") for q in ("q700", "q3000", "q65536")] == [2, 6, 128]


def test_launch_shapes_and_the_splits_that_span_a_seam():
    big, full = C.N_CLUSTERS, C.N_CLUSTERS_64
    assert len(C.targets("uniform1024")) == len(C.targets("uniform4096")) == big     # the same shapes as `clusters`
    # q3000: 32 splits of 3 groups, 22 of them hold groups; two walk groups of two super-groups
    shape = C.launch_shape(3000, big)
    assert shape == (66, 3, 32, 3)
    ranges = C.split_ranges(shape)
    assert len(ranges) == 22 and ranges[-1] == (63, 66) and all(b - a == 3 for a, b in ranges)
    assert C.seam_splits(shape) == {(0, 1): 30, (1, 2): 63}
    assert (30, 33) in ranges and (63, 66) in ranges
    # ... on exactly two super-groups the splits of 2 groups end on the seam: none spans it
    assert C.launch_shape(3000, full) == (64, 2, 32, 2) and C.seam_splits(C.launch_shape(3000, full)) == {}
    # q700: the grid is smaller, the targets are split as far as the groups allow: 64 splits of 2 groups, 33 of them hold groups
    shape = C.launch_shape(700, big)
    assert shape == (66, 3, 64, 2)
    assert len(C.split_ranges(shape)) == 33 and C.seam_splits(shape) == {}
    # the fp16 kernel's blocks hold four times the queries: it always splits down to 2 groups here
    assert C.launch_shape(3000, big, "f16") == (66, 3, 64, 2) == C.launch_shape(700, big, "f16")
    # q65536: 512 blocks, no split: one wave walks every group, across both seams
    shape = C.launch_shape(65536, big)
    assert shape == (66, 3, 1, 66) and shape[3] > C.HIT_LIST and shape[3] - C.HIT_LIST == 2     # a second batch of two
    assert C.split_ranges(shape) == [(0, 66)] and C.seam_splits(shape) == {(0, 1): 0, (1, 2): 0}
    shape = C.launch_shape(65536, full)
    assert shape == (64, 2, 1, 64) and shape[3] == C.HIT_LIST                                     # a list exactly full
    # one query fewer than 512 blocks' worth and the targets are split again
    assert C.launch_shape(65536 - 512, big)[2] == 2


def test_the_sets_are_what_they_claim():
    t = C.targets("clusters")
    assert len(t) == 67036 and -(-len(t) // C.GROUP) == 66 and -(-len(t) // C.SUPER) == 3
    cl = C.cluster_of(t["loc"])
    assert np.bincount(cl).tolist() == list(C.CLUSTER_COUNTS)
    assert (np.diff(cl) != 0).sum() > 20000                   # the caller's order is not the frame's
    # in the frame of horizontal bands (strips along y) each cluster fills whole super-groups: ranks by y
    rank = np.argsort(np.argsort(t["loc"][:, 1], kind="stable"), kind="stable")
    assert np.array_equal(rank // C.SUPER, cl)
    t64 = C.targets("clusters_64")
    assert len(t64) == 64 * C.GROUP == 2 * C.SUPER and np.array_equal(t64, t[:len(t64)])
    assert (np.bincount(C.cluster_of(t64["loc"])) > 1000).all()           # all three clusters, in two super-groups
    for name, side in (("uniform1024", 1024.0), ("uniform4096", 4096.0)):
        loc = C.targets(name)["loc"]
        assert loc.min() >= 0 and loc.max() <= side and loc.max() > 0.99 * side
    for where in ("clusters", "uniform1024", "uniform4096"):
        for name, n in C.NQ.items():
            if where == "clusters" or name == "q3000":
                q = C.queries(name, where)
                assert len(q) == n and q["values"].max() == 47
                if where == "clusters":
                    assert (np.bincount(C.cluster_of(q["loc"])) >= n // 3).all()


def _pairs(oracle_lib, q, t, eps):
    return H.oracle_match_pairs(oracle_lib, 2, 3, q, 7, t, None, C.F_HORIZONTAL.reshape(-1), eps, 0.0, None, C.REL, C.ABS)


@pytest.mark.parametrize("tname", ["clusters", "clusters_64"])
def test_narrow_cases_accept_targets_in_every_cluster_and_none_across(oracle_lib, tname):
    t = C.targets(tname)
    tc = C.cluster_of(t["loc"])
    for qname, stride in (("q3000", 1), ("q65536", C.QUERY_STRIDE_NARROW)):
        q = C.every(C.queries(qname, "clusters"), stride)[0]
        qc = C.cluster_of(q["loc"])
        o = _pairs(oracle_lib, q, t, C.EPS_NARROW)
        assert np.array_equal(o["a"][:, 1], np.arange(len(q)))
        ok = o["b"][:, 0] == 7
        # accepted targets in every cluster, the 1 500-target one included, each in its query's own cluster
        assert (np.bincount(qc[ok], minlength=3) > 0.95 * np.bincount(qc, minlength=3)).all(), np.bincount(qc[ok], minlength=3)
        assert np.array_equal(tc[o["b"][ok, 1]], qc[ok])
    # the per-pair test itself: a query's candidates all lie in its own cluster, and every cluster has queries with some
    q = C.every(C.queries("q3000", "clusters"), 8)[0]
    qc = C.cluster_of(q["loc"])
    for eps in (C.EPS_NARROW, 40.0):
        cand = C.candidates_horizontal(q, t, eps)
        assert not (cand & (qc[:, None] != tc[None, :])).any()
        per_query = cand.sum(1)
        assert all((per_query[qc == k] > 0).any() for k in range(3))
    # the oracle's winner is the candidate the reference's rule picks: smallest distance, then lowest f mod 32, then lowest f
    o = _pairs(oracle_lib, q, t, C.EPS_NARROW)
    cand = C.candidates_horizontal(q, t, C.EPS_NARROW)
    for i in range(0, len(q), 15):
        f = np.flatnonzero(cand[i])
        if len(f) == 0:
            assert o["b"][i, 0] == 3
            continue
        d = ((q["values"][i].astype(np.int64) - t["values"][f].astype(np.int64)) ** 2).sum(1)
        best = f[np.lexsort((f, f % 32, d))[0]]
        assert o["b"][i].tolist() == [7, best]


def test_wide_cases_make_every_target_a_candidate_of_every_query(oracle_lib):
    for tname in ("clusters", "clusters_64"):
        t = C.targets(tname)
        for qname in ("q700", "q65536"):
            q = C.queries(qname, "clusters")
            # |Y - y| <= 2 201 px for every pair, far inside epsilon; and the float32 test itself on a share of the queries
            assert float(t["loc"][:, 1].max()) - float(q["loc"][:, 1].min()) < 0.5 * C.EPS_WIDE
            assert float(q["loc"][:, 1].max()) - float(t["loc"][:, 1].min()) < 0.5 * C.EPS_WIDE
            assert C.candidates_horizontal(C.every(q, max(1, len(q) // 64))[0], t, C.EPS_WIDE).all()
    # then the band-culled contract is the brute-force one: the oracle says so on a few queries
    q, t = C.every(C.queries("q700", "clusters"), 50)[0], C.targets("clusters")
    o2 = _pairs(oracle_lib, q, t, C.EPS_WIDE)
    o0 = H.oracle_match_pairs(oracle_lib, 0, 3, q, 7, t, None, None, 0.0, 0.0, None, C.REL, C.ABS)
    assert np.array_equal(o2["a"], o0["a"]) and np.array_equal(o2["b"], o0["b"]) and (o2["b"][:, 0] == 7).all()
