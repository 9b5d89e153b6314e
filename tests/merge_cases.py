"""Inputs for the N-view merge (generateMatchesExhaustive's host half) that reach what `random_pairs` of
test_merge_parallel.py almost never reaches: walks of several hops, intersections of two long lists, accepted multi-matches
of four and more key points clearing lists of later images, conflict chains beyond the device's round limit, every grid
shape of the persistent kernel, and every configuration of four small models.  A case is (num_features, blocks): one
PAIR array per image pair in the reference's pair order (0,1), (0,2) .. (1,2) ..  Built once per process (case()) together
with what tests/merge_ref.py makes of it (reference()).

tests/test_merge_cases.py proves on the CPU that the cases hold what they promise; tests/test_gpu_merge_edges.py runs
every one of them through the device merge."""
import functools
import itertools

import numpy as np

from merge_ref import PAIR, merge_ref


def pair_list(V):
    return [(q, t) for q in range(V - 1) for t in range(q + 1, V)]


def block(q, t, qf, tf):
    blk = np.zeros(len(qf), PAIR)
    blk["a"][:, 0], blk["a"][:, 1] = q, qf
    blk["b"][:, 0], blk["b"][:, 1] = t, tf
    return blk


def from_dict(V, entries):
    """{(q, t): [(query feature, target feature), ..]} -> blocks in pair order"""
    assert all(k in pair_list(V) for k in entries), entries.keys()
    return [block(q, t, [e[0] for e in entries.get((q, t), [])], [e[1] for e in entries.get((q, t), [])]) for q, t in pair_list(V)]


# ---- tracks: scene points seen in a subset of the images at a private feature index each -----------------------------------
def tracks(seed, nf, vis, drop=0.0, wrong=0.0, collide=0.0, points=None):
    """Every scene point is seen by an image with probability `vis`, at a feature index of its own there.  The pair (q, t)
    matches the points both see, queries ascending; a match is left out with probability `drop`, goes to a random feature
    of t with probability `wrong`, or takes the target of the previous query of its block with probability `collide`
    (chains of them copy along).  No block holds a query twice."""
    rng = np.random.default_rng(seed)
    V, P = len(nf), int(points if points is not None else max(nf))
    feat = np.full((V, P), -1, np.int64)
    for i in range(V):
        seen = np.nonzero(rng.random(P) < vis)[0]
        if len(seen) > nf[i]:
            seen = np.sort(rng.permutation(seen)[: nf[i]])
        feat[i, seen] = rng.permutation(nf[i])[: len(seen)]
    blocks = []
    for q, t in pair_list(V):
        both = np.nonzero((feat[q] >= 0) & (feat[t] >= 0))[0]
        both = both[np.argsort(feat[q, both])]
        both = both[rng.random(len(both)) >= drop]
        qf, tf = feat[q, both], feat[t, both].copy()
        w = rng.random(len(both)) < wrong
        tf[w] = rng.integers(0, nf[t], int(w.sum()))
        for k in np.nonzero(rng.random(len(both)) < collide)[0]:
            if k:
                tf[k] = tf[k - 1]
        assert len(np.unique(qf)) == len(qf)
        blocks.append(block(q, t, qf, tf))
    return [int(n) for n in nf], blocks


TRACKS = {
    "tracks_v4_clean": dict(seed=401, nf=[1200, 1100, 1300, 1000], vis=0.8),
    "tracks_v4_drop": dict(seed=402, nf=[1500, 1400, 1450, 1300], vis=0.85, drop=0.15),
    "tracks_v5_mixed": dict(seed=501, nf=[1400, 1300, 1350, 1200, 1250], vis=0.8, drop=0.1, wrong=0.06, collide=0.06),
    "tracks_v8_mixed": dict(seed=801, nf=[900, 850, 800, 880, 820, 870, 790, 860], vis=0.75, drop=0.06, wrong=0.03, collide=0.03),
    "tracks_v6_collide": dict(seed=601, nf=[1200, 1100, 1150, 1000, 1050, 1100], vis=0.8, drop=0.05, wrong=0.02, collide=0.3),
    "tracks_v32_mixed": dict(seed=3201, nf=[300 + 7 * (i % 5) for i in range(32)], vis=0.6, drop=0.02, wrong=0.004, collide=0.004),
    "tracks_v32_full": dict(seed=3202, nf=[80] * 32, vis=1.0, points=64),
}
# tracks_v4_drop again with the largest seed image at N features: 1, 1, 1, 2, 16, 17, 34 and (CU count) blocks of the
# persistent kernel -- barrier groups uneven, full and wrapped; 70 000 takes the grid-stride loops.  682, 683 and 684 give
# 1023, 1024 and 1026 seeds (N + N // 2: the first two images seed): either side of k_merge_emit's tile of 256 x 4 seeds
GRID_SIZES = (1, 255, 256, 257, 682, 683, 684, 3841, 4097, 8449, 70000)
EMIT_TILE = 1024
assert [n + n // 2 for n in GRID_SIZES[4:7]] == [EMIT_TILE - 1, EMIT_TILE, EMIT_TILE + 2]


def grid(n):
    rest = max(1, n // 2)
    return tracks(402 + n, [n, rest, rest, rest], vis=0.85, drop=0.15)


# ---- small models: every configuration "feature f of image q matches nothing or one feature of image t", in one problem ------
SMALL_MODELS = ([2, 2, 2], [2, 2, 1, 1], [1, 2, 2, 2], [2, 2, 2, 1])
SMALL_MODEL_CONFIGS = (729, 4608, 19683, 46656)


def _digits(nf):
    """(q, t, f, radix) of every digit of a configuration number, least significant first"""
    return [(q, t, f, nf[t] + 1) for q, t in pair_list(len(nf)) for f in range(nf[q])]


def small_model_configs(nf):
    return int(np.prod([r for _, _, _, r in _digits(nf)]))


def small_model(nf, interleave):
    """All K configurations side by side: configuration k owns features [k nf_i, (k + 1) nf_i) of image i -- or interleaved,
    feature index local x K + k, so that the seeds of one configuration sit in different waves and blocks."""
    K = small_model_configs(nf)
    k = np.arange(K, dtype=np.int64)
    place = (lambda local, n: local * K + k) if interleave else (lambda local, n: k * n + local)
    per_pair, div = {}, 1
    for q, t, f, radix in _digits(nf):
        d = (k // div) % radix
        div *= radix
        sel = d > 0
        per_pair.setdefault((q, t), []).append((place(f, nf[q])[sel], place(d - 1, nf[t])[sel]))
    blocks = []
    for q, t in pair_list(len(nf)):
        qf = np.concatenate([p[0] for p in per_pair[(q, t)]])
        tf = np.concatenate([p[1] for p in per_pair[(q, t)]])
        o = np.argsort(qf, kind="stable")
        blocks.append(block(q, t, qf[o], tf[o]))
    return [n * K for n in nf], blocks


def small_model_single(nf, k):
    """configuration k of the model as a problem of its own"""
    entries, div = {}, 1
    for q, t, f, radix in _digits(nf):
        d = (k // div) % radix
        div *= radix
        if d:
            entries.setdefault((q, t), []).append((f, d - 1))
    return list(nf), from_dict(len(nf), entries)


def per_configuration(nf, interleave, mm, mem):
    """The packed problem's output split by configuration: K tuples of records, a record = its (image, local feature)s."""
    K = small_model_configs(nf)
    per_image = np.array(nf, np.int64)[mem[:, 0].astype(np.int64)]
    feat = mem[:, 1].astype(np.int64)
    cfg, local = (feat % K, feat // K) if interleave else (feat // per_image, feat % per_image)
    out = [[] for _ in range(K)]
    img = mem[:, 0].tolist()
    cfg_l, local_l = cfg.tolist(), local.tolist()
    for n, at in mm.tolist():
        assert len(set(cfg_l[at: at + n])) == 1, "a multi-match crosses configurations"
        out[cfg_l[at]].append(tuple(zip(img[at: at + n], local_l[at: at + n])))
    return [tuple(o) for o in out]


# ---- conflict chains: every seed of an image depends on the one before it ----------------------------------------------------
def chain(n, image=0, V=3):
    """Every seed of `image` is matched to the SAME feature 3 of the next image (which goes on to feature 5 of the one after),
    every other seed also to that feature 5 directly: one seed resolves per round."""
    nf = [8] * V
    nf[image] = n
    i = image
    entries = {(i, i + 1): [(f, 3) for f in range(n)], (i, i + 2): [(f, 5) for f in range(0, n, 2)], (i + 1, i + 2): [(3, 5)]}
    return nf, entries


def tail_image1():
    nf, entries = chain(300, image=1, V=4)
    # image 0: (0,1) = {(1,6), (3,5)} is inconsistent with (1,6) = {(2,3), (3,5)}; (0,2) = {(1,9), (2,3)} is accepted and
    # clears the chain seed (1,9), not the chain's shared list (2,3)
    entries[(0, 1)] = [(1, 6), (2, 9)]
    entries[(0, 2)] = [(2, 3)]
    entries[(0, 3)] = [(1, 5)]
    return nf, from_dict(4, entries)


def tail_two_images():
    """Chains on images 0 and 1 in one call: image 0's seeds share (1, 4), image 1's share (2, 3)."""
    n = 300
    entries = {(0, 1): [(f, 4) for f in range(n)], (0, 2): [(f, 3) for f in range(0, n, 2)], (0, 3): [(f, 5) for f in range(0, n, 2)],
               (1, 2): [(g, 3) for g in range(n)], (1, 3): [(g, 5) for g in range(0, n, 2)], (2, 3): [(3, 5)]}
    return [n, n, 8, 8], from_dict(4, entries)


def tail_mixed(groups=100):
    """A chain on image 1 of V = 5 whose seeds are accepted, rejected and skipped in turn.  Image 1 has three features per
    group j: 3j and 3j + 1 are chain seeds, 3j + 2 is cleared by seed j of image 0.  Chain seed c = {(2, x_c), (3, 0),
    (4, e_c)}: every one would clear the hub (3, 0) and list (2, x) = {(3, 0), (4, 0)} leads to it, so the seeds resolve
    nearly one per round.  e_c = 1 is an inconsistent direct entry to the last image: rejected while (2, x_c) is alive.
    By c mod 4: 0 accepted, clears (2, x); 1 shares that x and e = 1: accepted only because its lower neighbour cleared
    (2, x); 2 own x, e = 1: rejected; 3 own x: accepted."""
    J, C = groups, 2 * groups
    seeds1 = [3 * (c // 2) + (c % 2) for c in range(C)]
    x = [c - 1 if c % 4 == 1 else c for c in range(C)]
    e = [1 if c % 4 in (1, 2) else 0 for c in range(C)]
    entries = {(0, 1): [(j, 3 * j + 2) for j in range(J)], (0, 4): [(j, 0) for j in range(J)],
               (1, 2): [(seeds1[c], x[c]) for c in range(C)], (1, 3): [(seeds1[c], 0) for c in range(C)],
               (1, 4): sorted([(seeds1[c], e[c]) for c in range(C)] + [(3 * j + 2, 0) for j in range(J)]),
               (2, 3): [(xx, 0) for xx in sorted(set(x))], (2, 4): [(xx, 0) for xx in sorted(set(x))], (3, 4): [(0, 0)]}
    return [J, 3 * J, C, 1, 2], from_dict(5, entries)


# ---- hand-made cases, the expected arrays written out ---------------------------------------------------------------------
# name: (num_features, {(q, t): [(query, target)]}, MultiMatch {numKeyPoints, index}, members {image, feature}, device takes it)
HAND = {
    # (0,0) is accepted and clears (1,0); (0,1) then finds (1,0) empty and is accepted (alive, {(2,0)} is not in its list)
    "hand_reads_what_a_lower_seed_clears": (
        [2, 2, 2], {(0, 1): [(0, 0), (1, 0)], (0, 2): [(0, 0), (1, 1)], (1, 2): [(0, 0)]},
        [(3, 0), (3, 3)], [(0, 0), (1, 0), (2, 0), (0, 1), (1, 0), (2, 1)], True),
    # (0,0) = {(1,0)} meets (1,0) = {(2,0)} alive: rejected; (0,1), which clears (1,0), comes too late to save it
    "hand_clears_what_a_lower_seed_reads": (
        [2, 2, 2], {(0, 1): [(0, 0), (1, 0)], (0, 2): [(1, 0)], (1, 2): [(0, 0)]},
        [(3, 0)], [(0, 1), (1, 0), (2, 0)], True),
    # (0,0) and (0,1) read nothing of each other's (their heads' lists are empty) and both clear (2,0);
    # (1,2) = {(2,0)} is accepted only because (2,0) = {(3,0)} is gone
    "hand_two_ready_seeds_clear_one_list": (
        [2, 3, 1, 1], {(0, 1): [(0, 0), (1, 1)], (0, 2): [(0, 0), (1, 0)], (0, 3): [(0, 0), (1, 0)], (1, 2): [(2, 0)], (2, 3): [(0, 0)]},
        [(4, 0), (4, 4), (2, 8)], [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 0), (3, 0), (1, 2), (2, 0)], True),
    # (0,1) hops to (1,1) = {(2,0), (3,1)} and stops at (2,0), which (0,0) cleared; alive, (2,0) = {(3,0)} would reject it
    "hand_walk_stops_at_a_list_cleared_in_the_same_image": (
        [2, 2, 1, 2], {(0, 1): [(0, 0), (1, 1)], (0, 2): [(0, 0), (1, 0)], (0, 3): [(0, 0), (1, 1)], (1, 2): [(0, 0), (1, 0)],
                       (1, 3): [(0, 0), (1, 1)], (2, 3): [(0, 0)]},
        [(4, 0), (4, 4)], [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 0), (3, 1)], True),
    # one point in all five images: two hops, then the one-entry list (3,0) = {(4,0)} ends the walk; (1,0), (2,0) are skipped
    "hand_two_hops_to_a_single_entry": (
        [1, 1, 1, 1, 1], {(q, t): [(0, 0)] for q, t in pair_list(5)},
        [(5, 0)], [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)], True),
    # Where no block holds a query twice a list has one entry per later image, ascending, so only its LAST entry can be in
    # the last image: `head in the last image` can end a walk only at the seed's own list, and the clearing loop's stop at
    # the last image only where it ends anyway.  With (0,0), (1,0) and (2,0) matched to BOTH features of image 3 (which only
    # the host walk takes) the walk stops at head (3,0) after two hops, and the clearing stops at (3,0) with (3,1) to go.
    "hand_last_image_twice": (
        [1, 1, 1, 2], {(0, 1): [(0, 0)], (0, 2): [(0, 0)], (0, 3): [(0, 0), (0, 1)], (1, 2): [(0, 0)], (1, 3): [(0, 0), (0, 1)],
                       (2, 3): [(0, 0), (0, 1)]},
        [(5, 0)], [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1)], False),
    # image 1 has three features and no pair, as query or as target
    "hand_image_without_pairs": (
        [2, 3, 2, 2], {(0, 2): [(0, 0), (1, 1)], (0, 3): [(0, 0)], (2, 3): [(0, 0), (1, 1)]},
        [(3, 0)], [(0, 0), (2, 0), (3, 0)], True),
    # image 2 of five has no feature at all
    "hand_empty_image_in_the_middle": (
        [2, 2, 0, 2, 2], {(0, 1): [(0, 0), (1, 1)], (0, 3): [(0, 0)], (0, 4): [(0, 0), (1, 1)], (1, 3): [(0, 0), (1, 1)],
                          (1, 4): [(0, 0), (1, 1)], (3, 4): [(0, 0), (1, 1)]},
        [(4, 0), (3, 4)], [(0, 0), (1, 0), (3, 0), (4, 0), (1, 1), (3, 1), (4, 1)], True),
}

HOST_ONLY = tuple(n for n, h in HAND.items() if not h[4])  # a query twice in one pair: the device refuses it (status 2)

SMALL_NAMES = tuple("small_model_%s_%s" % ("".join(map(str, nf)), how) for nf in SMALL_MODELS for how in ("packed", "interleaved"))
CASES = (tuple(TRACKS) + tuple("grid_%d" % n for n in GRID_SIZES) + SMALL_NAMES +
         ("tail_image0", "tail_image1", "tail_two_images", "tail_mixed", "chain_47", "chain_48", "chain_49") + tuple(HAND))
DEVICE_CASES = tuple(n for n in CASES if n not in HOST_ONLY)
# chains that outlast the device's 48 rounds per image -> the fewest rounds the call can report (tail_two_images: both
# images reach the limit; tail_mixed: one round for image 0, then the chain on image 1)
TAIL_ROUNDS = {"tail_image0": 48, "tail_image1": 48, "tail_two_images": 96, "tail_mixed": 49, "chain_49": 48}


def small_model_of(name):
    digits, how = name.split("_")[2:]
    return [int(c) for c in digits], how == "interleaved"


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (num_features, blocks), built once"""
    if name in TRACKS:
        return tracks(**TRACKS[name])
    if name.startswith("grid_"):
        return grid(int(name[5:]))
    if name.startswith("small_model_"):
        nf, interleave = small_model_of(name)
        return small_model(nf, interleave)
    if name == "tail_image0":
        nf, entries = chain(300)
        return nf, from_dict(3, entries)
    if name.startswith("chain_"):
        nf, entries = chain(int(name[6:]))
        return nf, from_dict(3, entries)
    if name in HAND:
        nf = HAND[name][0]
        return list(nf), from_dict(len(nf), HAND[name][1])
    return {"tail_image1": tail_image1, "tail_two_images": tail_two_images, "tail_mixed": tail_mixed}[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (mm, members, stats) of tests/merge_ref.py on the case, computed once; do not write into the arrays"""
    mm, mem, stats = merge_ref(*case(name))
    mm.setflags(write=False)
    mem.setflags(write=False)
    return mm, mem, stats


@functools.lru_cache(maxsize=None)
def order_dependent(name):
    """seeds whose outcome differs when every image's seeds are walked last to first"""
    fwd = reference(name)[2]["outcome"]
    bwd = merge_ref(*case(name), reverse=True)[2]["outcome"]
    return sum(fwd.get(k) != bwd.get(k) for k in set(fwd) | set(bwd))


def per_configuration_outcomes(nf, interleave, outcome):
    """The reference's per-seed outcomes split by configuration: K tuples of (image, local feature, outcome)."""
    K = small_model_configs(nf)
    out = [[] for _ in range(K)]
    for (i, f), o in sorted(outcome.items()):
        k, local = (f % K, f // K) if interleave else (f // nf[i], f % nf[i])
        out[k].append((i, local, o))
    return [tuple(o) for o in out]


assert len(set(CASES)) == len(CASES) and not set(itertools.chain(TRACKS, HAND)) - set(CASES)
