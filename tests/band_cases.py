"""Seeded, deterministic inputs that take the band-culled matcher (csrc/matcher.hip run_match, csrc/matcher_i8.inc
k_match_i8<true, kQT8Band>) past one super-group of targets: three box levels, a hit list that fills and rolls over, a jump
over a whole super-group, a target split that straddles a super-group seam.  tests/test_gpu_match_band.py runs them on the
device against the CPU oracle; tests/test_band_cases.py shows without a GPU that they reach what they claim.  Every size is
derived from a named constant of the code it crosses, and tests/test_band_cases.py reads those constants and the two loops
back out of the sources, so a retuned kernel fails there first instead of leaving these sizes beside the seams."""
import functools
import math

import numpy as np

import helpers as H

# ---- csrc/matcher.hip, csrc/matcher_i8.inc
TILE = 32                          # targets per tile (one MFMA operand)
GROUP = 32 * TILE                  # 1 024: targets per group box
SUPER = 32 * GROUP                 # 32 768: targets per super-group box (stored at groupBox + numGroups)
HIT_LIST = 64                      # hit groups a wave collects before it visits them (one lane of `glist` each)
WAVES = 4                          # kWaves
QT, QT8, QT8_BAND = 4, 4, 1        # kQT, kQT8Brute, kQT8Band: query tiles of 32 per wave
Q_PER_BLOCK = WAVES * QT * 32               # 512: fp16 kernels
Q_PER_BLOCK8 = WAVES * QT8 * 32             # 512: int8 brute force
Q_PER_BLOCK8_BAND = WAVES * QT8_BAND * 32   # 128: int8 band-culled
SPLIT_GRID = 512                   # run_match's band branch splits the targets while the grid has fewer blocks than this
Q_PAD = math.lcm(Q_PER_BLOCK, Q_PER_BLOCK8, Q_PER_BLOCK8_BAND)
ARITHS = ("i8", "f16")


def nq_pad(nq):
    """make_layout: the query rows, a multiple of every kernel's queries per block"""
    return -(-max(nq, 1) // Q_PAD) * Q_PAD


def band_blocks(nq, arith):
    """qbBand of run_match: grid.x of the band-culled launch"""
    return nq_pad(nq) // (Q_PER_BLOCK8_BAND if arith == "i8" else Q_PER_BLOCK)


def launch_shape(nq, nt, arith="i8"):
    """the split rule of run_match's band branch -> (numGroups, numSuper, splits, groupsPerSplit)"""
    assert arith in ARITHS
    num_tiles = -(-max(nt, 1) // TILE)
    num_groups = -(-num_tiles // 32)
    num_super = -(-num_groups // 32)
    qb, splits = band_blocks(nq, arith), 1
    while qb * splits < SPLIT_GRID and splits * 2 <= num_groups:
        splits *= 2
    return num_groups, num_super, splits, -(-num_groups // splits)


def split_ranges(shape):
    """-> [(first group, one past the last group)] of the splits that hold a group (grid.y may be larger)"""
    num_groups, _, splits, per = shape
    return [(s * per, min((s + 1) * per, num_groups)) for s in range(splits) if s * per < num_groups]


def seam_splits(shape):
    """-> {seam (a, a + 1): first group of the split that walks groups of both super-groups}"""
    return {(b // 32 - 1, b // 32): g0 for g0, g1 in split_ranges(shape) for b in range(32, shape[0], 32) if g0 < b < g1}


# ---- the sets
N_CLUSTERS = 2 * SUPER + 1500      # 67 036: 66 groups, three super-groups; the last holds two groups, its last group 476
N_CLUSTERS_64 = HIT_LIST * GROUP   # 65 536: 64 groups, exactly two full super-groups, a hit list exactly full
CLUSTER_Y = ((0.0, 200.0), (1000.0, 1200.0), (2000.0, 2200.0))   # the three bands of y, 800 px apart
CLUSTER_COUNTS = (SUPER, SUPER, 1500)
CLUSTER_W = 4096.0
assert sum(CLUSTER_COUNTS) == N_CLUSTERS and (N_CLUSTERS, N_CLUSTERS_64) == (67036, 65536)
assert N_CLUSTERS % GROUP == 476 and N_CLUSTERS % TILE == 28          # partial last group, partial last tile

F_HORIZONTAL = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]], np.float32)   # the line of (x, y) is Y = y
F_TILTED = np.array([[0.0, -1e-4, 0.02], [1e-4, 0.0, -0.9], [-0.03, 1.0, 40.0]], np.float32)  # tests/test_gpu_matcher.py
EPS_NARROW, EPS_WIDE = 3.0, 1.0e4
REL, ABS = 0.9, 3.0e7
NQ = {"q700": 700, "q3000": 3000, "q65536": 65536}
QUERY_STRIDE_NARROW, QUERY_STRIDE_WIDE = 8, 64      # q65536: the oracle runs on every 8th (8 192) / 64th (1 024) query


def _features(n, rng, loc):
    f = np.zeros(n, H.FEATURE)
    f["parent"] = -1
    f["values"] = rng.integers(0, 48, (n, 128), dtype=np.uint8)
    f["loc"] = loc.astype(np.float32)
    f["sigma"] = 1.0
    return f


def _cluster_locs(counts, rng):
    loc = np.empty((sum(counts), 2), np.float64)
    at = 0
    for (y0, y1), n in zip(CLUSTER_Y, counts):
        loc[at:at + n, 0] = rng.uniform(0.0, CLUSTER_W, n)
        loc[at:at + n, 1] = rng.uniform(y0, y1, n)
        at += n
    return loc[rng.permutation(len(loc))]       # the caller's order is not the frame's order


def _frozen(f):
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def targets(name):
    """"clusters", "clusters_64", "uniform1024" (mode 1, the fixture cameras), "uniform4096" (mode 2, F_TILTED) -> FEATURE[]"""
    if name == "clusters":
        rng = np.random.default_rng(6101)
        return _frozen(_features(N_CLUSTERS, rng, _cluster_locs(CLUSTER_COUNTS, rng)))
    if name == "clusters_64":
        return _frozen(targets("clusters")[:N_CLUSTERS_64].copy())
    side = {"uniform1024": 1024.0, "uniform4096": 4096.0}[name]
    rng = np.random.default_rng(6102 if side == 1024.0 else 6103)
    return _frozen(_features(N_CLUSTERS, rng, rng.uniform(0.0, side, (N_CLUSTERS, 2))))


@functools.lru_cache(maxsize=None)
def queries(name, where):
    """name in NQ; where = "clusters" (a third of the queries in each band of y) or a uniform target set's area"""
    n = NQ[name]
    rng = np.random.default_rng(6200 + 7 * sorted(NQ).index(name) + ("clusters", "uniform1024", "uniform4096").index(where))
    if where == "clusters":
        return _frozen(_features(n, rng, _cluster_locs((n - 2 * (n // 3), n // 3, n // 3), rng)))
    side = {"uniform1024": 1024.0, "uniform4096": 4096.0}[where]
    return _frozen(_features(n, rng, rng.uniform(0.0, side, (n, 2))))


def every(q, stride):
    """-> (every stride-th query as an array of its own, their indices in q)"""
    return np.ascontiguousarray(q[::stride]), np.arange(0, len(q), stride)


def cluster_of(loc):
    """-> the band of y a location lies in (0, 1, 2)"""
    y = np.asarray(loc)[..., 1]
    c = np.full(y.shape, -1)
    for k, (y0, y1) in enumerate(CLUSTER_Y):
        c[(y >= y0) & (y < y1 + 1.0)] = k      # (a float32 rounding of a y just below y1 may land on y1)
    assert (c >= 0).all()
    return c


def candidates_horizontal(q, t, eps):
    """mode 2 with F_HORIZONTAL, the oracle's per-pair test in its own float32 arithmetic (oracle/oracle_match.c:155-159):
    the line of a query is (a, b, c) = (0, -1, y), p = -1 * ((a * X) + c) / b = y, a candidate has |Y - p| <= eps
    -> bool [len(q), len(t)]"""
    F = F_HORIZONTAL
    ql = q["loc"].astype(np.float32)
    a = (F[0, 0] * ql[:, 0]) + (F[0, 1] * ql[:, 1]) + F[0, 2]
    b = (F[1, 0] * ql[:, 0]) + (F[1, 1] * ql[:, 1]) + F[1, 2]
    c = (F[2, 0] * ql[:, 0]) + (F[2, 1] * ql[:, 1]) + F[2, 2]
    tx, ty = t["loc"][:, 0].astype(np.float32), t["loc"][:, 1].astype(np.float32)
    p = np.float32(-1.0) * ((a[:, None] * tx[None, :]) + c[:, None]) / b[:, None]
    return ~(np.abs(ty[None, :] - p) > np.float32(eps))
