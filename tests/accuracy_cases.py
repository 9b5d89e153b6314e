"""The surface-accuracy cases: clouds, reference maps and frames for ssrlcv_hip_dsm_difference, value sets and parameters for
ssrlcv_hip_difference_stats, and the rendered scene of the end-to-end tests.  Shared by tests/test_accuracy_cases.py (which
proves on the numpy reference alone that every case exercises what it claims) and tests/test_gpu_accuracy.py (which holds the
kernels to that reference).  Every reference result is computed once, shared and never modified."""
from collections import namedtuple

import numpy as np

import accuracy_ref as A
import dsm_cases as DC
import dsm_ref as D
import mesh_ref as M

f32 = np.float32
NAN, INF = float("nan"), float("inf")
INVALID = A.INVALID

# ---- the difference
# exempt: the case says that MESH mode has no inside for it (a grid side below 2) or that it has no point
DiffCase = namedtuple("DiffCase", "points height frame max_jump exempt")


def _map(rows, holes=()):
    b = D.bits(np.array(rows, np.float32)).copy()
    for (j, i) in holes:
        b[j, i] = D.INVALID_BITS
    return b.view(np.float32)


def lattice(w, h, cell, beyond=0.75, z=None):
    """points at every quarter of a cell in u and v, `beyond` cells outside the grid on every side: s and t of MESH mode are 0, 1/4,
    1/2 or 3/4, so s == 0, t == 0, s == t and s + t == 1 all occur exactly, and so do u == w, v == h and the half cell at the border"""
    us = np.arange(-beyond, w + beyond + 0.125, 0.25)
    vs = np.arange(-beyond, h + beyond + 0.125, 0.25)
    uu, vv = np.meshgrid(us, vs)
    n = uu.size
    zz = (np.arange(n) % 17 - 8) * 0.125 if z is None else np.broadcast_to(z, (n,))
    return np.stack([uu.ravel() * cell, vv.ravel() * cell, zz], 1).astype(np.float32)


def interior(n, w, h, cell, seed, origin=(0, 0, 0)):
    """n random points over the part of the grid MESH mode calls inside (for a side below 2: over the grid)"""
    rng = np.random.RandomState(seed)
    lo_u, hi_u = (0.5, w - 0.5) if w >= 2 else (0.0, float(w))
    lo_v, hi_v = (0.5, h - 0.5) if h >= 2 else (0.0, float(h))
    p = np.empty((n, 3), np.float32)
    p[:, 0] = (lo_u + rng.rand(n) * (hi_u - lo_u) * 0.999) * cell + origin[0]
    p[:, 1] = (lo_v + rng.rand(n) * (hi_v - lo_v) * 0.999) * cell + origin[1]
    p[:, 2] = rng.randn(n) + origin[2]
    return p


SPECIAL_POINTS = np.array([(NAN, 1, 1), (1, NAN, 1), (1, 1, NAN), (INF, 1, 1), (1, -INF, 1), (1, 1, INF), (1, 1, -INF), (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0),
                           (1e30, 1, 1), (1, -1e30, 1), (1, 1, 3e38), (0.0, 0.0, 1.0), (-0.0, 1.0, 0.0)], np.float32)

# 7 x 5, multiples of 1/8: an invalid cell (cells with three valid corners around it), a spike that max_jump cuts, slopes of both
# signs so that both diagonals occur, an infinite and a NaN-valued (valid) height
RELIEF = _map([[0.0, 0.5, 1.0, 1.5, 1.0, 0.5, 0.0],
               [0.25, 0.5, 0.75, 1.25, 0.5, 9.0, 0.25],
               [0.5, 0.25, 0.0, 1.0, 1.5, 0.75, 0.5],
               [0.75, 1.0, -0.5, 0.5, 1.25, 1.0, 0.25],
               [1.0, 0.75, 0.5, 0.25, 0.0, -0.25, -0.5]], holes=[(2, 3)])
SMOOTH = _map([[0.125 * ((3 * i + 5 * j) % 11) for i in range(7)] for j in range(5)])   # no hole, no cut: every inside point has a difference
ZEROS = np.array([[-0.0, 0.0], [0.0, -0.0]], np.float32)


def _difference_cases():
    c = {}
    mix = lambda w, h, cell, seed: np.concatenate([lattice(w, h, cell), SPECIAL_POINTS, interior(700, w, h, cell, seed)])  # noqa: E731
    c["relief_7x5"] = DiffCase(mix(7, 5, 0.5, 1), RELIEF, DC.axis_frame(7, 5, cell=0.5), 2.0, False)
    c["relief_7x5_uncut"] = DiffCase(mix(7, 5, 0.5, 2), RELIEF, DC.axis_frame(7, 5, cell=0.5), INF, False)
    special = D.bits(RELIEF).copy()
    special[0, 0], special[4, 6] = 0x7F800000, 0x7FFFFFFF            # +inf and a NaN that is a value
    c["special_heights"] = DiffCase(mix(7, 5, 0.5, 3), special.view(np.float32), DC.axis_frame(7, 5, cell=0.5), INF, False)
    c["grid_1x1"] = DiffCase(np.concatenate([lattice(1, 1, 1.0), SPECIAL_POINTS]), _map([[0.75]]), DC.axis_frame(1, 1), INF, True)
    c["grid_1x5"] = DiffCase(np.concatenate([lattice(1, 5, 1.0), interior(50, 1, 5, 1.0, 4)]), _map([[0.5], [1.0], [0.25], [2.0], [-1.0]]),
                             DC.axis_frame(1, 5), INF, True)
    c["grid_2x2"] = DiffCase(np.concatenate([lattice(2, 2, 2.0), interior(400, 2, 2, 2.0, 5)]), _map([[0.5, 1.0], [0.25, 2.0]]),
                             DC.axis_frame(2, 2, cell=2.0), INF, False)
    c["grid_2x2_bc"] = DiffCase(np.concatenate([lattice(2, 2, 2.0), interior(400, 2, 2, 2.0, 6)]), _map([[0.5, 1.0], [1.25, 2.0]]),
                                DC.axis_frame(2, 2, cell=2.0), INF, False)
    # z = -0 needs every product -0: ez = (-0, -0, 1) and points with positive a and b
    zeros = np.concatenate([lattice(2, 2, 1.0, beyond=0.0, z=-0.0), lattice(2, 2, 1.0, beyond=0.0, z=0.0), interior(200, 2, 2, 1.0, 7)])
    c["signed_zeros"] = DiffCase(zeros, ZEROS, DC.axis_frame(2, 2, ez=(-0.0, -0.0, 1)), INF, False)
    skew = D.frame(cell=0.37, w=7, h=5, **DC.SKEW)
    cloud = np.concatenate([DC._random_cloud(300, 12, 7, 5, cell=0.37) - f32(3), SPECIAL_POINTS])
    abz = interior(900, 7, 5, 0.37, 8).astype(np.float64)   # (a, b, z) in the frame -> the world, through the inverse of the affine map
    skew_pts = (np.linalg.solve(np.stack([skew.ex, skew.ey, skew.ez]).astype(np.float64), abz.T).T + skew.origin.astype(np.float64)).astype(np.float32)
    c["skew_frame"] = DiffCase(np.concatenate([cloud, skew_pts]), RELIEF, skew, 2.0, False)
    every = interior(1000, 7, 5, 0.5, 9, origin=(2, 3, -1))
    for n in (0, 1, 63, 64, 65, 1000):
        c["n%d" % n] = DiffCase(every[:n], SMOOTH, DC.axis_frame(7, 5, cell=0.5, origin=(2, 3, -1)), INF, n == 0)
    return c


DIFFERENCE = _difference_cases()
_DIFF_REF = {}


def cells_of(name):
    c = DIFFERENCE[name]
    return M.mesh(c.height, 1, c.max_jump)[1]


def difference_reference(name, mesh):
    """-> float32 (n,): the reference's differences of a case in MESH (mesh True) or CELL mode"""
    if (name, mesh) not in _DIFF_REF:
        c = DIFFERENCE[name]
        _DIFF_REF[name, mesh] = A.difference(c.points, c.height, c.frame, cells_of(name) if mesh else None)
    return _DIFF_REF[name, mesh]


def plane(p, q, c0, w=7, h=5):
    """-> (height map z = p i + q j + c0, frame of cell 0.5, points on that plane at every quarter of a cell): dyadic coefficients"""
    jj, ii = np.mgrid[0:h, 0:w]
    height = (p * ii + q * jj + c0).astype(np.float32)
    pts = lattice(w, h, 0.5)
    uu, vv = pts[:, 0] / f32(0.5) - f32(0.5), pts[:, 1] / f32(0.5) - f32(0.5)
    pts[:, 2] = p * uu + q * vv + c0
    return height, DC.axis_frame(w, h, cell=0.5), pts


PLANES = {"b-c": (0.5, 0.25, 1.0), "a-d": (0.5, -0.25, 1.0)}   # |zb - zc| = |p - q| against |za - zd| = |p + q|

# ---- the statistics
StatsCase = namedtuple("StatsCase", "values center absolute quantiles")
EIGHT = (0, 10000, 5000, 5000, 2500, 6827, 9000, 9500)
FLT_MAX = float(np.finfo(np.float32).max)


def _values(n, seed, invalid=0.1, inf=0.02):
    rng = np.random.RandomState(seed)
    b = D.bits((rng.randn(n) * 3).astype(np.float32)).copy()
    b[rng.rand(n) < inf] = 0x7F800000
    b[rng.rand(n) < inf] = 0xFF800000
    b[rng.rand(n) < invalid] = D.INVALID_BITS
    return b.view(np.float32)


def _stats_cases():
    c = {}
    for n in (0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 1):
        c["n%d" % n] = StatsCase(_values(n, 50 + n), 0.0, False, (5000,))
        c["n%d/eight" % n] = StatsCase(_values(n, 50 + n), 0.25, True, EIGHT)
    c["all_equal"] = StatsCase(np.full(5000, 7.25, np.float32), 0.0, False, EIGHT)
    c["all_invalid"] = StatsCase(np.full(5000, INVALID, np.float32), 0.0, False, (5000, 0))
    c["only_inf"] = StatsCase(np.array([INF, -INF] * 300, np.float32), 0.0, False, (5000,))
    zeros = np.array([0.0, -0.0, -0.0, 0.0, -0.0, 0.0, 0.0], np.float32)
    c["signed_zeros"] = StatsCase(zeros, 0.0, False, (0, 4999, 5000, 10000))           # three -0 then four +0 in key order
    ties = np.repeat(np.array([1.0, 2.0, 3.0, 4.0], np.float32), [100, 300, 1, 200])
    c["ties"] = StatsCase(np.random.RandomState(3).permutation(ties), 0.0, False, (1666, 1667, 6650, 6667, 6684, 5000))
    neg = -np.abs(_values(3000, 4)) - f32(1)
    c["negative"] = StatsCase(neg, 0.0, False, EIGHT)
    c["negative/absolute"] = StatsCase(neg, 0.0, True, EIGHT)
    # a non-finite center is refused, so inf - inf cannot be asked for: the nearest a caller gets is inf - finite and a y that
    # overflows to inf, and both must leave the selection
    over = np.array([INF, -INF, FLT_MAX, -FLT_MAX, 1.0, -2.0, 3e38, -3e38, 0.5], np.float32)
    c["center_overflows"] = StatsCase(over, -FLT_MAX, False, (0, 5000, 10000))
    c["center_overflows/absolute"] = StatsCase(over, FLT_MAX, True, (0, 5000, 10000))
    c["min_max"] = StatsCase(_values(3001, 5), 0.0, False, (0, 10000))
    c["same_quantile_twice"] = StatsCase(_values(3001, 6), 0.0, False, (2500, 7500, 2500, 7500))
    rng = np.random.RandomState(7)
    c["random_bits"] = StatsCase(rng.randint(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32), 0.0, False, EIGHT)
    c["random_bits/absolute"] = StatsCase(c["random_bits"].values, 1.5, True, EIGHT)
    c["no_quantile"] = StatsCase(_values(5000, 8), 0.5, False, ())
    return c


STATS = _stats_cases()
BIG_N = 4096 * 4096 + 5   # the smallest n at which the tile sums need a second level
_STATS_REF = {}


def big_case():
    if "big" not in STATS:
        rng = np.random.RandomState(9)
        v = rng.standard_normal(BIG_N).astype(np.float32)
        v[::1001] = INVALID
        STATS["big"] = StatsCase(v, 0.0, False, (5000,))
    return STATS["big"]


def stats_reference(name):
    if name not in _STATS_REF:
        c = big_case() if name == "big" else STATS[name]
        _STATS_REF[name] = A.stats(c.values, c.center, c.absolute, c.quantiles)
    return _STATS_REF[name]


# ---- the rendered scene: tools/scene.py's PinholeRig(3, 192), the frame of tests/dsm_cases.py
_TRUTH = {}


def truth_map():
    """the scene's ground-truth height at the centre of every cell of dsm_cases.scene_frame(), float32 (h, w)"""
    if "map" not in _TRUTH:
        import torch
        s, fr = DC.scene(), DC.scene_frame()
        half = DC.SCENE_SIZE * s["rig"].gsd / 2.0
        jj, ii = np.mgrid[0:fr.h, 0:fr.w]
        a, b = (ii.ravel() + 0.5) * float(fr.cell) - half, (jj.ravel() + 0.5) * float(fr.cell) - half
        _TRUTH["map"] = s["scene"].height(torch.from_numpy(a).float(), torch.from_numpy(b).float()).numpy().astype(np.float32).reshape(fr.h, fr.w)
    return _TRUTH["map"]


def truth_cloud(view=0, step=2):
    """the ground-truth 3-D points of every step-th pixel of a view (float32 (n, 3), the cameras' frame)"""
    if ("cloud", view, step) not in _TRUTH:
        import torch
        s = DC.scene()
        ys, xs = np.mgrid[0:DC.SCENE_SIZE:step, 0:DC.SCENE_SIZE:step].astype(np.float64)
        p = s["rig"].ground_points(s["scene"], view, torch.from_numpy(xs.ravel()), torch.from_numpy(ys.ravel()))[0]
        _TRUTH["cloud", view, step] = p.numpy().astype(np.float32)
    return _TRUTH["cloud", view, step]


def quantised_scene(delta=0.0):
    """-> (points, height, frame): the truth map rounded to multiples of 2^-8 in an axis frame of cell 1 with ez = +Z, and a cloud
    at the quarter-cell lattice whose heights are the neighbouring cell's rounded truth plus a multiple of 2^-8, raised by delta.
    Every product and sum of MESH mode is then exact, so raising the cloud by a power of two raises every difference by it."""
    t = truth_map()
    height = (np.round(t.astype(np.float64) * 256) / 256).astype(np.float32)
    h, w = height.shape
    pts = lattice(w, h, 1.0, beyond=0.25)[::3].copy()
    i = np.clip(np.floor(pts[:, 0]).astype(np.int64) + 1, 0, w - 1)
    j = np.clip(np.floor(pts[:, 1]).astype(np.int64), 0, h - 1)
    noise = (np.arange(len(pts)) % 13 - 6) / 256.0
    pts[:, 2] = height[j, i] + noise + delta
    return pts.astype(np.float32), height, DC.axis_frame(w, h)
