"""The surface-model cases: clouds and frames for ssrlcv_hip_dsm_rasterize, map sets for ssrlcv_hip_dsm_fuse, height maps for
ssrlcv_hip_dsm_points, and the three-pair scene of the end-to-end test.  Shared by tests/test_dsm_cases.py (which proves on the
numpy reference alone that every case exercises what it claims) and tests/test_gpu_dsm.py (which holds the kernels to that
reference).  Every reference result is computed once, shared and never modified."""
import os
import sys
from collections import namedtuple

import numpy as np

import helpers as H
import dsm_ref as D

sys.path.insert(0, os.path.join(H.ROOT, "tools"))

f32 = np.float32
NAN, INF = float("nan"), float("inf")
TINY = np.array([1], np.uint32).view(np.float32)[0]   # the smallest denormal: -TINY is the largest float below 0

X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def axis_frame(w, h, cell=1.0, origin=(0, 0, 0), ex=X, ey=Y, ez=Z):
    return D.frame(origin, ex, ey, ez, cell, w, h)


SKEW = dict(origin=(-3.3, 2.1, 0.7), ex=(1, 0.25, 0), ey=(0.1, 1, 0.05), ez=(0.2, -0.1, 1))   # an affine map, not orthonormal


def _pts(*rows):
    return np.array(rows, np.float32).reshape(-1, 3)


def _random_cloud(n, seed, w, h, cell=1.0, spill=0.15, levels=None):
    """n points over a w x h grid of `cell`, `spill` of the extent outside on every side; heights continuous, or drawn from
    `levels` values so that they tie"""
    rng = np.random.RandomState(seed)
    p = np.empty((n, 3), np.float32)
    p[:, 0] = (rng.rand(n) * (1 + 2 * spill) - spill) * w * cell
    p[:, 1] = (rng.rand(n) * (1 + 2 * spill) - spill) * h * cell
    p[:, 2] = rng.randn(n) * 3 if levels is None else rng.randint(0, levels, n) * 0.5 - 1
    if w * h > 1:   # the middle cell stays empty however dense the cloud: its points move far outside
        p[(np.floor(p[:, 0] / f32(cell)) == w // 2) & (np.floor(p[:, 1] / f32(cell)) == h // 2), 0] = -5 * w * cell
    return p


def _in_cell(n, i, j, heights):
    """n points at the centre of cell (i, j) of an axis frame of cell 1"""
    p = np.empty((n, 3), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = i + 0.5, j + 0.5, heights
    return p


def _runs(n, length, shift, cells_w):
    """point t lies in cell ((t + shift) // length) % cells_w of a one-row grid: runs of `length` equal cells in index order"""
    rng = np.random.RandomState(n + length)
    c = ((np.arange(n) + shift) // length) % cells_w
    return np.stack([c + 0.25, np.full(n, 0.5), rng.randn(n)], 1).astype(np.float32)


def _borders():
    """cell 0.5 on a 6 x 4 grid: every u and v an exact integer, the far edge u == w and v == h included"""
    us, vs = np.meshgrid(np.arange(-1, 8), np.arange(-1, 6))
    n = us.size
    return np.stack([us.ravel() * 0.5, vs.ravel() * 0.5, 1 + np.arange(n) * 0.125], 1).astype(np.float32)


Case = namedtuple("Case", "points frame exempt")   # exempt: the case says it has no occupied or no empty cell

BASE_W, BASE_H = 33, 17


def base_cloud():
    """20 000 points with distinct heights over a 33 x 17 grid: the cloud of the order cases"""
    p = _random_cloud(20000, 5, BASE_W, BASE_H)
    p[:, 2] = np.random.RandomState(6).permutation(20000).astype(np.float32) * 0.25 - 2000   # distinct, exact
    return p


def order_of(kind):
    """the permutation of the base cloud's indices for an order case: new index t holds old point order[t]"""
    cell = D.locate(base_cloud(), axis_frame(BASE_W, BASE_H))["cell"]
    if kind == "sorted":
        return np.argsort(cell, kind="stable")
    if kind == "reversed":
        return np.arange(len(cell))[::-1].copy()
    return np.random.RandomState(7).permutation(len(cell))


def _rasterize_cases():
    c = {}
    for n in (0, 1, 63, 64, 65, 257):
        c["n%d" % n] = Case(_pts((2.5, 3.5, 1.25)) if n == 1 else _random_cloud(n, 100 + n, 9, 7), axis_frame(9, 7), n == 0)
    c["grid_1x1"] = Case(_random_cloud(50, 1, 1, 1), axis_frame(1, 1), True)
    c["grid_w0"] = Case(_random_cloud(50, 2, 4, 4), axis_frame(0, 4), True)        # no cell at all
    c["grid_h0"] = Case(_random_cloud(50, 3, 4, 4), axis_frame(4, 0), True)
    c["grid_1x97"] = Case(_random_cloud(300, 4, 1, 97), axis_frame(1, 97), False)
    c["grid_97x1"] = Case(_random_cloud(300, 5, 97, 1), axis_frame(97, 1), False)
    c["one_cell_distinct"] = Case(_in_cell(100000, 3, 2, np.random.RandomState(8).permutation(100000) * 0.5 - 20000), axis_frame(5, 4), False)
    c["one_cell_equal"] = Case(_in_cell(100000, 3, 2, 7.25), axis_frame(5, 4), False)
    c["equal_heights"] = Case(_random_cloud(3000, 9, 9, 7, levels=3), axis_frame(9, 7), False)
    c["signed_zeros"] = Case(_pts((0.5, 0.5, 0.0), (0.5, 0.5, -0.0), (0.5, 0.5, 0.0), (0.5, 0.5, -0.0), (1.5, 0.5, -0.0), (1.5, 0.5, 0.0)),
                             axis_frame(3, 1, ez=(-0.0, -0.0, 1)), False)   # z = -0 needs every product -0
    neg = _random_cloud(2000, 10, 9, 7)
    neg[:, 2] = -np.abs(neg[:, 2]) - 1
    c["negative_heights"] = Case(neg, axis_frame(9, 7), False)
    den = f32(1e-40)                                                                  # a denormal cell: p = k cell exactly
    k = np.random.RandomState(11).randint(-2, 9, size=(400, 2)).astype(np.float32)
    c["denormal_cell"] = Case(np.stack([k[:, 0] * den, k[:, 1] * den, np.arange(400, dtype=np.float32)], 1), axis_frame(6, 4, cell=den), False)
    c["borders"] = Case(_borders(), axis_frame(6, 4, cell=0.5), True)
    # a = -0 (every product -0: inside cell 0) and a = the largest float below 0 (floor -1: outside)
    c["minus_zero_a"] = Case(_pts((-0.0, 0.5, 2.0), (0.5, 1.5, 1.0)), axis_frame(2, 3, ex=(1, -0.0, -0.0)), False)
    c["just_below_zero_a"] = Case(_pts((-TINY, 0.5, 2.0), (0.5, 1.5, 1.0)), axis_frame(2, 3), False)
    c["huge"] = Case(_pts((1e30, 0.5, 1), (-1e30, 0.5, 2), (0.5, 1e30, 3), (0.5, -1e30, 4), (0.5, 0.5, 1e30), (1.5, 0.5, -1e30), (1e30, 1e30, 1e30)),
                     axis_frame(3, 2), False)
    c["nan_inf"] = Case(_pts((NAN, 0.5, 1), (0.5, NAN, 1), (0.5, 0.5, NAN), (INF, 0.5, 1), (0.5, -INF, 1), (0.5, 0.5, INF), (0.5, 0.5, -INF),
                             (1.5, 0.5, 3)), axis_frame(3, 2), False)
    c["zero_points"] = Case(_pts((0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (0.0, -0.0, -0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)),
                            axis_frame(3, 3, origin=(-1, -1, 0)), False)
    c["z_overflows"] = Case(_pts((0.5, 0.5, 2.0), (0.5, 0.5, 0.5), (1.5, 0.5, -2.0)), axis_frame(3, 1, ez=(0, 0, 3e38)), False)
    c["skew_frame"] = Case(_random_cloud(5000, 12, 20, 20) - f32(3), D.frame(cell=0.37, w=31, h=23, **SKEW), False)
    c["runs_cross_waves"] = Case(_runs(1100, 10, 3, 37), axis_frame(40, 1), False)    # 10 does not divide 64 or 256: runs straddle both
    c["runs_longer_than_a_wave"] = Case(_runs(1100, 150, 20, 5), axis_frame(6, 1), False)
    c["large"] = Case(_random_cloud(200000, 13, 257, 131), axis_frame(257, 131), False)
    c["sparse"] = Case(_random_cloud(4000, 14, 257, 131), axis_frame(257, 131), False)
    base = base_cloud()
    c["order_given"] = Case(base, axis_frame(BASE_W, BASE_H), False)
    for kind in ("sorted", "reversed", "shuffled"):
        c["order_" + kind] = Case(base[order_of(kind)], axis_frame(BASE_W, BASE_H), False)
    return c


RASTERIZE = _rasterize_cases()
_RASTER_REF = {}


def rasterize_reference(name, rule):
    if (name, rule) not in _RASTER_REF:
        c = RASTERIZE[name]
        _RASTER_REF[name, rule] = D.rasterize(c.points, c.frame, rule)
    return _RASTER_REF[name, rule]


# ---- fuse
FuseCase = namedtuple("FuseCase", "maps min_views max_spread rule")
FUSE_SIZES = ((1, 1), (63, 5), (257, 131))
SPECIALS = np.array([0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x7FFFFFFF, 0xFFC00000], np.uint32)   # +-inf, +-0, two other NaNs


def fuse_maps(m, w, h, seed):
    """m maps of multiples of 0.25 in -2 .. 2 (every difference exact), 35 % invalid, a few infinities, zeros of both signs and
    NaNs that are values; cell c < m + 1 of the first row holds exactly c valid entries when the map has the room"""
    rng = np.random.RandomState(seed)
    vals = (rng.randint(-8, 9, size=(m, h, w)) * 0.25).astype(np.float32)
    b = D.bits(vals).copy()
    special = rng.rand(m, h, w) < 0.04
    b[special] = SPECIALS[rng.randint(0, len(SPECIALS), int(special.sum()))]
    b[rng.rand(m, h, w) < 0.35] = D.INVALID_BITS
    if w * h >= m + 1:
        flat = b.reshape(m, -1)
        for c in range(m + 1):
            flat[:, c] = D.INVALID_BITS
            flat[:c, c] = D.bits(f32(0.25) * np.arange(c, dtype=np.float32))
    return [x.view(np.float32) for x in b]


def _fuse_cases():
    c = {}
    for (w, h) in FUSE_SIZES:
        for m in (1, 2, 3, 8):
            maps = fuse_maps(m, w, h, 1000 * m + w)
            for rule in (D.FUSE_MIN, D.FUSE_MEDIAN, D.FUSE_MAX):
                c["%dx%d/m%d/rule%d/spread1" % (w, h, m, rule)] = FuseCase(maps, 1, 1.0, rule)   # 1.0 is hi - lo exactly in some cells
            c["%dx%d/m%d/all_views" % (w, h, m)] = FuseCase(maps, m, INF, D.FUSE_MEDIAN)
            c["%dx%d/m%d/spread0" % (w, h, m)] = FuseCase(maps, 1, 0.0, D.FUSE_MAX)
            c["%dx%d/m%d/spread_inf" % (w, h, m)] = FuseCase(maps, min(2, m), INF, D.FUSE_MIN)
    w, h = 63, 5
    hole = np.full((h, w), D.INVALID_BITS, np.uint32).view(np.float32)
    c["all_invalid"] = FuseCase([hole, hole.copy(), hole.copy()], 1, INF, D.FUSE_MEDIAN)
    maps = fuse_maps(3, w, h, 77)
    c["same_map_twice"] = FuseCase([maps[0], maps[1], maps[0], maps[0]], 2, 0.5, D.FUSE_MEDIAN)   # identity decides: the GPU test passes one pointer
    return c


FUSE = _fuse_cases()
_FUSE_REF = {}


def fuse_reference(name):
    if name not in _FUSE_REF:
        c = FUSE[name]
        _FUSE_REF[name] = D.fuse(c.maps, c.min_views, c.max_spread, c.rule)
    return _FUSE_REF[name]


# ---- points
def height_map(w, h, seed, holes=0.3):
    rng = np.random.RandomState(seed)
    b = D.bits((rng.randn(h, w) * 2).astype(np.float32)).copy()
    b[rng.rand(h, w) < holes] = D.INVALID_BITS
    return b.view(np.float32)


POINTS = {
    "1x1": (height_map(1, 1, 1, 0.0), axis_frame(1, 1, cell=0.5)),
    "63x5_skew": (height_map(63, 5, 2), D.frame(cell=0.37, w=63, h=5, **SKEW)),
    "257x131": (height_map(257, 131, 3), axis_frame(257, 131, cell=0.125, origin=(10, -20, 3))),
    "all_holes": (height_map(9, 7, 4, 1.1), axis_frame(9, 7)),
}

# x east, y south, height up: (ex, ey, -ez) right-handed
SOUTH = (0, -1, 0)


def tilted_plane(w=17, h=9):
    """-> (height map, frame): z = 0.3 i - 0.2 j + 1 with two holes"""
    jj, ii = np.mgrid[0:h, 0:w]
    z = (0.3 * ii - 0.2 * jj + 1).astype(np.float32)
    b = D.bits(z).copy()
    b[2, 3] = b[5, 11] = D.INVALID_BITS
    return b.view(np.float32), axis_frame(w, h, cell=0.5, origin=(2, 3, -1), ey=SOUTH)


# ---- the scene: three pairs of tools/scene.py's PinholeRig(3, 192)
SCENE_SIZE = 192
PAIRS = ((0, 2), (1, 0), (1, 2))   # (0, 1) does not rectify in that order (camera 1 lies to the left of camera 0): the same pair as (1, 0)
_SCENE = {}


def scene():
    """-> dict: rig, scene, images (uint8 numpy a view, rendered on the CPU whatever the machine), cams"""
    if not _SCENE:
        import torch
        import scene as S
        rig = S.PinholeRig(3, SCENE_SIZE)
        sc = S.Scene(SCENE_SIZE, rig.gsd, torch.device("cpu"))
        _SCENE.update(rig=rig, scene=sc, images=[rig.render(sc, v).numpy() for v in range(3)], cams=rig.cameras)
    return _SCENE


def scene_frame():
    """the ground grid from the rig itself: ex = e1, ey = e2, ez = -down, origin at the patch centre minus half the extent,
    cells of two ground pixels"""
    rig = scene()["rig"]
    half = SCENE_SIZE * rig.gsd / 2.0
    return D.frame(rig.centre - half * rig.e1 - half * rig.e2, rig.e1, rig.e2, -rig.down, 2 * rig.gsd, SCENE_SIZE // 2, SCENE_SIZE // 2)


def pair_range(views):
    """(min_disparity, num_disparities, rect) of a pair: the true disparities of the rectified left view's pixels whose source
    lies inside the left image, two pixels wider on either side (tests/rectify_cases.py truth(), for any pair)"""
    import torch
    import rectify_cases as RC
    from ssrlcv_amd import capi
    s = scene()
    a, b = views
    rect = capi.rectify_cameras(s["cams"][a], s["cams"][b])
    n = SCENE_SIZE
    ys, xs = np.mgrid[0:n, 0:n].astype(np.float64)
    sx, sy = RC.eval64(rect["Hl"], xs.ravel(), ys.ravel())
    seen = (sx >= 0) & (sx <= n - 1) & (sy >= 0) & (sy <= n - 1)
    ground = s["rig"].ground_points(s["scene"], a, torch.from_numpy(sx), torch.from_numpy(sy))[0].numpy()
    u, v, _ = RC.project(s["cams"][b], s["rig"].M[b], ground)
    xr, _ = RC.eval64(rect["Gr"], u, v)
    d = xs.ravel() - xr
    lo, hi = int(np.floor(d[seen].min())) - 2, int(np.ceil(d[seen].max())) + 2
    return lo, hi - lo + 1, rect
