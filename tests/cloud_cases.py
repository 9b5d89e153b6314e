"""Edge cases of the point-cloud stage (ssrlcv_hip_knn / _neighbor_distance_filter / _point_normals), numpy only, seeded and
small.  Shared by tests/test_cloud_cases.py (which proves on the reference alone that the cases are what they claim) and
tests/test_gpu_cloud_edges.py (which holds csrc/cloud.hip to cloud_ref.knn_brute and the float64 reference on them).

The sizes sit on the constants of csrc/cloud.hip: TopK<8 / 16 / 32> with a run-time k, 256-thread blocks, far blocks of 64
queries whose 8 waves take 256-point tiles (2048 points a round), 512 fixed statistic partitions, compaction tiles of 2048
points run by at most 2048 blocks, the volume / sheet / line / point branches of the automatic cell size, h raised to
extent / 2^20, and the scales at which the float32 products of d2 go subnormal, vanish or overflow."""
from collections import namedtuple

import numpy as np

import cloud_ref as R

NONE = 0xFFFFFFFF
ECEF_OFFSET = np.array([-1500.0, 4500.0, 4250.0])      # |.| = 6369: float32 spacing 2^-13 / 2^-11 / 2^-11
SCALE_EXPONENTS = (-80, -70, -64, -60, -40, 0, 40, 62)

KnnCase = namedtuple("KnnCase", "p k cells all_far one_cell")   # cells: the cell sizes to run (0 = automatic); one_cell: the
# one among them that puts the whole cloud into a single cell
FilterCase = namedtuple("FilterCase", "d2 k sigma keep exact")  # keep: the mask the construction promises (None: reference's)
NormalCase = namedtuple("NormalCase", "p nbr k vp zero_rows line")


def cube(n, seed=1):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def scaled(p, e):
    """p times 2^e, exactly (no value of the unit cube leaves the normal float32 range for |e| <= 80)"""
    return (p * np.float32(2.0) ** np.float32(e)).astype(np.float32)


def _cells(p, k, auto_only=False):
    """automatic, tiny (many queries leave the grid), about right, huge (one cell) for the extent of p's finite points"""
    if auto_only:
        return (0.0,)
    f = p[R.finite_mask(p)].astype(np.float64)
    ext = float((f.max(0) - f.min(0)).max()) if len(f) else 0.0
    if not ext > 0:
        ext = 1.0
    right = ext * (k / max(len(f), 1)) ** (1.0 / 3.0)
    return (0.0, float(np.float32(ext * 2.0 ** -12)), float(np.float32(right)), float(np.float32(ext * 64.0)))


def _knn(p, k, cells=None, all_far=False, more_cells=()):
    p = np.ascontiguousarray(p, np.float32)
    auto = _cells(p, k)
    return KnnCase(p, k, tuple(more_cells) + auto if cells is None else tuple(cells), all_far, auto[3] if cells is None else None)


ALL_FAR_CELL = 2.0 ** -19   # unit cube: above extent / 2^20 (not raised), and four cells are far below any spacing


def knn_cases():
    """name -> KnnCase"""
    c = {}
    c["n2_k1"] = _knn(cube(2, 20), 1)
    for k in (1, 8, 9, 16, 17, 32):
        c["n_is_k_plus_1_k%d" % k] = _knn(cube(k + 1, 21 + k), k)
    for n in (255, 256, 257):
        for k in (8, 16, 32):
            c["block_edges_n%d_k%d" % (n, k)] = _knn(cube(n, n), k)
    for n in (63, 64, 65, 257, 2047, 2048, 2049):
        for k in (5, 16, 32):
            c["all_far_n%d_k%d" % (n, k)] = _knn(cube(n, 100 + n), k, cells=(ALL_FAR_CELL,), all_far=True)
    few = cube(20, 30)
    few[[1, 4, 9], 0] = np.nan
    few[[12, 13], 2] = np.inf
    few[19, 1] = -np.inf
    c["few_finite_13_others"] = _knn(few, 16)
    c["few_finite_none"] = _knn(np.full((20, 3), np.nan, np.float32), 16)
    one = np.full((20, 3), np.inf, np.float32)
    one[7] = (0.25, -3.0, 1e3)
    c["few_finite_one"] = _knn(one, 16)
    c["coincident"] = _knn(np.tile(np.float32([0.3, -7.25, 1e3]), (300, 1)), 16)
    rng = np.random.default_rng(40)
    plane = rng.random((1200, 3)).astype(np.float32)
    plane[:, 2] = 0.5
    c["plane"] = _knn(plane, 16)
    line = np.zeros((700, 3), np.float32)
    line[:, 0], line[:, 1], line[:, 2] = rng.random(700) * 50, 2.0, -1.0
    c["line"] = _knn(line, 16)
    lattice = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    c["lattice_patch"] = _knn(lattice, 26, more_cells=(1.0, 2.0))
    # h = 2 on the integer lattice: a query at an odd coordinate has its cell's far faces at distance exactly 1, where the
    # next cells' nearest points sit; its own cell holds 3 points at d2 = 1, the k-th key EQUAL to the bound, while lower
    # indices at d2 = 1 wait outside.  The ring stop must be strict.
    c["lattice_ties_k3"] = _knn(lattice, 3, more_cells=(2.0,))
    out = np.concatenate([cube(1500, 41) * np.float32(1e-3), np.float32([[4e3, 0, 0]])])
    c["outlier_range_auto"] = _knn(out, 16, cells=(0.0,))
    c["outlier_range_raised"] = _knn(out, 16, cells=(1e-5,))        # 1e-5 < 4e3 / 2^20 = 3.8e-3
    ecef = (ECEF_OFFSET + cube(2000, 42).astype(np.float64) * 0.01).astype(np.float32)
    c["ecef_quantised"] = _knn(ecef, 16)
    for e in SCALE_EXPONENTS:
        c["scale_sweep_e%+d" % e] = _knn(scaled(cube(1500, 1), e), 16)
    c["scale_sweep_overflow"] = _knn(scaled(cube(20, 43), 64), 16)
    return c


# ---------------------------------------------------------------- filter: hand-made dist2
def filter_points(n):
    """any points and normals do: the filter only compacts them"""
    i = np.arange(3 * n, dtype=np.float32).reshape(n, 3)   # exact below 2^24, merely distinct-ish above: compared by index
    return i * np.float32(0.5) - np.float32(7.0), -i


def _two_level(n, k, low_rows):
    """m = 1 on low_rows, 2 elsewhere: with sigma = 0 the threshold is the mean, strictly between (both levels present)"""
    d2 = np.full((n, k), 4.0, np.float32)
    d2[low_rows] = 1.0
    keep = np.zeros(n, bool)
    keep[low_rows] = True
    return d2, keep


def _random_d2(n, k, seed):
    """spread d2 (m spans two decades), every 23rd row with an empty tail (+inf, as k-NN writes it)"""
    rng = np.random.default_rng(seed)
    d2 = np.sort((10.0 ** rng.uniform(-2, 2, (n, 1)) * rng.uniform(0.5, 1.5, (n, k))).astype(np.float32), 1)
    if n > 2:
        d2[5::23, k - 1] = np.inf
    return d2


FILTER_SIZES = (2, 17, 511, 512, 513, 2047, 2048, 2049, 4097)
FILTER_SIGMAS = (0.0, 2.0, -10.0, 1e6)
BIG_N = 2048 * 2048 + 2049   # the smallest n at which one block of k_filter_compact takes a second tile


def filter_cases():
    """name -> FilterCase (the 4.2 M-point case is built by filter_big(): it is large)"""
    c = {}
    for n in FILTER_SIZES:
        k = 1 if n == 2 else 16
        for s in FILTER_SIGMAS:
            d2 = _random_d2(n, k, 1000 + n)
            keep = np.zeros(n, bool) if s == -10.0 else np.isfinite(d2).all(1) if s == 1e6 else None
            c["n%d_sigma%g" % (n, s)] = FilterCase(d2, k, s, keep, False)
    n = 4097
    d2, keep = _two_level(n, 2, [0])
    c["first_only"] = FilterCase(d2, 2, 0.0, keep, False)
    d2, keep = _two_level(n, 2, [n - 1])
    c["last_only"] = FilterCase(d2, 2, 0.0, keep, False)
    d2, keep = _two_level(n, 2, np.arange(0, n, 2))
    c["alternating"] = FilterCase(d2, 2, 0.0, keep, False)
    d2, keep = _two_level(3 * 2048, 1, np.r_[0:2048, 4096:6144])
    c["tile_rejected"] = FilterCase(d2, 1, 0.0, keep, False)
    # every m equal: std is exactly 0, t = mu = m, and `<=` keeps both whatever sigma is
    for s in (0.0, -10.0):
        c["all_equal_sigma%g" % s] = FilterCase(np.full((2, 1), 0.25, np.float32), 1, s, np.ones(2, bool), True)
    nonfin = np.full((600, 16), np.inf, np.float32)
    nonfin[::7, 3] = np.nan
    nonfin[1::7, :15] = 1.0         # finite head, empty tail: m is still +inf
    c["all_nonfinite"] = FilterCase(nonfin, 16, 2.0, np.zeros(600, bool), False)
    rng = np.random.default_rng(77)
    ext = rng.choice(np.float32([0.0, 1e-45, 3e-42, 1.1754942e-38, 1.1754944e-38, 1e-30, 1.0, 1e30, 3e38]), (1000, 1))
    c["extremes_sigma0"] = FilterCase(ext.astype(np.float32), 1, 0.0, None, False)
    c["extremes_sigma2"] = FilterCase(ext.astype(np.float32), 1, 2.0, None, False)
    return c


def filter_big():
    d2 = (np.random.default_rng(78).random((BIG_N, 1), np.float32) + np.float32(0.01))
    d2[123456::99991] = np.inf
    return FilterCase(d2, 1, 0.0, None, False)


# ---------------------------------------------------------------- normals
def quantised_cube(n, seed):
    """the unit cube on a 2^-10 lattice: adding ECEF_OFFSET or scaling by 2^+-60 is then exact in float32, so the
    differences the covariance is made of are the same numbers (times the scale) and the normals must agree"""
    return (np.random.default_rng(seed).integers(0, 1024, (n, 3)) / 1024.0).astype(np.float32)


def plane_cloud():
    p = (np.random.default_rng(50).integers(0, 4096, (400, 3)) / 256.0).astype(np.float32)
    p[:, 2] = 2.5
    return p


LINE_DIR = np.array([1.0, 2.0, -2.0]) / 3.0


def _table(p, k):
    return R.knn_brute(p, k)[0]


def normal_cases():
    """name -> NormalCase; nbr tables come from cloud_ref.knn_brute or are hand-made"""
    c = {}
    for n in (255, 256, 257):
        p = cube(n, 60 + n)
        for k in (1, 2, 16, 32):
            c["cube_n%d_k%d" % (n, k)] = NormalCase(p, _table(p, k), k, (0.5, 0.5, 9.0), None, None)
    t, _, up = R.terrain_cloud(3000, seed=6)
    tvp = tuple((t.astype(np.float64).mean(0) + 400.0 * up).astype(np.float32))
    for k in (2, 16, 32):
        c["terrain_k%d" % k] = NormalCase(t, _table(t, k), k, tvp, None, None)
    pl = plane_cloud()
    nb = _table(pl, 8)
    c["plane_vp_above"] = NormalCase(pl, nb, 8, (8.0, 8.0, 12.5), None, None)
    c["plane_vp_below"] = NormalCase(pl, nb, 8, (8.0, 8.0, -7.5), None, None)
    c["plane_vp_inside"] = NormalCase(pl, nb, 8, (40.0, -3.0, 2.5), None, None)
    # hand-made tables.  Exactly collinear points (integer multiples of (1, 2, -2)): any neighbour table is collinear
    rng = np.random.default_rng(51)
    tt = rng.permutation(400)[:120].astype(np.float64)
    ln = np.outer(tt, [1.0, 2.0, -2.0]).astype(np.float32)
    nb = np.stack([rng.permutation(119)[:8] for _ in range(120)]).astype(np.uint32)
    nb += (nb >= np.arange(120)[:, None]).astype(np.uint32)      # never the row itself (it would still be collinear)
    c["collinear_table"] = NormalCase(ln, nb, 8, (3.0, 50.0, 7.0), None, LINE_DIR)
    two = np.float32([[0.0, 0.0, 0.0], [3.0, 4.0, 12.0]])
    c["k1_table"] = NormalCase(two, np.uint32([[1], [0]]), 1, (1.0, 5.0, -2.0), None, np.array([3.0, 4.0, 12.0]) / 13.0)
    co = cube(40, 52)
    co[10:20] = co[10]                                           # ten copies of one point
    nb = _table(co, 4)
    nb[10:20] = np.uint32([[11, 12, 13, 14]] * 4 + [[10, 11, 12, 13]] * 6)
    c["coincident_table"] = NormalCase(co, nb, 4, (0.5, 0.5, 9.0), np.arange(10, 20), None)
    # rows that must give (0, 0, 0): UINT32_MAX in the table, exactly n in the table, a non-finite centre
    z = cube(300, 53)
    z[[17, 255, 299], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    nb = _table(z, 16)
    nb[3, 15] = NONE
    nb[256, 0] = 300
    nb[298, 7] = NONE
    zero = np.nonzero(~R.finite_mask(z) | (nb >= 300).any(1))[0]
    c["zero_rows"] = NormalCase(z, nb, 16, (0.5, 0.5, 9.0), zero, None)
    # scale and offset invariance: one table, four exact images of one cloud
    q = quantised_cube(256, 54)
    nb = _table(q, 16)
    vp = np.array([0.5, 0.25, 9.0])
    c["invariance_base"] = NormalCase(q, nb, 16, tuple(vp), None, None)
    c["invariance_2^-60"] = NormalCase(scaled(q, -60), nb, 16, tuple(vp * 2.0 ** -60), None, None)
    c["invariance_2^+60"] = NormalCase(scaled(q, 60), nb, 16, tuple(vp * 2.0 ** 60), None, None)
    c["invariance_ecef"] = NormalCase((q.astype(np.float64) + ECEF_OFFSET).astype(np.float32), nb, 16,
                                      tuple(vp + ECEF_OFFSET), None, None)
    return c


INVARIANT = ("invariance_2^-60", "invariance_2^+60", "invariance_ecef")
# the keys of normal_cases(), for parametrising without building the cases at collection time
NORMAL_NAMES = tuple(["cube_n%d_k%d" % (n, k) for n in (255, 256, 257) for k in (1, 2, 16, 32)] +
                     ["terrain_k%d" % k for k in (2, 16, 32)] +
                     ["plane_vp_above", "plane_vp_below", "plane_vp_inside", "collinear_table", "k1_table", "coincident_table",
                      "zero_rows", "invariance_base"] + list(INVARIANT))


def angle_bound(k, gap):
    """the normal's angle to the eigh reference: the float32 rounding of the output (each component within 2^-25, so the
    vector within sqrt(3) 2^-25 < 4 2^-24 with the renormalisation) plus both float64 solvers' perturbation of a
    (k + 1)-term covariance over the relative eigengap"""
    return 4.0 * 2.0 ** -24 + 64.0 * (k + 1) * 2.0 ** -53 / gap


# Eigen-residual of a float32 normal n = e + d against the float64 covariance C, e the unit eigenvector of l_min:
# |d| <= sqrt(3) 2^-25 (three components, each rounded to within 2^-25).  To first order
#   C n - (n'C n) n = (C - l_min) d - 2 l_min (e'd) e,   norm <= (l_max - l_min) |d| + 2 l_min |d| <= 2 l_max |d|
#   n'C n - l_min   = 2 l_min e'd + d'(C - l_min) d      <= 2 l_max |d|
# so both are within sqrt(3) 2^-24 l_max; 2 covers the second-order terms and the float64 solver (~1e-15 l_max).
RESIDUAL_C = 2.0
