"""The surface-registration cases: clouds, poses, reference maps, frames and gates for ssrlcv_hip_register_terms and
ssrlcv_hip_transform_points, and the displaced scene of the end-to-end tests.  Shared by tests/test_register_cases.py (which proves
on the numpy reference alone that every case exercises what it claims), tests/test_register_host.py (the host steps on the
reference's records) and tests/test_gpu_register.py (which holds the kernels to that reference).  Every reference result is computed
once, shared and never modified."""
from collections import namedtuple

import numpy as np

import accuracy_cases as AC
import dsm_cases as DC
import mesh_ref as M
import register_ref as R

f32 = np.float32
INF = float("inf")

TermsCase = namedtuple("TermsCase", "points pose height frame max_jump center gate")

IDENTITY = R.pose()
RIGID = R.pose(R.rotation((0.01, -0.02, 0.03)), (0.05, -0.04, 0.03), pivot=(1.5, 1.0, 0.5))
SIMILARITY = R.pose(1.03 * R.rotation((-0.02, 0.01, 0.015)), (-0.03, 0.06, -0.02), pivot=(1.75, 1.25, 0.25))
HALF_OFF = R.pose(R.rotation((0, 0, 0.02)), (1.75, 0.0, 0.0), pivot=(0, 0, 0))    # 3.5 of 7 cells of 0.5 to the right
POSES = {"identity": IDENTITY, "rigid": RIGID, "similarity": SIMILARITY, "half_off": HALF_OFF}
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 1)


def _cases():
    c = {}
    d = AC.DIFFERENCE
    for name in ("grid_2x2", "grid_2x2_bc"):
        c[name] = TermsCase(d[name].points, R.pose(pivot=(2, 2, 1)), d[name].height, d[name].frame, d[name].max_jump, 0.0, INF)
    for pose_name, g in sorted(POSES.items()):
        c["relief/" + pose_name] = TermsCase(d["relief_7x5"].points, g, d["relief_7x5"].height, d["relief_7x5"].frame, 2.0, 0.0, INF)
        c["relief/%s/gated" % pose_name] = TermsCase(d["relief_7x5"].points, g, d["relief_7x5"].height, d["relief_7x5"].frame, 2.0, 0.25, 0.75)
    c["relief_uncut"] = TermsCase(d["relief_7x5_uncut"].points, RIGID, d["relief_7x5_uncut"].height, d["relief_7x5_uncut"].frame, INF, 0.0, 2.0)
    c["special_heights"] = TermsCase(d["special_heights"].points, IDENTITY, d["special_heights"].height, d["special_heights"].frame, INF, 0.0, INF)
    c["grid_1x5"] = TermsCase(d["grid_1x5"].points, IDENTITY, d["grid_1x5"].height, d["grid_1x5"].frame, INF, 0.0, INF)
    c["signed_zeros"] = TermsCase(d["signed_zeros"].points, R.pose(pivot=(1, 1, 0)), d["signed_zeros"].height, d["signed_zeros"].frame, INF, 0.0, INF)
    c["skew_frame"] = TermsCase(d["skew_frame"].points, R.pose(pivot=(-2, 3, 1)), d["skew_frame"].height, d["skew_frame"].frame, 2.0, 0.0, INF)
    c["skew_frame/gated"] = TermsCase(d["skew_frame"].points, R.pose(R.rotation((0.01, 0.01, -0.01)), (0.02, 0.01, 0.0), pivot=(-2, 3, 1)),
                                      d["skew_frame"].height, d["skew_frame"].frame, 2.0, -0.1, 1.0)
    # a difference exists but the slope over the cell overflows: G, N and J are not finite and no point is used
    steep = np.array([[1e38, -1e38], [-1e38, 1e38]], np.float32)
    c["overflowing_slopes"] = TermsCase(AC.interior(300, 2, 2, 0.5, 24), IDENTITY, steep, DC.axis_frame(2, 2, cell=0.5), INF, 0.0, INF)
    every = AC.interior(SIZES[-1], 7, 5, 0.5, 21, origin=(2, 3, -1))
    g = R.pose(R.rotation((0.01, -0.02, 0.03)), (0.05, -0.04, 0.03), pivot=(3.5, 4.0, -0.5))
    g["m"][3::4] += (np.eye(3) - np.asarray(g["m"], np.float64).reshape(3, 4)[:, :3]) @ np.array([3.75, 4.25, -1.0])   # rotate about the grid's middle
    for n in SIZES:
        c["n%d" % n] = TermsCase(every[:n], g, AC.SMOOTH, DC.axis_frame(7, 5, cell=0.5, origin=(2, 3, -1)), INF, 0.125, 1.0)
    return c


TERMS = _cases()
BIG_N = 4096 * 4096 + 5      # the smallest n at which the tile sums need a second level
BIG_TILES = (0, 2000, 4096)  # the tiles that hold usable points: the first, a middle one and the last (5 points)
_REF = {}


def big_case():
    """n = 4096 * 4096 + 5: every point is (0, 0, 0), skipped, except those of three tiles"""
    if "big" not in TERMS:
        base = TERMS["n4097"]
        p = np.zeros((BIG_N, 3), np.float32)
        src = AC.interior(3 * 4096, 7, 5, 0.5, 22, origin=(2, 3, -1))
        for k, t in enumerate(BIG_TILES):
            m = min(4096, BIG_N - t * 4096)
            p[t * 4096:t * 4096 + m] = src[k * 4096:k * 4096 + m]
        TERMS["big"] = base._replace(points=p)
    return TERMS["big"]


def cells_of(name):
    c = big_case() if name == "big" else TERMS[name]
    if ("cells", name) not in _REF:
        _REF["cells", name] = M.mesh(c.height, 1, c.max_jump)[1]
    return _REF["cells", name]


def rows_reference(name):
    if ("rows", name) not in _REF:
        c = TERMS[name]
        _REF["rows", name] = R.rows(c.points, c.pose, c.height, c.frame, cells_of(name), c.center, c.gate)
    return _REF["rows", name]


def terms_reference(name):
    """-> the reference's RECORD of a case"""
    if ("terms", name) not in _REF:
        c = big_case() if name == "big" else TERMS[name]
        _REF["terms", name] = R.terms(c.points, c.pose, c.height, c.frame, cells_of(name), c.center, c.gate)
    return _REF["terms", name]


# ---- the transform: every case's cloud and pose, and the special points
TRANSFORM = {name: (c.points, c.pose) for name, c in TERMS.items() if name.startswith(("relief/", "skew")) or name in ("n0", "n1", "n257", "n4097")}
TRANSFORM["specials"] = (np.concatenate([AC.SPECIAL_POINTS, AC.SPECIAL_POINTS[::-1]]), SIMILARITY)

# ---- a flat reference: N is (0, 0, 1) exactly, so N.x is 0 and the system of tx has no pivot; heights and the cloud's z are
# multiples of 1/8, so every sum is exact
FLAT_HEIGHT = np.full((5, 7), 0.5, np.float32)
FLAT_FRAME = DC.axis_frame(7, 5, cell=0.5)


def flat_case():
    p = AC.interior(500, 7, 5, 0.5, 23)
    p[:, 2] = 0.5 + (np.arange(500) % 9 - 3) * 0.125
    return TermsCase(p, R.pose(pivot=(1.75, 1.25, 0.5)), FLAT_HEIGHT, FLAT_FRAME, INF, 0.0, INF)


# ---- the rendered scene: accuracy_cases.truth_cloud(0, 2) displaced by the inverse of a known motion
MOTION_CELLS = (0.8, -0.6, 0.5)          # along ex, ey, ez
MOTION_ROTATION = (0.004, -0.003, 0.006)  # a rotation vector, rad, about the cloud's centroid
MOTION_SCALE = 1.01                       # "similarity" only
OUTLIER_EVERY, OUTLIER_CELLS = 10, 20.0
_SCENE = {}


def motion(similarity=False):
    """-> (A float64 (3, 3), b float64 (3,)): the true motion x -> A x + b that takes the displaced cloud back"""
    fr = DC.scene_frame()
    truth = AC.truth_cloud(0, 2).astype(np.float64)
    c = truth.mean(0)
    A = (MOTION_SCALE if similarity else 1.0) * R.rotation(MOTION_ROTATION)
    t = float(fr.cell) * (MOTION_CELLS[0] * fr.ex.astype(np.float64) + MOTION_CELLS[1] * fr.ey.astype(np.float64) + MOTION_CELLS[2] * fr.ez.astype(np.float64))
    return A, c - A @ c + t


def displaced(similarity=False, outliers=False):
    """-> (cloud float32 (n, 3): the truth cloud under the inverse of motion(), every tenth point raised 20 cells along ez with
    `outliers`; truth float32 (n, 3); keep bool (n,): the points that are no outliers)"""
    key = (similarity, outliers)
    if key not in _SCENE:
        fr = DC.scene_frame()
        truth = AC.truth_cloud(0, 2)
        A, b = motion(similarity)
        cloud = np.linalg.solve(A, (truth.astype(np.float64) - b).T).T
        keep = np.ones(len(truth), bool)
        if outliers:
            keep[::OUTLIER_EVERY] = False
            cloud[~keep] += OUTLIER_CELLS * float(fr.cell) * fr.ez.astype(np.float64)
        _SCENE[key] = (cloud.astype(np.float32), truth, keep)
    return _SCENE[key]


def offset_cells(cloud, g, truth, keep):
    """the RMS distance, in cells, of the kept points of `cloud` under pose g from their true places"""
    fr = DC.scene_frame()
    err = R.apply64(g, cloud[keep]) - truth[keep].astype(np.float64)
    return float(np.sqrt((err ** 2).sum(1).mean()) / float(fr.cell))


def scene_reference(dof, gate, outliers, iterations=6):
    """the reference's registration of the displaced scene -> (result, offset in cells before, after)"""
    key = ("register", dof, gate, outliers, iterations)
    if key not in _SCENE:
        cloud, truth, keep = displaced(dof == "similarity", outliers)
        res = R.register(cloud, AC.truth_map(), DC.scene_frame(), dof=dof, iterations=iterations, gate=gate)
        _SCENE[key] = (res, offset_cells(cloud, R.pose(), truth, keep), offset_cells(cloud, res["pose"], truth, keep))
    return _SCENE[key]
