"""The height maps the surface simplification is held to (include/ssrlcv_hip.h "surface simplification"): shared by
tests/test_simplify_cases.py (the restatement against a plain bintree walk and the mesh's properties, no GPU) and
tests/test_gpu_simplify.py (the kernels against the restatement).  Sizes are (w, h)."""
import itertools

import numpy as np

import simplify_ref as R

TILE = 64  # the side the sizes are built from: a level whose lattice has at most TILE^2 nodes runs in the one-block tail of
#            csrc/simplify.hip (kTailNodes), a larger one as two launches of its own; T and T + 1 lie on either side of that bound
AXIS = (1, 2, 3, 5, TILE, TILE + 1, TILE + 2, 2 * TILE + 1, 2 * TILE + 3)
UPPER = (4 * TILE + 1, 4 * TILE + 1)   # S = 4 T: the levels 0, 1 and 2 run as launches of their own, the others in the tail
THIN = (3, 2 * TILE + 3)
ALL_SIZES = tuple(itertools.product(AXIS, AXIS)) + (UPPER, THIN)
# the sizes every other content runs at: a 2^L + 1 square, both axes past one tile with different tile counts, the odd corner
# of the list, the size with levels above the tile, the thin map and one below every tile
FEW_SIZES = ((TILE + 1, TILE + 1), (TILE + 2, 2 * TILE + 1), (2 * TILE + 3, 2 * TILE + 3), UPPER, THIN, (5, 2))
SMALL_SIZES = ((2, 2), (3, 3), (5, 5), (4, 7), (9, 9), (17, 12), (33, 33), (20, 34))  # the bintree walk's


def _rng(name, w, h):
    return np.random.default_rng([sum(name.encode()), w, h])


def noise(w, h):
    return _rng("noise", w, h).random((h, w), np.float32)


def relief(w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    return (np.float32(3) * np.sin(x / np.float32(7)) * np.cos(y / np.float32(5)) + np.float32(0.02) * x).astype(np.float32)


def plane(w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    return (np.float32(0.5) * x - np.float32(0.25) * y + np.float32(3)).astype(np.float32)  # exact in float32: every e is 0


def _spike(at):
    def make(w, h):
        m = np.zeros((h, w), np.float32)
        m[min(at[1], h - 1), min(at[0], w - 1)] = np.float32(7)
        return m
    return make


def holes(w, h):
    m = relief(w, h)
    m[_rng("holes", w, h).random((h, w)) < 0.05] = R.invalid()
    return m


def seam_hole(w, h):
    m = relief(w, h)
    m[min(TILE, h - 1), min(TILE // 2, w - 1)] = R.invalid()   # on a tile's edge
    m[min(TILE, h - 1), min(TILE, w - 1)] = R.invalid()        # on a tile's corner
    return m


def all_invalid(w, h):
    return np.full((h, w), R.invalid(), np.float32)


def specials(w, h):
    m = noise(w, h)
    r = _rng("specials", w, h)
    pick = r.random((h, w))
    m[pick < 0.03] = np.float32(np.inf)
    m[(pick >= 0.03) & (pick < 0.06)] = np.array([0x7FC00001], np.uint32).view(np.float32)[0]  # a NaN that is a valid value
    m[(pick >= 0.06) & (pick < 0.12)] = np.float32(-0.0)
    m[(pick >= 0.12) & (pick < 0.14)] = np.float32(-np.inf)
    return m


def huge(w, h):
    big = np.float32(3.0e38)
    sign = np.where(_rng("huge", w, h).random((h, w)) < 0.3, np.float32(-1), np.float32(1))
    return (big * sign * (np.float32(0.9) + np.float32(0.1) * noise(w, h))).astype(np.float32)  # h(a) + h(b) overflows


CONTENTS = {
    "noise": (noise, ALL_SIZES),
    "relief": (relief, FEW_SIZES),
    "plane": (plane, FEW_SIZES),
    "spike_tile_corner": (_spike((TILE, TILE)), FEW_SIZES),
    "spike_tile_edge": (_spike((TILE, TILE // 2 + 1)), FEW_SIZES),
    "spike_tile_interior": (_spike((TILE + 5, 27)), FEW_SIZES),
    "holes": (holes, FEW_SIZES),
    "seam_hole": (seam_hole, FEW_SIZES),
    "all_invalid": (all_invalid, FEW_SIZES),
    "specials": (specials, FEW_SIZES),
    "huge": (huge, FEW_SIZES),
}


def tolerances(error):
    """-1, 0, one near the median of the map's finite positive errors -- roughly half of the triangles go --, a huge finite one;
    ascending"""
    e = error[np.isfinite(error) & (error > 0)]
    half = float(np.median(e.astype(np.float64))) if e.size else 0.5  # in float64: the mean of two errors near FLT_MAX is finite
    return tuple(sorted((-1.0, 0.0, half, 1.0e30)))


def cases(names=None):
    """(id, height) of every case"""
    for name, (make, sizes) in CONTENTS.items():
        if names is not None and name not in names:
            continue
        for w, h in sizes:
            yield "%s-%dx%d" % (name, w, h), make(w, h)
