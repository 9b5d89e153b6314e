"""The map kernels of the stereo and the surface chains past the caps of their launch grids.  Shared by tests/test_large_cases.py
(which proves on the references alone that every case reaches what it claims) and tests/test_gpu_large.py (which holds the kernels
to the references bit for bit).

These kernels launch at most CAP blocks of 256 threads and walk the rest of the map in a grid-stride loop: up to CAP x 256
elements the loop body runs once for every thread, and the later trips are what the small cases of the other files never run.
Every cap is read out of the kernels' sources (CAPS: file, pattern), so a changed cap moves the sizes here, and
tests/test_large_cases.py fails if a size no longer passes its threshold.  A map is w wide and threshold // w + 1 + tail rows
high: the first row that holds an element of the second trip, and `tail` rows behind it.

  kernel                                                   cap            threshold     case
  k_stereo_fill, k_stereo_lr (stereo.hip)                  2048 x 256       524 288     1031 x 770, r 1, dmin -1, D 6, lr 1, subpixel
  k_census<1, 2, 3> (stereo.hip)                           8192 x 256     2 097 152     2049 x 1100 random bytes
  k_cc_roots, k_cc_sizes, k_speckle_apply, k_fill_select   4096 x 256     1 048 576     1025 x 1200: 17 x 75 tiles, ten strips of the fill
  k_ortho_top (ortho.hip)                                  2048 x 256, four loads a lane: load t reads [t, t + 1) x 524 288 on the
                                                           first trip, the second trip starts at 2 097 152: 1449 x 1449
  k_render_scatter (render.hip)                            8192 x 256     2 097 152     1450 x 1449 nodes = 1449 x 1448 cells
  k_subtract (terrain.hip)                                 65536 x 256   16 777 216     4097 x 4096

Every reference is computed once, shared and never modified."""
import math
import os
import re
from collections import namedtuple

import numpy as np

import helpers as H
import speckle_cases as S

CSRC = os.path.join(H.ROOT, "ssrlcv_amd", "csrc")
BLOCK = 256

# name -> (file, the pattern whose groups are all the cap)
CAPS = {
    "stereo": ("stereo.hip", r"if \(fillBlocks > (\d+)u\) fillBlocks = (\d+)u;"),
    "census": ("stereo.hip", r"if \(blocks > (\d+)u\) blocks = (\d+)u;\s+hipLaunchKernelGGL\(k_census<C>, dim3\(blocks\), dim3\(256\)"),
    "filter": ("disparity_filter.hip", r"unsigned capped_blocks\(uint32_t items\) \{\s+const unsigned b = [^;]+;\s+return b > (\d+)u \? (\d+)u : b;"),
    "ortho": ("ortho.hip", r"unsigned top_blocks\(uint32_t cells\) \{\s+const unsigned b = [^;]+;\s+return b > (\d+)u \? (\d+)u : b;"),
    "render": ("render.hip", r"constexpr uint32_t kScatterBlocks = (\d+);"),
    "subtract": ("terrain.hip", r"hipLaunchKernelGGL\(k_subtract, dim3\(umin\(\(n \+ 255u\) / 256u, (\d+)u\)\), dim3\(256\)"),
}
ORTHO_LOADS_PATTERN = ("ortho.hip", r"c0 < cells; c0 \+= (\d+)u \* stride\) \{[^\n]*\n\s+uint32_t bits\[(\d+)\];")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def read_constant(file, pattern):
    """the one number the pattern's groups name, in the one place of the file that matches"""
    found = re.findall(pattern, source(file))
    assert len(found) == 1, (file, pattern, found)
    values = {int(v) for v in (found[0] if isinstance(found[0], tuple) else (found[0],))}
    assert len(values) == 1, (file, pattern, found)
    return values.pop()


CAP = {name: read_constant(*where) for name, where in CAPS.items()}
THRESHOLD = {name: cap * BLOCK for name, cap in CAP.items()}      # the elements one trip of the grid covers
ORTHO_LOADS = read_constant(*ORTHO_LOADS_PATTERN)


def rows_past(name, w, tail):
    """the height of a map w wide whose row threshold // w is the first with an element of the second trip, `tail` rows behind it"""
    return THRESHOLD[name] // w + 1 + tail


def later(name, shape):
    """bool map: the elements the second and later trips of the kernels of `name` own"""
    h, w = shape
    return (np.arange(h * w).reshape(h, w) >= THRESHOLD[name])


# ---- 1. block matching and semi-global matching
STEREO_W = CAP["stereo"] // 2 + 7      # odd, no multiple of a tile's width
STEREO_H = rows_past("stereo", STEREO_W, 261)       # SGM's diagonals run up to h - 2 r steps
SGM = dict(clamp=1000, P1=40, P2=400, paths=0xFF)
MATCH_IDS = (3, 7)
_STEREO = {}


def stereo_case():
    import stereo_cases as SC
    return SC.Case(STEREO_W, STEREO_H, 1, -1, 6, SC.NO_LIMIT, 1, 1, "scene", 31)


def stereo_scene():
    import stereo_cases as SC
    if "scene" not in _STEREO:
        _STEREO["scene"] = SC.scene(stereo_case())
    return _STEREO["scene"]


def stereo_reference():
    import stereo_ref as R
    if "bm" not in _STEREO:
        c = stereo_case()
        left, right = stereo_scene()
        _STEREO["bm"] = R.disparity_ref(left, right, c.r, c.dmin, c.D, c.max_cost, c.lr, c.subpixel)
    return _STEREO["bm"]


def sgm_reference():
    import sgm_ref as G
    if "sgm" not in _STEREO:
        c = stereo_case()
        left, right = stereo_scene()
        _STEREO["sgm"] = G.sgm_ref(left, right, c.r, c.dmin, c.D, SGM["clamp"], SGM["P1"], SGM["P2"], SGM["paths"], c.lr, c.subpixel)
    return _STEREO["sgm"]


def matches_reference():
    import stereo_ref as R
    if "matches" not in _STEREO:
        _STEREO["matches"] = R.matches_ref(stereo_reference()["disparity"], 1, *MATCH_IDS)
    return _STEREO["matches"]


# ---- 2. census codes
CENSUS_W = CAP["census"] // 4 + 1
CENSUS_TAIL = 76
CENSUS_H = rows_past("census", CENSUS_W, CENSUS_TAIL)
CENSUS_RADII = (1, 2, 3)
_CENSUS = {}


def census_image():
    if "image" not in _CENSUS:
        _CENSUS["image"] = np.random.RandomState(41).randint(0, 256, size=(CENSUS_H, CENSUS_W)).astype(np.uint8)
    return _CENSUS["image"]


def census_reference(c):
    import census_ref as CR
    if c not in _CENSUS:
        _CENSUS[c] = CR.census(census_image(), c)
    return _CENSUS[c]


# ---- 3. components, speckles and fill
FILTER_W = CAP["filter"] // 4 + 1
FILTER_H = rows_past("filter", FILTER_W, 176)
TILES_X, TILES_Y = -(-FILTER_W // S.TILE_W), -(-FILTER_H // S.TILE_H)
LATER_ROW = THRESHOLD["filter"] // FILTER_W + 1     # from this row on every pixel belongs to a later trip
MAX_SPECKLE = S.MAX_SPECKLE
BAR_ROW, BAR_COLUMN = 69 * S.TILE_H, 7 * S.TILE_W   # a horizontal and a vertical tile seam below LATER_ROW
BAR_SIZES = (MAX_SPECKLE - 1, MAX_SPECKLE, MAX_SPECKLE + 1)
COMPONENT_NAMES = ("serpentine", "serpentine_t", "comb_bottom", "noise")
_FILTER = {}


def _noise():
    """three levels, 10 % holes, linked only where equal; the bars of speckle_cases' `blobs` astride a seam each, below LATER_ROW,
    in values of their own"""
    rng = np.random.RandomState(43)
    d = np.array([1.0, 2.0, 3.0], np.float32)[rng.randint(0, 3, size=(FILTER_H, FILTER_W))]
    d[rng.rand(FILTER_H, FILTER_W) < 0.10] = S.INVALID
    y0 = BAR_ROW - 30
    d[y0 - 2:BAR_ROW + 12, BAR_COLUMN - 12:BAR_COLUMN + 12] = S.INVALID     # a clearing for the bars
    for k, n in enumerate(BAR_SIZES):
        d[y0 + 3 * k, BAR_COLUMN - 6:BAR_COLUMN - 6 + n] = 4.0 + k                    # astride x = BAR_COLUMN
        d[BAR_ROW - 6:BAR_ROW - 6 + n, BAR_COLUMN - 9 + 3 * k] = 9.0                  # astride y = BAR_ROW
    return d


def component_case(name):
    """-> speckle_cases.Case"""
    if name not in _FILTER:
        if name == "serpentine":
            d, n = S._serpentine(FILTER_W, FILTER_H)
            k = S.Case(d, 0.25, MAX_SPECKLE, [n])
        elif name == "serpentine_t":
            d, n = S._serpentine(FILTER_W, FILTER_H)
            k = S.Case(np.ascontiguousarray(d.T), 0.25, MAX_SPECKLE, [n])
        elif name == "comb_bottom":
            d = S._holes(FILTER_W, FILTER_H)
            d[:, 0::2] = 6.0
            d[FILTER_H - 1, :] = 6.0
            k = S.Case(d, 1.0, MAX_SPECKLE, [(FILTER_W + 1) // 2 * (FILTER_H - 1) + FILTER_W])
        else:
            k = S.Case(_noise(), 0.0, MAX_SPECKLE, None)
        k.d.setflags(write=False)
        _FILTER[name] = k
    return _FILTER[name]


def component_reference(name):
    """-> (labels, sizes) of speckle_ref.components_ref"""
    import speckle_ref as R
    key = ("components", name)
    if key not in _FILTER:
        k = component_case(name)
        _FILTER[key] = R.components_ref(k.d, k.max_diff)
    return _FILTER[key]


def speckle_cost():
    """a cost of its own at every pixel, UINT32_MAX at the holes"""
    import speckle_ref as R
    d = component_case("noise").d
    cost = (np.arange(d.size, dtype=np.uint32).reshape(d.shape) * np.uint32(2654435761)) >> np.uint32(8)
    cost[~R.valid_mask(d)] = 0xFFFFFFFF
    return cost


def speckle_reference():
    """-> (disparity, cost) of speckle_ref.speckles_ref on the noise map"""
    import speckle_ref as R
    if "speckles" not in _FILTER:
        k = component_case("noise")
        _FILTER["speckles"] = R.speckles_ref(k.d, speckle_cost(), k.max_diff, k.max_size)
    return _FILTER["speckles"]


FILL_STRIP = 128                  # rows of a strip of the fill's march
FILL_SHARE = 0.08                 # of holes, at most: the reference is a loop over the holes
FILL_BAND = (FILL_STRIP * 8 - 7, FILL_STRIP * 8 + 10)   # rows, across the strip seam at 1024
FILL_COLUMN = 3
FILL_BLOCK = (1100, 1130, 300, 340)                     # rows, columns of holes: its middle is out of every ray's reach at maxGap 7


def fill_calls():
    import fill_ref as F
    return (dict(paths=0xFF, max_gap=7, min_hits=3, rule=F.MEDIAN), dict(paths=0xFC, max_gap=F.NO_LIMIT, min_hits=3, rule=F.MEDIAN))


def fill_map():
    import fill_cases as FC
    if "fill" not in _FILTER:
        rng = np.random.default_rng(47)
        d = FC._rich(rng, FILTER_W, FILTER_H)
        hole = rng.random((FILTER_H, FILTER_W)) < 0.01
        for _ in range(1800):
            x, y = int(rng.integers(0, FILTER_W)), int(rng.integers(0, FILTER_H))
            hole[y:y + int(rng.integers(1, 9)), x:x + int(rng.integers(1, 13))] = True
        hole[FILL_BAND[0]:FILL_BAND[1], :] = True
        hole[:, FILL_COLUMN] = True
        hole[FILL_BLOCK[0]:FILL_BLOCK[1], FILL_BLOCK[2]:FILL_BLOCK[3]] = True
        d[hole] = FC.INVALID
        d[FILL_BAND[0]:FILL_BAND[1], 7] = 9.5          # one measured column through the band
        d.setflags(write=False)
        _FILTER["fill"] = d
    return _FILTER["fill"]


def fill_reference(call):
    """-> (out, filled) of fill_ref.fill for fill_calls()[call]"""
    import fill_ref as F
    key = ("fill", call)
    if key not in _FILTER:
        _FILTER[key] = F.fill(fill_map(), **fill_calls()[call])
    return _FILTER[key]


# ---- 4. ortho top
ORTHO_SIDE = math.isqrt(ORTHO_LOADS * THRESHOLD["ortho"]) + 1     # the smallest square with a second trip
ORTHO_RANGE = THRESHOLD["ortho"]                                  # load t of the first trip reads cells [t, t + 1) x ORTHO_RANGE
ORTHO_VARIANTS = tuple("load%d" % t for t in range(4)) + ("trip2",)
TOWER_HEIGHT, TOWER_HALF = 6.0, 4
ORTHO_STEPS, ORTHO_BIAS = 256, 0.05
_ORTHO = {}


def _ground():
    if "ground" not in _ORTHO:
        import dsm_ref as D
        rng = np.random.RandomState(53)
        z = (rng.rand(ORTHO_SIDE, ORTHO_SIDE) * 0.2).astype(np.float32)
        b = D.bits(z).copy()
        b[rng.rand(ORTHO_SIDE, ORTHO_SIDE) < 0.01] = D.INVALID_BITS
        _ORTHO["ground"] = b.view(np.float32)
    return _ORTHO["ground"]


def tower_cells(variant):
    """(j0, j1, i0, i1): the cells of the tower, all inside the index range that one load, or the second trip alone, reads"""
    i = ORTHO_SIDE // 2
    if variant == "trip2":   # a short wall on the last row
        return ORTHO_SIDE - 1, ORTHO_SIDE, i - 10, i + 11
    t = ORTHO_VARIANTS.index(variant)
    j = (t * ORTHO_RANGE + ORTHO_RANGE // 2) // ORTHO_SIDE
    return j - TOWER_HALF, j + TOWER_HALF + 1, i - TOWER_HALF, i + TOWER_HALF + 1


def ortho_case(variant, tower=True):
    """-> ortho_cases.Case: the ground, the tower of the variant (tower = False: flattened to the ground) and one oblique view
    with a narrow field, aimed at the tower from beyond it (+y), so that the tower's shadow falls back onto the map"""
    import dsm_cases as DC
    import ortho_cases as OC
    key = (variant, tower)
    if key not in _ORTHO:
        fr = DC.axis_frame(ORTHO_SIDE, ORTHO_SIDE, cell=OC.CELL)
        j0, j1, i0, i1 = tower_cells(variant)
        z = _ground().copy()
        if tower:
            z[j0:j1, i0:i1] = TOWER_HEIGHT
        foot = np.array([(i0 + i1) / 2.0 * OC.CELL, (j0 + j1) / 2.0 * OC.CELL, 0.0])
        pos = foot + (0.0, 120.0, 60.0)
        img = OC.IMAGES["96x96"]
        cam = OC.camera(pos, foot - pos, (img.shape[1], img.shape[0]), 2.0 * math.atan(30.0 / 134.0))
        _ORTHO[key] = OC.Case(z, fr, [OC.view_of(cam, fr, img)], ORTHO_STEPS, ORTHO_BIAS, OC.R.FIRST, True)
    return _ORTHO[key]


def ortho_reference(variant, tower=True):
    import ortho_ref as R
    key = ("ref", variant, tower)
    if key not in _ORTHO:
        c = ortho_case(variant, tower)
        _ORTHO[key] = R.ortho(c.height, c.frame, c.views, c.max_steps, c.bias, c.rule)
    return _ORTHO[key]


# ---- 5. render scatter
RENDER_GW = math.isqrt(THRESHOLD["render"]) + 2
RENDER_GH = RENDER_GW - 1
RENDER_CELLS = (RENDER_GW - 1) * (RENDER_GH - 1)
RENDER_LAST_ROW = RENDER_GH - 2                                        # the last cell row
RENDER_FIRST_LATE = THRESHOLD["render"] - RENDER_LAST_ROW * (RENDER_GW - 1)   # its first cell of the second trip
Quad = namedtuple("Quad", "name cj ci byte corners grey")
_RENDER = {}


def render_quads():
    """the few quads of the grid.  `far` and `front` lie in the first trip, `near`, `large` and `bad` in the last cell row behind
    RENDER_FIRST_LATE: `near` lies in front of `far` and behind `front`"""
    import render_cases as RC
    late = RENDER_FIRST_LATE + (RENDER_FIRST_LATE & 1)   # even columns: no two quads share a node
    nan = float("nan")
    sq = RC.square(1, 1, 5)
    return [Quad("far", 0, 0, 3, RC.square(0, 0, 7, z=2.0), (10, 90, 170, 250)),
            Quad("front", 700, 10, 7, RC.square(3, 1, 4, z=1.25), (200, 210, 220, 230)),
            Quad("near", RENDER_LAST_ROW, late, 3, RC.square(2, 2, 3, z=1.5), (5, 5, 5, 5)),
            Quad("large", RENDER_LAST_ROW, late + 2, 1, RC.square(-1, -1, 9), (1, 2, 3, 4)),         # 9 pixels wide at maxExtent 8
            Quad("bad", RENDER_LAST_ROW, late + 4, 1, [(nan, 1.0, 1.0)] + sq[1:], (9, 9, 9, 9))]


def render_case():
    """-> render_cases.Case"""
    import render_cases as RC
    import render_ref as R
    if "case" not in _RENDER:
        quads = render_quads()
        vertex_index = np.full((RENDER_GH, RENDER_GW), R.NONE, np.uint32)
        cells = np.zeros((RENDER_GH - 1, RENDER_GW - 1), np.uint8)
        points, grey = np.zeros((4 * len(quads), 3), np.float32), np.zeros(4 * len(quads), np.uint8)
        for k, q in enumerate(quads):
            cells[q.cj, q.ci] = q.byte
            vertex_index[q.cj, q.ci:q.ci + 2] = (4 * k, 4 * k + 1)           # a, b
            vertex_index[q.cj + 1, q.ci:q.ci + 2] = (4 * k + 2, 4 * k + 3)   # c, d
            points[4 * k:4 * k + 4] = q.corners
            grey[4 * k:4 * k + 4] = q.grey
        _RENDER["case"] = RC.Case(points, grey, vertex_index, cells, RC.eye_view(8, 8), 8)
    return _RENDER["case"]


def render_reference():
    """-> (render_ref.render's dict, cover: triangle id -> the set of pixels (x, y) it covers)"""
    import render_ref as R
    if "ref" not in _RENDER:
        c = render_case()
        cover = {}

        def on_cover(ids, xs, ys, v):
            for t, x, y in zip(ids.tolist(), xs.tolist(), ys.tolist()):
                cover.setdefault(t, set()).add((x, y))

        _RENDER["ref"] = (R.render(c.points, c.grey, c.vertex_index, c.cells, c.view, c.max_extent, on_cover=on_cover), cover)
    return _RENDER["ref"]


# ---- 6. subtract
SUBTRACT_W = CAP["subtract"] // 16 + 1
SUBTRACT_H = rows_past("subtract", SUBTRACT_W, 0)
_SUBTRACT = {}


def subtract_pair():
    """terrain_cases.subtract_pair, its four forced pairs also at the end of the last row: in the second trip"""
    import terrain_cases as TC
    if "pair" not in _SUBTRACT:
        a, b = TC.subtract_pair(SUBTRACT_W, SUBTRACT_H)
        a, b = a.view(np.uint32), b.view(np.uint32)
        a[-1, -4:], b[-1, -4:] = a[0, :4], b[0, :4]
        a, b = a.view(np.float32), b.view(np.float32)
        a.setflags(write=False), b.setflags(write=False)
        _SUBTRACT["pair"] = (a, b)
    return _SUBTRACT["pair"]


def subtract_reference():
    import terrain_ref as R
    if "ref" not in _SUBTRACT:
        _SUBTRACT["ref"] = R.bits_of(R.subtract(*subtract_pair()))
    return _SUBTRACT["ref"]
