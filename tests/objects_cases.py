"""The cases of "surface objects" (include/ssrlcv_hip.h): the maps and parameters that tests/test_objects_cases.py runs through the
restatement and the plain loop of tests/objects_ref.py without a GPU, and tests/test_gpu_objects.py through csrc/objects.hip.
Sizes are (w, h), around the 64 x 16 tile of the reduction; LARGE lies past the cap of every capped grid of objects.hip, read from
its source.  Every reference is computed once, shared and never modified."""
import os
import re
import zlib
from collections import namedtuple

import numpy as np

import objects_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
Case = namedtuple("Case", "name d min_height max_diff scale min_cells")
SIZES = ((1, 1), (1, 37), (37, 1), (64, 16), (65, 17), (63, 5), (130, 35))
TILE_W, TILE_H = 64, 16


def _bits(values):
    return np.array(values, np.uint32).view(np.float32)


def hole_map(w, h):
    return np.full((h, w), R.INVALID, np.uint32).view(np.float32).copy()


def _rng(name, w, h):
    return np.random.RandomState(zlib.crc32(("%s-%dx%d" % (name, w, h)).encode()) & 0x7FFFFFFF)


def case(name, d, min_height=1.0, max_diff=INF, scale=256.0, min_cells=1):
    return Case(name, np.ascontiguousarray(d, np.float32), float(min_height), float(max_diff), float(scale), int(min_cells))


# ---- object content
def whole(w, h):
    """one object that is the whole map: every tile flushes into one record"""
    rng = _rng("whole", w, h)
    return (2.0 + rng.rand(h, w) * 3).astype(np.float32)


def checkerboard(w, h):
    """one-cell objects, as many as a map can hold; the other cells are ground, holes or low"""
    rng = _rng("checker", w, h)
    d = (rng.rand(h, w) * 0.9).astype(np.float32)
    d.view(np.uint32)[rng.rand(h, w) < 0.3] = R.INVALID
    yy, xx = np.mgrid[:h, :w]
    on = (xx + yy) % 2 == 0
    d[on] = (1.0 + rng.rand(int(on.sum())) * 4).astype(np.float32)
    return d


def serpentine(w, h):
    """one object through every tile: full even rows, joined at alternating ends"""
    d = np.zeros((h, w), np.float32)
    d[0::2] = 2.5
    for y in range(1, h, 2):
        d[y, w - 1 if (y // 2) % 2 == 0 else 0] = 3.5
    return d


def seams(w, h):
    """a bar across a vertical seam, one across a horizontal seam, a block on a four-tile corner; each alone"""
    d = np.zeros((h, w), np.float32)
    if w > TILE_W + 6 and h > TILE_H + 6:
        d[3, TILE_W - 5:TILE_W + 6] = 2.0
        d[TILE_H - 4:TILE_H + 5, 7] = 3.0
        d[TILE_H - 2:TILE_H + 2, TILE_W - 2:TILE_W + 2] = 4.0
    return d


def ring(w, h):
    """a ring around a hole with an island in it: the ring's box holds cells that are not its own"""
    d = np.zeros((h, w), np.float32)
    if w >= 13 and h >= 11:
        x0, y0 = w - 12, h - 10
        d[y0:y0 + 9, x0:x0 + 11] = 2.0
        d[y0 + 2:y0 + 7, x0 + 2:x0 + 9] = 0.0
        d[y0 + 4, x0 + 4:x0 + 7] = 5.0
    return d


def blobs(w, h):
    """random members over holes: many shapes, some one cell, some over several tiles"""
    rng = _rng("blobs", w, h)
    d = (rng.rand(h, w) * 6 - 1).astype(np.float32)
    d.view(np.uint32)[rng.rand(h, w) < 0.1] = R.INVALID
    d[rng.rand(h, w) < 0.42] = 0.25
    return d


def two_levels(w, h):
    """a block whose halves stand 2 and 5 high, a ramp of 0.5 a cell beside it: a finite maxDiff parts the block and keeps the ramp"""
    d = np.zeros((h, w), np.float32)
    half = max(w // 4, 1)
    d[: max(h // 2, 1), :half] = 2.0
    d[: max(h // 2, 1), half:2 * half] = 5.0
    if h > 2:
        d[-1, :] = (1.0 + 0.5 * np.arange(w)).astype(np.float32)
    return d


# ---- values
def hard_values(w, h):
    """equal peaks, -0 against +0, +inf, NaNs beside the invalid pattern, -inf, both sides of the clip bound, ties of rintf"""
    pool = np.concatenate([
        _bits([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC00000, 0x7FFFFFFF, R.INVALID, 0x7F7FFFFF, 0xFF7FFFFF]),
        np.array([256.0, 255.99998, 256.00003, -256.0, -256.00003, 0.001953125, 0.005859375, 0.009765625, -0.001953125, -0.005859375,
                  1.5, 1.5, 1.5, 3.0, 3.0, 100.0, -100.0], np.float32)])
    rng = _rng("hard", w, h)
    return pool[rng.randint(len(pool), size=(h, w))]


def zeros_pair(w, h):
    """a map of -0 and +0 alone: at minHeight 0 both are members, the peak is +0 and the low -0 where both occur"""
    rng = _rng("zeros", w, h)
    return _bits([0x00000000, 0x80000000])[rng.randint(2, size=(h, w))]


def _content_cases():
    out = []
    for w, h in SIZES:
        size = "%dx%d" % (w, h)
        out.append(case("whole " + size, whole(w, h)))
        out.append(case("checkerboard " + size, checkerboard(w, h)))
        out.append(case("blobs " + size, blobs(w, h)))
        out.append(case("blobs minCells 4 " + size, blobs(w, h), min_cells=4))
        out.append(case("hard -inf " + size, hard_values(w, h), min_height=-INF))
        out.append(case("hard +inf " + size, hard_values(w, h), min_height=INF))
        out.append(case("hard 0 maxDiff 1 " + size, hard_values(w, h), min_height=0.0, max_diff=1.0))
        out.append(case("hard -300 scale 1 " + size, hard_values(w, h), min_height=-300.0, scale=1.0))
        out.append(case("zeros " + size, zeros_pair(w, h), min_height=0.0))
        out.append(case("zeros maxDiff 0 " + size, zeros_pair(w, h), min_height=-0.0, max_diff=0.0))
        out.append(case("nothing " + size, hole_map(w, h)))
        out.append(case("two levels maxDiff 0.5 " + size, two_levels(w, h), max_diff=0.5))
        out.append(case("two levels " + size, two_levels(w, h)))
    for w, h in ((65, 17), (130, 35)):
        size = "%dx%d" % (w, h)
        out.append(case("serpentine " + size, serpentine(w, h)))
        out.append(case("seams " + size, seams(w, h)))
        out.append(case("ring " + size, ring(w, h)))
        out.append(case("blobs minCells 0 " + size, blobs(w, h), min_cells=0))
        out.append(case("blobs minCells 40 maxDiff 2 " + size, blobs(w, h), max_diff=2.0, min_cells=40))
    return out


CASES = _content_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
_REFERENCE = {}


def reference(c):
    """the restatement's result of a case, computed once"""
    if c.name not in _REFERENCE:
        _REFERENCE[c.name] = R.objects(c.d, c.min_height, c.max_diff, c.scale, c.min_cells)
    return _REFERENCE[c.name]


# ---- the boxed scene of tests/terrain_cases.py behind the terrain filter: what the references give, fixed here
SCENE_MIN_HEIGHT = 1.0
SCENE_CELLS = (25, 9, 1, 64, 256)            # in raster order of the objects' first cells: the boxes of side 5, 3, 1, 8 and 16
SCENE_PERIMETERS = (20, 12, 4, 32, 64)
_SCENE = {}


def scene_objects():
    """-> dict(objects: the object-height map of the boxed scene from terrain_ref and fill_ref with terrain_cases.SCHEDULE, as
    pipeline.surface_terrain computes it; want: the restatement's result at SCENE_MIN_HEIGHT); computed once"""
    if not _SCENE:
        import fill_ref as F
        import terrain_cases as TC
        import terrain_ref as T
        height = TC.scene()["height"]
        radii, thresholds = T.schedule(**TC.SCHEDULE)
        bare = T.terrain(height, radii, thresholds)["terrain"]
        objects = T.subtract(height, F.fill(bare, 0xFF, F.NO_LIMIT, 1, F.MEDIAN)[0])
        _SCENE.update(objects=objects, want=R.objects(objects, SCENE_MIN_HEIGHT))
    return _SCENE


# ---- past the caps of the launch grids
def caps():
    """the capped grids of csrc/objects.hip -> dict(mask, reduce, finish): blocks"""
    source = open(os.path.join(ROOT, "ssrlcv_amd", "csrc", "objects.hip")).read()
    found = {name.lower(): int(value) for name, value in re.findall(r"constexpr uint32_t k(Mask|Reduce|Finish)GridCap = (\d+);", source)}
    assert sorted(found) == ["finish", "mask", "reduce"], found
    return found


def large_size():
    """(w, h): more cells than the mask's grid has threads, more tiles than the reduction's has blocks, and a checkerboard of more
    objects than the last pass's has threads; w is no multiple of the tile and leaves an odd last column of tiles"""
    k = caps()
    cells = max(k["mask"] * 256, k["reduce"] * TILE_W * TILE_H, 2 * k["finish"] * 256)
    w = 1100
    h = cells // w + 47
    assert w * h > cells and (w // TILE_W) * (h // TILE_H) > k["reduce"] and (h // 2) * w // 2 > k["finish"] * 256
    return w, h


def large():
    """the checkerboard over the top half -- past the cap of the last pass --, one object over the bottom half that crosses every tile
    there, with a gradient so that the peak lies in the last row; one row of ground between them"""
    w, h = large_size()
    d = np.zeros((h, w), np.float32)
    top = h // 2
    yy, xx = np.mgrid[:top, :w]
    d[:top][(xx + yy) % 2 == 0] = 1.25
    d[:top][(xx + yy) % 2 == 0] += ((xx + 3 * yy)[(xx + yy) % 2 == 0] % 7).astype(np.float32)
    rows = np.arange(h - top - 1, dtype=np.float32)[:, None]
    d[top + 1:] = 2.0 + rows * np.float32(0.03125) + (np.arange(w) % 5 == 0).astype(np.float32)
    return case("large %dx%d" % (w, h), d)
