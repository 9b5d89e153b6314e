"""The disparity-mesh cases.  Shared by tests/test_mesh_cases.py (which proves on the numpy reference alone that the cases test
something) and tests/test_gpu_mesh.py (which holds the kernels of csrc/mesh.hip to that reference bit for bit).

The kernels are a thread per node or cell and two ordered compactions (csrc/compact.h: a wave owns a run of 1024 elements, a
block 4096), over the nodes and over two triangle slots a cell.  So the shapes go from one node up past both seams:

  shape_WxH         1 x 1, 1 x 37 and 41 x 1 (no cell at all), 2 x 2 (one cell), 3 x 2, random maps at step 1
  step_past_w       5 x 4 at step 7: one node
  rand_67x19        1273 nodes: past a wave's run.  rand_131x70_s2 and rand_97x83_s3: the grid is not the map
  rand_97x83        step 1: 8051 nodes and 2 x 7872 triangle slots, past a block of either compaction; _s5: step 5
  all_valid, all_invalid   a constant map: two triangles in every cell; no vertex at all
  ramp              all valid, d = 0.5 x + 0.25 y plus a ridge: every cell has both triangles, both diagonals occur, ties included
  jump_0, jump_inf  rand_67x19's map under max_jump 0 (only equal neighbours join, -0 and +0 among them) and +inf (only a NaN
                    difference cuts: the foreign NaN, and inf - inf)

A random map draws its disparities from the 0.5 grid over 0 .. 5.5, with about 30 % holes, about 2 % each of +inf and the foreign
NaN 0x7FC00001 (both valid values) and some -0; max_jump is 1.0.  random_case() keeps the first seed, counting up from the one
given, for which the reference's own cells show every byte value 1, 2, 3, 5, 6 and 7."""
from collections import namedtuple

import numpy as np

import mesh_ref as R

INVALID = R.INVALID
FOREIGN_NAN = np.array([0x7FC00001], np.uint32).view(np.float32)[0]
BYTES = (1, 2, 3, 5, 6, 7)

Case = namedtuple("Case", "d step max_jump")


def random_map(w, h, rng):
    d = (rng.integers(0, 12, (h, w)) * 0.5).astype(np.float32)
    d[(d == 0) & (rng.random((h, w)) < 0.5)] = -0.0
    u = rng.random((h, w))
    d[u < 0.30] = INVALID
    d[(u >= 0.30) & (u < 0.32)] = np.inf
    d[(u >= 0.32) & (u < 0.34)] = FOREIGN_NAN
    return d


def random_case(w, h, step, seed, max_jump=1.0):
    for s in range(seed, seed + 64):
        d = random_map(w, h, np.random.default_rng(s))
        cells = R.mesh(d, step, max_jump)[1]
        if all((cells == b).any() for b in BYTES):
            return Case(d, step, max_jump)
    raise AssertionError("no seed from %d shows every cell byte at %d x %d step %d" % (seed, w, h, step))


def _small(w, h, seed, step=1):
    return Case(random_map(w, h, np.random.default_rng(seed)), step, 1.0)


def _ramp(w, h):
    y, x = np.mgrid[0:h, 0:w]
    d = (0.5 * x + 0.25 * y).astype(np.float32)
    d[h // 2, :] += np.float32(0.75)               # a ridge: the diagonal flips along it
    d[:, w // 3] -= np.float32(0.5)
    return d


def _build():
    cases = {
        "shape_1x1": _small(1, 1, 3), "shape_1x37": _small(1, 37, 4), "shape_41x1": _small(41, 1, 5), "shape_2x2": Case(np.full((2, 2), 2.5, np.float32), 1, 1.0),
        "shape_3x2": Case(np.array([[1.0, 1.5, 4.0], [1.0, INVALID, 1.5]], np.float32), 1, 1.0),
        "step_past_w": _small(5, 4, 6, step=7),
        "rand_67x19": random_case(67, 19, 1, 1), "rand_131x70_s2": random_case(131, 70, 2, 1), "rand_97x83_s3": random_case(97, 83, 3, 1),
        "rand_97x83": random_case(97, 83, 1, 1), "rand_97x83_s5": _small(97, 83, 1, step=5),
        "all_valid": Case(np.full((17, 33), 3.0, np.float32), 1, 1.0), "all_invalid": Case(np.full((17, 33), INVALID, np.float32), 1, 1.0),
        "ramp": Case(_ramp(45, 23), 1, 1.0),
    }
    cases["jump_0"] = Case(cases["rand_67x19"].d, 1, 0.0)
    cases["jump_inf"] = Case(cases["rand_67x19"].d, 1, np.inf)
    for k in cases.values():
        k.d.setflags(write=False)
    return cases


CASES = _build()
_cache = {}


def points_of(name, n):
    """positions for the n vertices of a case: random, so that every order of the sums shows; a few coincide (zero cross products)"""
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    p = rng.normal(0, 4, (n, 3)).astype(np.float32)
    if n > 8:
        p[n // 2] = p[n // 2 - 1]
    return p


def reference(name):
    """-> dict(vertex_index, cells, n, faces, points, normals), computed once and read-only"""
    if name not in _cache:
        k = CASES[name]
        vi, cells, n = R.mesh(k.d, k.step, k.max_jump)
        pts = points_of(name, n)
        ref = dict(vertex_index=vi, cells=cells, n=n, faces=R.faces(vi, cells), points=pts, normals=R.normals(pts, vi, cells))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = ref
    return _cache[name]
