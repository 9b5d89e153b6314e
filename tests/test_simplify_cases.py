"""The numpy restatement of the surface simplification (tests/simplify_ref.py) held to a plain recursive bintree walk -- written
from the bintree alone, without the closed forms of include/ssrlcv_hip.h "surface simplification" -- and to the properties a
conforming, error-bounded mesh has.  No GPU."""
import math
from collections import Counter

import numpy as np
import pytest

import simplify_cases as C
import simplify_ref as R

WALK_TOLERANCES = (-1.0, 0.0, 0.05, 0.5, 1e9)


# ---- the plain walk: roots (0,0)-(S,S)-(S,0) and (S,S)-(0,0)-(0,S); (a, b, c) = hypotenuse a-b, apex c; children (c, a, m), (b, c, m)
class Walk:
    def __init__(self, height):
        self.height = height
        self.h, self.w = height.shape
        self.S = 1
        while self.S < max(self.w - 1, self.h - 1, 1):
            self.S *= 2
        S = self.S
        self.roots = [((0, 0), (S, S), (S, 0)), ((S, S), (0, 0), (0, S))]
        self.at = {}  # midpoint -> the triangles split there
        for t in self.roots:
            self._collect(t)
        self.E = {}

    def present(self, p):
        return p[0] < self.w and p[1] < self.h and self.height[p[1], p[0]].view(np.uint32) != R.INVALID_BITS

    @staticmethod
    def is_leaf(t):
        return abs(t[0][0] - t[1][0]) == 1  # the hypotenuse is one cell's diagonal

    @staticmethod
    def mid(t):
        return ((t[0][0] + t[1][0]) // 2, (t[0][1] + t[1][1]) // 2)

    def children(self, t):
        a, b, c = t
        m = self.mid(t)
        return (c, a, m), (b, c, m)

    def _collect(self, t):
        if self.is_leaf(t):
            return
        self.at.setdefault(self.mid(t), []).append(t)
        for ch in self.children(t):
            self._collect(ch)

    def error(self, m):
        if m in self.E:
            return self.E[m]
        tris = self.at[m]
        a, b = tris[0][0], tris[0][1]
        e = np.float32(np.inf)
        if self.present(m) and self.present(a) and self.present(b) and all(self.present(t[2]) for t in tris):
            with np.errstate(all="ignore"):
                mid = (self.height[a[1], a[0]] + self.height[b[1], b[0]]) * np.float32(0.5)
                d = np.abs(self.height[m[1], m[0]] - mid)
            if d < np.inf:
                e = np.float32(d)
        for t in tris:
            for ch in self.children(t):
                if not self.is_leaf(ch):
                    e = max(e, self.error(self.mid(ch)))
        self.E[m] = e
        return e

    def error_map(self):
        out = np.full((self.h, self.w), np.inf, np.float32)
        for m in self.at:
            if m[0] < self.w and m[1] < self.h:
                out[m[1], m[0]] = self.error(m)
        return out

    def triangles(self, tol):
        out = set()

        def go(t):
            if self.is_leaf(t):
                if all(self.present(p) for p in t):
                    out.add(frozenset(t))
            elif self.error(self.mid(t)) <= np.float32(tol):
                out.add(frozenset(t))
            else:
                for ch in self.children(t):
                    go(ch)
        for t in self.roots:
            go(t)
        return out


def _small_maps():
    rng = np.random.default_rng(5)
    for w, h in C.SMALL_SIZES:
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        smooth = (np.sin(x / np.float32(4)) + np.cos(y / np.float32(3))).astype(np.float32)
        holed = smooth.copy()
        holed[rng.random((h, w)) < 0.05] = R.invalid()
        yield "smooth-%dx%d" % (w, h), smooth
        yield "noise-%dx%d" % (w, h), rng.random((h, w)).astype(np.float32)
        yield "plane-%dx%d" % (w, h), C.plane(w, h)
        yield "holes-%dx%d" % (w, h), holed


def _tri_set(mesh):
    return {frozenset(map(tuple, t)) for t in mesh["nodes"].tolist()}


def test_the_restatement_equals_the_plain_bintree_walk():
    maps = list(_small_maps()) + [(n, m) for n, m in C.cases() if max(m.shape) <= C.TILE + 2 and not n.startswith("noise")]
    maps += [(n, m) for n, m in C.cases(("noise",)) if m.shape in ((5, 3), (C.TILE + 2, C.TILE + 1), (2, C.TILE + 2), (1, 5))]
    for name, height in maps:
        walk = Walk(height)
        err = R.errors(height)
        assert np.array_equal(err.view(np.uint32), walk.error_map().view(np.uint32)), name
        assert not np.isnan(err).any() and not np.signbit(err).any(), name
        for tol in WALK_TOLERANCES:
            mesh = R.mesh(height, err, tol)
            got = _tri_set(mesh)
            assert len(got) == len(mesh["nodes"]), name                      # no triangle twice
            assert got == walk.triangles(tol), (name, tol)


def _inner_nodes(tri):
    """the grid nodes a triangle covers, its border included, with their barycentric weights (float64)"""
    (x0, y0), (x1, y1), (x2, y2) = tri
    det = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    ys, xs = np.mgrid[min(y0, y1, y2):max(y0, y1, y2) + 1, min(x0, x1, x2):max(x0, x1, x2) + 1]
    l1 = ((xs - x0) * (y2 - y0) - (ys - y0) * (x2 - x0)) / det
    l2 = ((x1 - x0) * (ys - y0) - (y1 - y0) * (xs - x0)) / det
    l0 = 1.0 - l1 - l2
    inside = (l0 >= 0) & (l1 >= 0) & (l2 >= 0)
    return xs[inside], ys[inside], l0[inside], l1[inside], l2[inside]


def check_properties(name, height, err, tol, mesh):
    h, w = height.shape
    L = R.levels(w, h)
    nodes, vi = mesh["nodes"], mesh["vertex_index"]
    valid = height.view(np.uint32) != R.INVALID_BITS
    # the winding of "disparity mesh" item 3: (q - p) x (r - p) has negative z
    p, q, r = nodes[:, 0], nodes[:, 1], nodes[:, 2]
    assert ((q[:, 0] - p[:, 0]) * (r[:, 1] - p[:, 1]) - (q[:, 1] - p[:, 1]) * (r[:, 0] - p[:, 0]) < 0).all(), name
    edges = Counter()
    finite = np.isfinite(height[valid]).all()
    hmax = float(np.abs(height[valid].astype(np.float64)).max()) if valid.any() and finite else 0.0
    bound = 2 * L * (max(float(np.float32(tol)), 0.0) + 2.0 ** -22 * hmax)
    worst = 0.0
    for tri in nodes.tolist():
        tri = [tuple(c) for c in tri]
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            edges[frozenset((a, b))] += 1
            g = math.gcd(abs(b[0] - a[0]), abs(b[1] - a[1]))
            sx, sy = (b[0] - a[0]) // g, (b[1] - a[1]) // g
            for s in range(1, g):                                          # no kept vertex inside an edge: no T-junction
                assert vi[a[1] + s * sy, a[0] + s * sx] == R.NONE, (name, tol, tri)
        xs, ys, l0, l1, l2 = _inner_nodes(tri)
        assert valid[ys, xs].all(), (name, tol, tri)                         # every covered node is valid
        if finite and hmax < 1e30:
            z = [float(height[c[1], c[0]]) for c in tri]
            dev = np.abs(height[ys, xs].astype(np.float64) - (l0 * z[0] + l1 * z[1] + l2 * z[2]))
            worst = max(worst, float(dev.max()))
    assert worst <= bound, (name, tol, worst, bound)
    assert not edges or max(edges.values()) <= 2, name
    # the vertices: exactly the corners, ranked in raster order
    used = np.zeros((h, w), bool)
    used[nodes[:, :, 1].ravel(), nodes[:, :, 0].ravel()] = True
    assert np.array_equal(vi != R.NONE, used) and np.array_equal(vi[used], np.arange(used.sum(), dtype=np.uint32)), name
    assert np.array_equal(mesh["faces"], vi[nodes[:, :, 1], nodes[:, :, 0]]), name
    # the order: the doubled midpoint of the hypotenuse (q-r), then the apex p
    key = np.stack([q[:, 1] + r[:, 1], q[:, 0] + r[:, 0], p[:, 1], p[:, 0]], 1)
    assert (np.diff(np.lexsort(key.T[::-1])) == 1).all() or len(key) < 2, name
    assert len(np.unique(key, axis=0)) == len(key), name
    return worst


@pytest.mark.parametrize("content", sorted(C.CONTENTS))
def test_the_mesh_is_conforming_covers_valid_nodes_and_keeps_the_bound(content):
    for name, height in C.cases((content,)):
        if content == "noise" and height.size > 6 * 6 and height.shape not in ((C.TILE + 1, C.TILE + 2), (2 * C.TILE + 3, C.TILE)):
            continue  # the walk above and the GPU comparison run every size; the properties need not
        if height.size > 70 * 70 and (content not in ("noise", "relief", "holes") or height.shape == C.UPPER):
            continue  # a step of Python a triangle: the larger sizes run with three contents
        err = R.errors(height)
        last = None
        for tol in C.tolerances(err):
            mesh = R.mesh(height, err, tol, R.full_node_index(height))
            check_properties(name, height, err, tol, mesh)
            count = len(mesh["faces"])
            assert last is None or count <= last, (name, tol)                # the triangle set never grows with the tolerance
            last = count
            kept = mesh["kept"].astype(np.int64)
            assert (np.diff(kept) > 0).all() and (kept < (height.view(np.uint32) != R.INVALID_BITS).sum()).all(), name


def test_counts_at_the_ends_of_the_tolerance_range():
    for w, h in C.SMALL_SIZES + C.FEW_SIZES:
        height = C.relief(w, h)
        err = R.errors(height)
        mesh = R.mesh(height, err, -1.0)
        assert len(mesh["faces"]) == 2 * (w - 1) * (h - 1) and (mesh["vertex_index"] != R.NONE).all() == (w > 1 and h > 1), (w, h)
        assert np.array_equal(mesh["kept"], np.arange(w * h if w > 1 and h > 1 else 0, dtype=np.uint32))
    for side in (2, 3, 5, 9, 17, 33, 65):
        flat = C.plane(side, side)
        assert len(R.mesh(flat, R.errors(flat), 0.0)["faces"]) == 2, side
    for (w, h), n in (((33, 33), 2), ((20, 34), 147), ((17, 12), 46)):        # the border refinement the header accepts
        flat = C.plane(w, h)
        assert len(R.mesh(flat, R.errors(flat), 0.0)["faces"]) == n, (w, h)


def test_the_triangle_set_shrinks_by_merging_only():
    """a larger tolerance never adds a vertex: the kept nodes are nested"""
    for name, height in C.cases(("relief", "holes", "spike_tile_edge")):
        err = R.errors(height)
        finite = np.unique(err[np.isfinite(err)])
        tols = [-1.0] + [float(t) for t in finite[:: max(len(finite) // 6, 1)]] + [1e30]
        before = None
        for tol in tols:
            kept = R.mesh(height, err, tol)["vertex_index"] != R.NONE
            assert before is None or not (kept & ~before).any(), (name, tol)
            before = kept
