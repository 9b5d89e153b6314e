"""The mesh-render cases test something, and the reference keeps its own invariants: proved on the numpy restatement alone
(tests/render_ref.py), without a GPU.  tests/test_gpu_render.py holds csrc/render.hip to the same reference on the same cases."""
from fractions import Fraction

import numpy as np
import pytest

import render_cases as C
import render_ref as R


def covers(c, name):
    """every (id, x, y, v) the reference's scatter touches, next to its outputs"""
    seen = []
    out = R.render(c.points, c.grey, c.vertex_index, c.cells, c.view, c.max_extent,
                   on_cover=lambda ids, xs, ys, v: seen.extend(zip(ids.tolist(), xs.tolist(), ys.tolist(), v.tolist())))
    for k, a in C.reference(name).items():
        assert np.array_equal(out[k], a), (name, k)
    return out, seen


def corners_of(c):
    """-> a function id -> the exact projected corners of a triangle as Fractions of a pixel, from the reference's fixed-point vertices"""
    fx, fy, _, usable = R.project(c.points, c.view)
    tris = dict(R.triangles(c.vertex_index, c.cells))
    cache = {}

    def corners(tid):
        if tid not in cache:
            assert all(usable[k] for k in tris[tid])
            cache[tid] = [(Fraction(int(fx[k]), 256), Fraction(int(fy[k]), 256)) for k in tris[tid]]
        return cache[tid]
    return corners


def inside(p, q, r, x, y):
    """exact rational arithmetic: (x, y) in the closed triangle, whichever way it winds"""
    e = lambda a, b: (b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0])  # noqa: E731
    s = [e(p, q), e(q, r), e(r, p)]
    return all(v >= 0 for v in s) or all(v <= 0 for v in s)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_a_drawn_pixel_lies_in_its_triangle_and_holds_the_greatest_v(name):
    c = C.CASES[name]
    out, seen = covers(c, name)
    best = {}
    for tid, x, y, v in seen:
        k = (y, x)
        if k not in best or (v, -tid) > (best[k][0], -best[k][1]):
            best[k] = (v, tid)
    hit = out["triangle"] != R.NONE
    assert set(zip(*np.nonzero(hit))) == set(best)
    assert ((out["depth"] != R.INVALID_BITS) == hit).all() and (out["shade"][~hit] == 0).all()
    corners = corners_of(c)
    for (y, x), (v, tid) in best.items():
        assert int(out["triangle"][y, x]) == tid
        assert out["depth"][y, x] == (np.float32(1.0) / np.float32(v)).view(np.uint32)
        assert inside(*corners(tid), x, y), (name, tid, x, y)
    # a centre that no triangle claims lies in no drawn triangle: the coverage misses nothing
    if name.split("/")[0] in ("one_triangle", "shared_edge", "negative_area", "off_image", "cell_bytes", "view_65x3"):
        drawn = {tid for tid, *_ in seen}
        for y, x in zip(*np.nonzero(~hit)):
            assert not any(inside(*corners(tid), x, y) for tid in drawn), (name, x, y)


@pytest.mark.parametrize("name", ["coincident", "near_hides_far", "cell_bytes", "off_image", "fold", "fold/selected", "extent/8", "shared_edge/tilted"])
def test_the_order_of_the_triangles_changes_nothing(name):
    c, want = C.CASES[name], C.reference(name)
    n = len(R.triangles(c.vertex_index, c.cells))
    assert n >= 2
    for order in (list(range(n))[::-1], np.random.RandomState(5).permutation(n).tolist()):
        got = R.render(c.points, c.grey, c.vertex_index, c.cells, c.view, c.max_extent, order=order)
        for k in want:
            assert np.array_equal(got[k], want[k]), (name, k)


def counts(name):
    return C.reference(name)["counts"].tolist()


def test_the_edge_cases_are_what_they_claim():
    ref = C.reference
    # centres on the edges and corners: the closed triangle (1,1) (1,5) (5,5) holds 15 centres, 5 of them on each edge
    one = ref("one_triangle/on_centres")
    assert counts("one_triangle/on_centres") == [1, 0, 0] and int((one["triangle"] == 0).sum()) == 15
    assert all(one["triangle"][y, x] == 0 for x, y in ((1, 1), (1, 5), (5, 5), (3, 3), (1, 3), (3, 5)))
    assert one["shade"][1, 1] == 10 and one["shade"][5, 1] == 170 and one["shade"][5, 5] == 250 and one["shade"][3, 3] == 130   # a, c, d and the middle of a-d
    assert int((ref("one_triangle/other_diagonal")["triangle"] == 0).sum()) == 15 and ref("one_triangle/other_diagonal")["triangle"][5, 5] == R.NONE
    # the shared edge: both triangles cover its centres with equal v, the smaller id has them
    for name, diag in (("shared_edge/ad", [(k, k) for k in range(1, 7)]), ("shared_edge/bc", [(7 - k, k) for k in range(1, 7)])):
        tri = ref(name)["triangle"]
        assert counts(name) == [2, 0, 0] and all(tri[y, x] == 0 for x, y in diag) and (tri == 1).sum() == 15 and (tri == 0).sum() == 21
    tilted = ref("shared_edge/tilted")
    assert len(np.unique(tilted["depth"][tilted["triangle"] != R.NONE])) > 4 and {0, 1} <= set(tilted["triangle"].ravel().tolist())
    co = ref("coincident")                   # ids 0, 1 lie under 4, 5 and (with the other diagonal) 8, 9: only 0 and 1 are seen
    assert counts("coincident") == [6, 0, 0] and set(co["triangle"].ravel().tolist()) == {0, 1, int(R.NONE)} and co["shade"].max() >= 200
    hid = ref("near_hides_far")              # the depths are the planes' z, the nearest quad in front
    assert set(np.round(hid["depth"][hid["triangle"] != R.NONE].view(np.float32), 5).tolist()) == {1.5, 2.0}     # the weights' roundings: a few ulp
    assert round(float(hid["depth"].view(np.float32)[3, 3]), 5) == 1.5 and hid["triangle"][3, 3] in (4, 5) and hid["triangle"][1, 6] in (0, 1)
    # a corner that is not usable takes its triangles with it: b is in both triangles of a b-c cell, d in both of an a-d cell
    for name in C.CASES:
        if name.startswith("unusable/"):
            assert counts(name) == [0, 0, 4], name
            assert (ref(name)["triangle"] == R.NONE).all(), name
    assert counts("usable/w_2p60") == [2, 0, 0] and (ref("usable/w_2p60")["triangle"] == 0).any()
    assert counts("usable/sx_2p20") == [2, 2, 0]      # T0 = (a, c, d) of the first and T1 = (a, d, b) of the second stay small
    for e in (1, 8, 64):
        assert counts("extent/%d" % e) == [2, 2, 0], e
        assert set(ref("extent/%d" % e)["triangle"].ravel().tolist()) == {0, 8, int(R.NONE)}
    assert counts("zero_area") == [0, 0, 4] and (ref("zero_area")["triangle"] == R.NONE).all()
    neg = ref("negative_area")
    fx, fy, _, _ = R.project(C.CASES["negative_area"].points, C.CASES["negative_area"].view)
    # with x to the right and y down the mesh's own winding has A < 0 and the mirror image A > 0: both signs are drawn
    assert R.edge(*[int(v) for v in (256, 256, 256, 1536, 1536, 1536)]) < 0 < R.edge(fx[0], fy[0], fx[2], fy[2], fx[3], fy[3])
    assert counts("negative_area") == [4, 0, 0] and (neg["triangle"][1:7, 1:7] <= 1).all() and neg["depth"][3, 3] == np.float32(1.0).view(np.uint32)
    assert counts("off_image") == [12, 0, 0]          # six half off, the seven wholly off neither drawn nor counted
    off = ref("off_image")["triangle"]
    assert off[0, 0] != R.NONE and off[7, 7] != R.NONE and off[0, 7] == R.NONE
    assert (R.project(C.CASES["off_image"].points, C.CASES["off_image"].view)[0] < 0).any()
    assert counts("between_centres") == [2, 0, 0] and (ref("between_centres")["triangle"] != R.NONE).sum() == 1
    assert ref("view_1x1")["triangle"].tolist() == [[4]] and counts("view_1x1") == [3, 0, 0]
    flat = ref("view_65x3")
    assert flat["triangle"].shape == (3, 65) and (flat["triangle"] != R.NONE).all() and len(np.unique(flat["triangle"])) > 20
    bytes_seen = sorted(set(C.CASES["cell_bytes"].cells[::2, 0].tolist()))
    assert bytes_seen == [0, 1, 2, 3, 5, 6, 7] and counts("cell_bytes") == [8, 0, 0]
    assert counts("stale_index") == [2, 0, 2] and counts("no_vertex") == [1, 0, 3] and counts("no_points") == [0, 0, 0]
    for name in ("grid_1x1", "grid_5x1", "grid_1x5", "grid_0x0", "no_points"):
        r = ref(name)
        assert counts(name) == [0, 0, 0] and (r["depth"] == R.INVALID_BITS).all() and (r["triangle"] == R.NONE).all() and (r["shade"] == 0).all()


def test_the_fold_hides_ground_and_the_extent_bites():
    c = C.CASES["fold"]
    seen = {}
    out = R.render(c.points, c.grey, c.vertex_index, c.cells, c.view, c.max_extent,
                   on_cover=lambda ids, xs, ys, v: [seen.setdefault((y, x), set()).add(t) for t, x, y in zip(ids.tolist(), xs.tolist(), ys.tolist())])
    deep = [k for k, ids in seen.items() if len({t // 2 for t in ids}) >= 3]      # three cells and more behind one pixel: a fold, not a shared edge
    assert len(deep) > 20
    drawn, large, unusable = out["counts"].tolist()
    assert drawn > 4000 and large == 0 and unusable == 0
    hit = out["triangle"] != R.NONE
    assert 0.4 < hit.mean() < 1.0 and not hit.all()                                # the mesh's holes and the margin show the background
    small = C.reference("fold/small_extent")["counts"].tolist()
    assert small[1] > 0 and small[0] < drawn <= small[0] + small[1]                 # the tower's flanks are longer than two pixels; the size is judged before the image's bounds
    sel = C.reference("fold/selected")["counts"].tolist()
    assert 0 < sel[0] < drawn and sel[2] == 0                                       # select clears the bits: nothing is left to skip
    assert (C.CASES["fold/selected"].vertex_index == R.NONE).sum() > (c.vertex_index == R.NONE).sum()


def test_the_residual_marks_exactly_the_undrawn_pixels():
    r = C.reference("fold")
    image = np.random.RandomState(9).randint(0, 256, r["shade"].shape).astype(np.uint8)
    res = R.residual(image, r["shade"], r["depth"])
    holes = r["depth"] == R.INVALID_BITS
    assert holes.any() and (res[holes] == R.INVALID_BITS).all() and not (res[~holes] == R.INVALID_BITS).any()
    want = image.astype(np.int64) - r["shade"].astype(np.int64)
    assert np.array_equal(res.view(np.float32)[~holes], want[~holes].astype(np.float32))
    s = R.stats(res)
    assert s["coverage"] == (~holes).mean() and s["rms"] > 0 and s["nmad"] > 0
