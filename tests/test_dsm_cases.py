"""The surface-model cases test something: on the numpy reference alone (no GPU) every case of tests/dsm_cases.py exercises what
it claims, so that tests/test_gpu_dsm.py, which compares the kernels with the same reference, cannot pass on cases that miss
their point."""
import numpy as np
import pytest

import dsm_cases as C
import dsm_ref as D

f32 = np.float32


def test_the_key_is_the_float_order_with_minus_zero_below_plus_zero():
    v = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    k = D.key(v)
    assert (np.diff(k) > 0).all() and k[3] == -1 and k[4] == 0


@pytest.mark.parametrize("name", sorted(C.RASTERIZE))
def test_rasterize_case_has_occupied_and_empty_cells_and_a_brute_force_agrees(name):
    c = C.RASTERIZE[name]
    for rule in (D.MAX, D.MIN):
        height, source, count = C.rasterize_reference(name, rule)
        occupied = D.bits(height) != D.INVALID_BITS
        assert np.array_equal(occupied, count > 0) and np.array_equal(occupied, source != D.NONE)
        if not c.exempt:
            assert occupied.any() and not occupied.all(), name
        if len(c.points) <= 5000:   # point by point, in index order: a later point wins only with a strictly better key
            loc = D.locate(c.points, c.frame)
            best = {}
            for t in np.nonzero(loc["inside"])[0]:
                cell, k = int(loc["cell"][t]), int(D.key(loc["z"][t:t + 1])[0])
                if cell not in best or (k > best[cell][0] if rule == D.MAX else k < best[cell][0]):
                    best[cell] = (k, t)
            assert {int(x) for x in np.nonzero(occupied.ravel())[0]} == set(best)
            for cell, (k, t) in best.items():
                assert source.ravel()[cell] == t and D.bits(height).ravel()[cell] == D.bits(loc["z"])[t]


def test_the_edge_cases_are_the_edges_they_name():
    loc = lambda name: D.locate(C.RASTERIZE[name].points, C.RASTERIZE[name].frame)   # noqa: E731
    # ties: equal keys at different indices in one cell, and the smallest index wins under both rules
    for name in ("equal_heights", "one_cell_equal"):
        l = loc(name)
        height, source, count = C.rasterize_reference(name, D.MAX)
        ties = 0
        for cell in np.nonzero(count.ravel() > 1)[0][:50]:
            members = np.nonzero(l["cell"] == cell)[0]
            winners = members[D.key(l["z"][members]) == D.key(l["z"][members]).max()]
            ties += len(winners) > 1
            assert source.ravel()[cell] == winners.min()
        assert ties > 0, name
    assert C.rasterize_reference("one_cell_equal", D.MIN)[1][2, 3] == 0 and C.rasterize_reference("one_cell_equal", D.MAX)[2][2, 3] == 100000
    h_max, s_max, _ = C.rasterize_reference("one_cell_distinct", D.MAX)
    assert 0 < s_max[2, 3] < 99999 and h_max[2, 3] == C.RASTERIZE["one_cell_distinct"].points[:, 2].max()
    # +0 and -0 in one cell: MAX takes +0 (index 0), MIN takes -0 (index 1); in the next cell -0 comes first
    zmax, zmin = C.rasterize_reference("signed_zeros", D.MAX), C.rasterize_reference("signed_zeros", D.MIN)
    assert D.bits(zmax[0])[0, 0] == 0 and zmax[1][0, 0] == 0 and D.bits(zmin[0])[0, 0] == 0x80000000 and zmin[1][0, 0] == 1
    assert D.bits(zmax[0])[0, 1] == 0 and zmax[1][0, 1] == 5 and D.bits(zmin[0])[0, 1] == 0x80000000 and zmin[1][0, 1] == 4
    assert (C.rasterize_reference("negative_heights", D.MAX)[0][C.rasterize_reference("negative_heights", D.MAX)[2] > 0] < 0).all()
    # the borders: every u and v an exact integer, u == w and v == h among them and outside
    l, fr = loc("borders"), C.RASTERIZE["borders"].frame
    assert np.array_equal(l["u"], l["fi"]) and np.array_equal(l["v"], l["fj"])
    assert (l["u"] == fr.w).any() and (l["v"] == fr.h).any() and not l["inside"][(l["u"] == fr.w) | (l["v"] == fr.h)].any()
    assert l["inside"][(l["u"] == fr.w - 1) & (l["v"] == fr.h - 1)].all()
    # a denormal cell: u an exact integer again
    l, fr = loc("denormal_cell"), C.RASTERIZE["denormal_cell"].frame
    assert 0 < fr.cell < np.finfo(np.float32).tiny and np.array_equal(l["u"], l["fi"]) and (l["u"] == fr.w).any() and (l["u"] < 0).any()
    # a = -0 is inside cell 0; the largest float below 0 is outside
    l = loc("minus_zero_a")
    assert D.bits(l["a"])[0] == 0x80000000 and D.bits(l["fi"])[0] == 0x80000000 and l["inside"][0] and l["cell"][0] == 0
    l = loc("just_below_zero_a")
    assert D.bits(l["a"])[0] == 0x80000001 and l["fi"][0] == -1 and not l["inside"][0] and l["inside"][1]
    # huge coordinates: outside, or a finite height of 1e30 that is inside
    l = loc("huge")
    assert list(l["inside"]) == [False, False, False, False, True, True, False] and abs(l["z"][4]) == f32(1e30)
    l = loc("nan_inf")
    assert list(l["inside"]) == [False] * 7 + [True]
    l = loc("zero_points")   # the three zero points would lie in cell (1, 1)
    assert list(l["inside"]) == [False, False, False, True, True] and l["cell"][0] == -1 and (l["fi"][:3] == 1).all()
    l = loc("z_overflows")
    assert np.isinf(l["z"][0]) and np.isinf(l["z"][2]) and list(l["inside"]) == [False, True, False] and (l["fi"][[0, 2]] >= 0).all()
    fr = C.RASTERIZE["skew_frame"].frame
    assert abs(np.dot(fr.ex, fr.ey)) > 0.1 and abs(np.dot(fr.ex, fr.ez)) > 0.1 and 100 < loc("skew_frame")["inside"].sum() < 4900


def test_the_runs_cross_a_wave_and_a_block():
    for name in ("runs_cross_waves", "runs_longer_than_a_wave"):
        cell = D.locate(C.RASTERIZE[name].points, C.RASTERIZE[name].frame)["cell"]
        assert (cell >= 0).all()
        for edge in (64, 256, 512, 1024):   # lane 63 -> 0, and a block's last -> first thread
            assert cell[edge - 1] == cell[edge], (name, edge)
    cell = D.locate(C.RASTERIZE["runs_longer_than_a_wave"].points, C.RASTERIZE["runs_longer_than_a_wave"].frame)["cell"]
    assert (cell[64:128] == cell[64]).all()   # a whole wave in one cell


def test_the_order_cases_are_one_cloud_and_give_one_map():
    base = C.RASTERIZE["order_given"]
    assert len(np.unique(base.points[:, 2])) == len(base.points)   # distinct heights: the winner does not depend on the index
    for rule in (D.MAX, D.MIN):
        height, source, count = C.rasterize_reference("order_given", rule)
        for kind in ("sorted", "reversed", "shuffled"):
            order = C.order_of(kind)
            assert sorted(order) == list(range(len(order))) and not np.array_equal(order, np.arange(len(order)))
            h2, s2, c2 = C.rasterize_reference("order_" + kind, rule)
            assert h2.tobytes() == height.tobytes() and np.array_equal(c2, count)
            back = np.where(s2 == D.NONE, D.NONE, order[np.minimum(s2, len(order) - 1)].astype(np.uint32))
            assert np.array_equal(back, source)
    cell = D.locate(C.RASTERIZE["order_sorted"].points, base.frame)["cell"]
    inside = cell[cell >= 0]
    assert (np.diff(inside) >= 0).all()


@pytest.mark.parametrize("name", sorted(C.FUSE))
def test_fuse_case_against_a_cell_by_cell_restatement(name):
    c = C.FUSE[name]
    out, views = C.fuse_reference(name)
    stack = np.stack([D.bits(m) for m in c.maps]).reshape(len(c.maps), -1)
    cells = stack.shape[1]
    pick = np.random.RandomState(3).permutation(cells)[:400]
    for cell in list(range(min(cells, 12))) + list(pick):
        vals = [b for b in stack[:, cell] if b != D.INVALID_BITS]
        vals.sort(key=lambda b: int(D.key(np.array([b], np.uint32).view(np.float32))[0]))
        want = D.INVALID_BITS
        if vals and len(vals) >= c.min_views:
            lo, hi = (np.array([b], np.uint32).view(np.float32)[0] for b in (vals[0], vals[-1]))
            with np.errstate(all="ignore"):
                if hi - lo <= f32(c.max_spread):
                    want = vals[{D.FUSE_MIN: 0, D.FUSE_MEDIAN: (len(vals) - 1) // 2, D.FUSE_MAX: len(vals) - 1}[c.rule]]
        assert D.bits(out).ravel()[cell] == want and views.ravel()[cell] == len(vals), (name, cell)


def test_the_fuse_cases_hold_what_they_claim():
    for (w, h) in C.FUSE_SIZES[1:]:
        for m in (1, 2, 3, 8):
            c = C.FUSE["%dx%d/m%d/rule1/spread1" % (w, h, m)]
            out, views = C.fuse_reference("%dx%d/m%d/rule1/spread1" % (w, h, m))
            assert list(views.ravel()[:m + 1]) == list(range(m + 1))                  # every n from 0 to m
            survive = D.bits(out) != D.INVALID_BITS
            assert survive.any() and not survive.all()
            if m >= 2:
                stack = np.stack(c.maps)
                valid = np.stack([D.bits(x) != D.INVALID_BITS for x in c.maps])
                with np.errstate(all="ignore"):
                    lo = np.where(valid, stack, np.inf).min(0)
                    hi = np.where(valid, stack, -np.inf).max(0)
                    spread = hi - lo
                assert (spread[valid.sum(0) >= 2] == 1.0).any()                       # maxSpread exactly hi - lo: survives
                assert (survive & (spread == 1.0)).any() and not (survive & (spread > 1.0)).any()
                assert np.isnan(spread[valid.sum(0) >= 2]).any()                      # inf - inf among the valid entries
            all_views = C.fuse_reference("%dx%d/m%d/all_views" % (w, h, m))
            ok = D.bits(all_views[0]) != D.INVALID_BITS
            assert ok.any() and (all_views[1][ok] == m).all()
    assert (D.bits(C.fuse_reference("all_invalid")[0]) == D.INVALID_BITS).all() and not C.fuse_reference("all_invalid")[1].any()
    twice = C.FUSE["same_map_twice"]
    assert twice.maps[0] is twice.maps[2] is twice.maps[3]
    assert (C.fuse_reference("same_map_twice")[1] >= 3).any()


def test_the_points_cases_and_the_tilted_plane():
    for name, (height, fr) in C.POINTS.items():
        pts = D.points(height, fr)
        valid = D.bits(height) != D.INVALID_BITS
        assert len(pts) == valid.sum() and (name == "all_holes") == (len(pts) == 0)
        if len(pts) and "skew" not in name:   # orthonormal frames: the points fall back into their own cells, in raster order
            loc = D.locate(pts, fr)
            assert np.array_equal(loc["cell"], np.nonzero(valid.ravel())[0])
    height, fr = C.tilted_plane()
    assert np.allclose(np.cross(fr.ex, fr.ey), -fr.ez)   # (ex, ey, -ez) right-handed
    import mesh_ref as M
    vi, cells, n = M.mesh(height, 1, np.inf)
    pts = D.points(height, fr)
    assert n == len(pts) and np.array_equal(vi[vi != M.NONE], np.arange(n))   # the mesh's numbering is the points' order
    normals = M.normals(pts, vi, cells)
    dots = normals @ fr.ez
    assert (np.abs(normals).sum(1) > 0).sum() > 100 and (dots[np.abs(normals).sum(1) > 0] > 0).all()
