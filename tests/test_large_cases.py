"""The cases of tests/large_cases.py test something, shown without a GPU: every cap is the one in the kernels' sources, every
kernel of the list launches that many blocks of 256 threads and strides by its whole grid, every size lies past its threshold,
and the references (the plain restatements the small cases are held to) put into the later trips what each case claims: pixels
the left-right check alone removes, interior census codes, tile-local roots that must hop to pixel 0, speckles astride a seam,
holes that fill and holes that stay, a tower only one load sees, triangles that win and lose, the forced pairs of the subtraction.
tests/test_gpu_large.py then holds the kernels to the same references on the same cases."""
import re

import numpy as np
import pytest

import large_cases as L


@pytest.mark.parametrize("name", sorted(L.CAPS))
def test_the_caps_are_the_sources(name):
    assert L.CAP[name] == L.read_constant(*L.CAPS[name]) and L.THRESHOLD[name] == L.CAP[name] * 256
    assert L.CAP == dict(stereo=2048, census=8192, filter=4096, ortho=2048, render=8192, subtract=65536)   # what DESIGN.md's table says


def test_the_loops_and_launches_are_the_sources():
    """a thread's first element is blockIdx.x * 256 + threadIdx.x and its stride the whole grid, in every kernel of the list; each
    is launched with the capped grid and 256 threads"""
    s = L.source("stereo.hip")
    for kernel in ("k_stereo_fill", "k_stereo_lr", "k_census"):
        body = s[s.index("void %s(" % kernel):]
        assert re.search(r"for \(size_t (\w) = \(size_t\)blockIdx\.x \* 256 \+ threadIdx\.x; \1 < n; \1 \+= \(size_t\)gridDim\.x \* 256\) \{", body[:600]), kernel
    assert len(re.findall(r"hipLaunchKernelGGL\(k_stereo_fill, dim3\(fillBlocks\), dim3\(256\)", s)) == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(k_stereo_lr, dim3\(fillBlocks\), dim3\(256\)", s)) == 1
    assert "unsigned fillBlocks = (unsigned)((n + 255) / 256);" in s and "unsigned blocks = (unsigned)((n + 255) / 256);" in s
    f = L.source("disparity_filter.hip")
    loop = "for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {"
    for kernel in ("k_cc_roots", "k_cc_sizes", "k_speckle_apply", "k_fill_select"):
        body = f[f.index("void %s(" % kernel):]
        assert loop in body[:700], kernel
        assert len(re.findall(r"hipLaunchKernelGGL\(%s, dim3\(capped_blocks\(n\)\), dim3\(256\)" % kernel, f)) == 1, kernel
    assert f.count(loop) == 4
    o = L.source("ortho.hip")
    assert "const uint32_t stride = gridDim.x * 256u;" in o and "(unsigned long long)c0 + (unsigned long long)t * stride;" in o
    assert "for (uint32_t c0 = blockIdx.x * 256u + threadIdx.x; c0 < cells; c0 += 4u * stride) {" in o
    assert "hipLaunchKernelGGL(k_ortho_top, dim3(top_blocks(cells)), dim3(256)" in o and L.ORTHO_LOADS == 4
    r = L.source("render.hip")
    assert "for (uint32_t base = blockIdx.x * 256u; base < numCells; base += gridDim.x * 256u) {" in r
    assert "hipLaunchKernelGGL(k_render_scatter, dim3(blocks < kScatterBlocks ? blocks : kScatterBlocks), dim3(256)" in r
    t = L.source("terrain.hip")
    assert "for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {" in t[t.index("void k_subtract("):][:300]


def test_the_sizes_lie_past_their_thresholds():
    T = L.THRESHOLD
    assert (L.STEREO_W, L.STEREO_H) == (1031, 770) and L.STEREO_W * L.STEREO_H > T["stereo"]
    assert (L.CENSUS_W, L.CENSUS_H) == (2049, 1100) and L.CENSUS_W * (L.CENSUS_H - L.CENSUS_TAIL) > T["census"] >= L.CENSUS_W * (L.CENSUS_H - L.CENSUS_TAIL - 1)
    assert (L.FILTER_W, L.FILTER_H) == (1025, 1200) and (L.TILES_X, L.TILES_Y) == (17, 75) and L.FILTER_H % L.S.TILE_H == 0
    assert L.LATER_ROW * L.FILTER_W >= T["filter"] > (L.LATER_ROW - 1) * L.FILTER_W and L.LATER_ROW < L.BAR_ROW - 40
    assert L.FILTER_H == 9 * L.FILL_STRIP + 48                                      # ten strips of the fill's march
    assert L.ORTHO_SIDE == 1449 and L.ORTHO_SIDE ** 2 > 4 * T["ortho"] >= (L.ORTHO_SIDE - 1) ** 2
    assert (L.RENDER_GW, L.RENDER_GH) == (1450, 1449) and L.RENDER_CELLS > T["render"] > L.RENDER_CELLS - (L.RENDER_GW - 1)
    assert 0 < L.RENDER_FIRST_LATE and L.RENDER_FIRST_LATE + 6 < L.RENDER_GW - 1
    assert (L.SUBTRACT_W, L.SUBTRACT_H) == (4097, 4096) and L.SUBTRACT_W * L.SUBTRACT_H > T["subtract"] > L.SUBTRACT_W * (L.SUBTRACT_H - 1)
    # the stereo matches: the candidates pass the second round of the compaction's 256-thread scan (tests/glue_cases.py)
    import glue_cases as G
    assert L.STEREO_W * L.STEREO_H > G.N_SCAN_ROUND2 == 524288 + 513


# ---- 1. block matching and SGM
def test_the_stereo_case_puts_every_kind_of_pixel_into_the_later_trips():
    c, ref = L.stereo_case(), L.stereo_reference()
    late = L.later("stereo", (c.h, c.w))
    assert int((ref["valid_before_lr"] & ~ref["valid"] & late).sum()) >= 100     # only k_stereo_lr invalidates these
    assert int((ref["valid"] & late).sum()) > 100000                             # ... and leaves these
    border = np.ones((c.h, c.w), bool)
    border[c.r:c.h - c.r, c.r:c.w - c.r] = False
    assert (border & late).sum() > c.w and not ref["has"][border].any()          # only k_stereo_fill writes these
    bits = ref["disparity"].view(np.uint32)
    assert (bits[border] == 0x7FC00000).all() and (ref["cost"][border] == 0xFFFFFFFF).all()
    assert len(L.matches_reference()) == int(ref["valid"].sum()) > 524288 + 513


def test_the_sgm_case_runs_long_diagonals_into_the_later_trips():
    c, ref = L.stereo_case(), L.sgm_reference()
    late = L.later("stereo", (c.h, c.w))
    assert min(c.w, c.h) - 2 * c.r == 768                                        # steps of the longest diagonal path
    assert int((ref["valid_before_lr"] & ~ref["valid"] & late).sum()) >= 100 and int((ref["valid"] & late).sum()) > 100000
    assert (ref["disparity"].view(np.uint32) != L.stereo_reference()["disparity"].view(np.uint32)).sum() > 1000   # the penalties did something


# ---- 2. census
@pytest.mark.parametrize("c", L.CENSUS_RADII)
def test_the_second_trip_of_the_census_holds_interior_codes(c):
    want = L.census_reference(c)
    late = L.later("census", want.shape)
    assert late[-L.CENSUS_TAIL:].all() and not late[:-L.CENSUS_TAIL - 1].any()   # the last 76 rows, and a part of the row before
    inner = np.zeros(want.shape, bool)
    inner[c:-c, c:-c] = True
    assert (want[late & inner] != 0).sum() > 100000 and (want[~inner] == 0).all() and (late & ~inner).sum() > 0
    assert int(want[late].max()).bit_length() == (2 * c + 1) ** 2 - 1            # the code's last bit is met there


# ---- 3. components, speckles, fill
def _sorted_sizes(labels, sizes):
    roots = labels == np.arange(labels.size, dtype=np.uint32).reshape(labels.shape)
    return sorted(sizes[roots].tolist())


@pytest.mark.parametrize("name", ["serpentine", "serpentine_t", "comb_bottom"])
def test_one_component_over_every_tile_with_its_closed_form(name):
    k = L.component_case(name)
    labels, sizes = L.component_reference(name)
    valid = L.S.INVALID.view(np.uint32) != k.d.view(np.uint32)
    assert _sorted_sizes(labels, sizes) == k.sizes and len(k.sizes) == 1 and k.sizes[0] == valid.sum()
    assert (labels[valid] == 0).all() and (sizes[valid] == k.sizes[0]).all()     # the root is pixel 0: every other tile-local root hops
    h, w = k.d.shape
    assert w * h > L.THRESHOLD["filter"]
    late = L.later("filter", (h, w))
    tiles_late = {(y // L.S.TILE_H, x // L.S.TILE_W) for y, x in zip(*np.nonzero(valid & late))}
    later_row = L.THRESHOLD["filter"] // w + 1           # 1024, and 874 of the transpose
    assert len(tiles_late) >= (h - later_row) // L.S.TILE_H * (w // L.S.TILE_W) > 100   # valid pixels in every tile of the later trips
    if name == "comb_bottom":
        assert k.sizes[0] == 513 * 1199 + 1025 and not valid[:-1, 1::2].any() and valid[-1].all()   # joined in the last row only
    if name == "serpentine":
        assert k.sizes[0] == 600 * 1025 + 599


def test_the_noise_map_has_speckles_and_survivors_wholly_inside_the_later_trips():
    k = L.component_case("noise")
    labels, sizes = L.component_reference("noise")
    valid = k.d.view(np.uint32) != L.S.INVALID.view(np.uint32)
    assert 0.09 < 1.0 - valid.mean() < 0.11 and k.max_diff == 0.0
    first_row = labels // np.uint32(L.FILTER_W)          # of a component: its root is its smallest raster index
    inside = valid & (first_row >= L.LATER_ROW)
    assert (inside & (sizes <= L.MAX_SPECKLE)).sum() > 1000 and (inside & (sizes > L.MAX_SPECKLE)).sum() > 1000
    # the bars: sizes 11, 12 and 13, each astride a tile seam, twice
    got = []
    for j, n in enumerate(L.BAR_SIZES):
        y, x = L.BAR_ROW - 30 + 3 * j, L.BAR_COLUMN - 6
        assert (sizes[y, x:x + n] == n).all() and x < L.BAR_COLUMN < x + n and L.BAR_COLUMN % L.S.TILE_W == 0
        y, x = L.BAR_ROW - 6, L.BAR_COLUMN - 9 + 3 * j
        assert (sizes[y:y + n, x] == n).all() and y < L.BAR_ROW < y + n and L.BAR_ROW % L.S.TILE_H == 0 and y > L.LATER_ROW
        got += [n, n]
    assert sorted(got) == sorted(2 * list(L.BAR_SIZES))
    # components larger than a tile exist, so counts are summed over tiles in the later trips
    assert int(sizes[L.LATER_ROW:].max()) > 40
    d, cost = L.speckle_reference()
    removed = valid & (d.view(np.uint32) == L.S.INVALID.view(np.uint32))
    assert (removed == (valid & (sizes <= L.MAX_SPECKLE))).all() and (cost[removed] == 0xFFFFFFFF).all()
    assert (cost[valid & ~removed] == L.speckle_cost()[valid & ~removed]).all() and removed[L.LATER_ROW:].sum() > 1000


def test_the_fill_map_fills_and_leaves_holes_in_the_later_trips():
    import fill_ref as F
    d = L.fill_map()
    hole = d.view(np.uint32) == F.INVALID
    assert 0.04 < hole.mean() <= L.FILL_SHARE
    assert hole[:, L.FILL_COLUMN].all()                                           # a whole column: carried through all ten strips
    band = hole[L.FILL_BAND[0]:L.FILL_BAND[1]]
    assert L.FILL_BAND[0] < 8 * L.FILL_STRIP < L.FILL_BAND[1] and band[:, :7].all() and band[:, 8:].all() and not band[:, 7].any()
    assert len(set(np.unique(d[~hole].view(np.uint32)).tolist())) >= 12           # rich values, the foreign NaN among them
    for call, p in enumerate(L.fill_calls()):
        out, filled = L.fill_reference(call)
        stays = hole & (filled == 0)
        assert (filled[~hole] == 0).all() and (out.view(np.uint32)[~hole] == d.view(np.uint32)[~hole]).all()
        assert (filled[L.LATER_ROW:] == 1).sum() > 1000, call
        if p["max_gap"] == 7:   # the middle of the band and of the block lie out of reach
            assert stays[L.LATER_ROW:].sum() > 500 and stays[8 * L.FILL_STRIP + 1, 20:].all()
            assert stays[(L.FILL_BLOCK[0] + L.FILL_BLOCK[1]) // 2, (L.FILL_BLOCK[2] + L.FILL_BLOCK[3]) // 2]
        else:                   # no limit: the vertical and diagonal rays reach across the band; a hole stays only for want of hits
            assert filled[8 * L.FILL_STRIP + 1, 20:-20].all()
    a, b = L.fill_reference(0), L.fill_reference(1)
    assert (a[1] != b[1]).sum() > 1000                                            # the two calls differ


# ---- 4. ortho top
@pytest.mark.parametrize("variant", L.ORTHO_VARIANTS)
def test_only_one_load_sees_the_tower_and_it_hides_cells(variant):
    j0, j1, i0, i1 = L.tower_cells(variant)
    first, last = j0 * L.ORTHO_SIDE + i0, (j1 - 1) * L.ORTHO_SIDE + i1 - 1
    if variant == "trip2":
        assert first >= L.ORTHO_LOADS * L.ORTHO_RANGE
    else:
        t = L.ORTHO_VARIANTS.index(variant)
        assert t * L.ORTHO_RANGE <= first and last < (t + 1) * L.ORTHO_RANGE
    c, flat = L.ortho_case(variant), L.ortho_case(variant, tower=False)
    assert float(np.nanmax(flat.height)) <= 0.2 and float(np.nanmax(c.height)) == L.TOWER_HEIGHT
    rest = np.ones(c.height.shape, bool)
    rest[j0:j1, i0:i1] = False
    assert float(np.nanmax(np.where(rest, c.height, 0))) <= 0.2                   # nothing else is high: `top` hangs on those cells alone
    with_tower, without = L.ortho_reference(variant), L.ortho_reference(variant, tower=False)
    seen, seen_flat = with_tower["seen"] != 0, without["seen"] != 0
    inside = with_tower["inside"][0]
    assert 10000 < inside.sum() < 200000 and inside[j0:j1, i0:i1].any()           # a narrow view, on the tower
    # the cells a too-low `top` would call visible: seen over the flat map, hidden behind the tower
    assert int(seen_flat.sum()) - int(seen.sum()) >= 100 and int((seen_flat & ~seen & rest).sum()) >= 100
    assert seen.sum() > 5000 and with_tower["steps"].max() > 20


# ---- 5. render scatter
def test_the_fast_triangle_list_is_the_loop_on_every_render_case():
    import render_cases as RC
    import render_ref as R
    for name, c in sorted(RC.CASES.items()):
        assert R.triangles(c.vertex_index, c.cells) == R.triangles(c.vertex_index, c.cells, loop=True), name
    assert sum(len(R.triangles(c.vertex_index, c.cells)) for c in RC.CASES.values()) > 5000
    c = L.render_case()
    assert len(R.triangles(c.vertex_index, c.cells)) == 8


def test_second_trip_triangles_win_lose_and_count():
    import render_ref as R
    c = L.render_case()
    (ref, cover), quads = L.render_reference(), {q.name: q for q in L.render_quads()}
    assert c.cells.size == L.RENDER_CELLS and (c.cells != 0).sum() == len(quads) == 5
    cell = {name: q.cj * (L.RENDER_GW - 1) + q.ci for name, q in quads.items()}
    T = L.THRESHOLD["render"]
    assert cell["far"] < T and cell["front"] < T and all(cell[n] >= T for n in ("near", "large", "bad"))
    assert all(cell[n] < L.RENDER_CELLS and quads[n].cj == L.RENDER_GH - 2 for n in ("near", "large", "bad"))
    assert ref["counts"].tolist() == [6, 1, 1]                                    # drawn, too large, unusable
    first = R.render(c.points, c.grey, c.vertex_index, np.where(np.arange(c.cells.size).reshape(c.cells.shape) < T, c.cells, 0).astype(np.uint8),
                     c.view, c.max_extent)
    assert first["counts"].tolist() == [4, 0, 0]                                  # every count hangs on the second trip
    near = (2 * cell["near"], 2 * cell["near"] + 1)
    covered = cover[near[0]] | cover[near[1]]
    won = {(x, y) for y, x in zip(*np.nonzero((ref["triangle"] == near[0]) | (ref["triangle"] == near[1])))}
    assert len(won) >= 3 and len(covered - won) >= 3 and won <= covered           # it wins some pixels and loses others
    lost_to = {int(ref["triangle"][y, x]) // 2 for x, y in covered - won}
    assert lost_to == {cell["front"]}
    far = {(x, y) for t in (2 * cell["far"], 2 * cell["far"] + 1) for x, y in cover[t]}
    assert won <= far                                                             # ... against a first-trip triangle behind it
    assert (first["triangle"] != ref["triangle"]).sum() == len(won) and (first["shade"] != ref["shade"]).sum() > 0


# ---- 6. subtract
def test_the_forced_pairs_of_the_subtraction_lie_in_the_second_trip():
    import terrain_ref as R
    a, b = L.subtract_pair()
    want = L.subtract_reference()
    n = a.size
    assert n - 4 >= L.THRESHOLD["subtract"]                                       # the last four cells of the last row
    for row, cols in ((0, slice(0, 4)), (-1, slice(-4, None))):
        assert want[row, cols].tolist() == [R.INVALID, R.INVALID, 0x7F800000, R.INVALID]   # inf - inf does not reach the map
    late = want.reshape(-1)[L.THRESHOLD["subtract"]:]
    assert len(late) == L.SUBTRACT_W - 1 and len(np.unique(late)) >= 6 and (late == R.INVALID).sum() > 100 and (late != R.INVALID).sum() > 100
    assert R.bits_of(a).tobytes() != R.bits_of(b).tobytes() and (want != R.INVALID).sum() > n // 5   # half the patterns are NaNs
