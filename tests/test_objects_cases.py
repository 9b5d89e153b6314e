"""The cases of tests/objects_cases.py test something, shown without a GPU: the numpy restatement of "surface objects"
(tests/objects_ref.py) equals the plain loop on every case, the records add up to the members, ids and records say the same,
a transposed map gives the transposed records, and the cases hold what they claim -- seams, a ring whose box holds foreign cells,
equal peaks, both zeros, clipped cells, ties of rintf."""
import numpy as np
import pytest

import objects_cases as C
import objects_ref as R

NAMES = [c.name for c in C.CASES]


def equal_records(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_equals_the_plain_loop(name):
    c = C.BY_NAME[name]
    want, loop = C.reference(c), R.objects_loop(c.d, c.min_height, c.max_diff, c.scale, c.min_cells)
    assert want["count"] == loop["count"] and np.array_equal(want["ids"], loop["ids"])
    for field in R.RECORD.names:
        assert np.array_equal(want["records"][field].view(np.uint32 if field in ("peak", "low") else want["records"][field].dtype),
                              loop["records"][field].view(np.uint32 if field in ("peak", "low") else loop["records"][field].dtype)), field
    assert equal_records(want["records"], loop["records"])


@pytest.mark.parametrize("name", NAMES)
def test_records_and_ids_are_consistent(name):
    c = C.BY_NAME[name]
    want = C.reference(c)
    ids, records = want["ids"], want["records"]
    member = R.members(c.d, c.min_height)
    h, w = c.d.shape
    assert not (ids[~member] != R.NONE).any()
    dropped = member & (ids == R.NONE)
    assert int(records["cells"].sum()) + int(dropped.sum()) == int(member.sum())
    assert (records["cells"] >= max(c.min_cells, 1)).all() and (np.diff(records["label"].astype(np.int64)) > 0).all()
    assert np.array_equal(np.bincount(ids[ids != R.NONE].astype(np.int64), minlength=len(records)), records["cells"])
    flat = ids.reshape(-1)
    assert np.array_equal(flat[records["label"]], np.arange(len(records), dtype=np.uint32))    # the label is a cell of its object
    assert np.array_equal(flat[records["peakIndex"]], np.arange(len(records), dtype=np.uint32))
    assert np.array_equal(R.S.bits(c.d).reshape(-1)[records["peakIndex"]], records["peak"].view(np.uint32))
    assert (records["label"] // w == records["minY"]).all() and (records["reserved"] == 0).all()
    assert (records["perimeter"] >= 4).all() and (records["perimeter"] <= 2 * records["cells"].astype(np.int64) + 2).all()
    assert (records["perimeter"] % 2 == 0).all() and (records["clipped"] <= records["cells"]).all()
    box = (records["maxX"].astype(np.int64) - records["minX"] + 1) * (records["maxY"].astype(np.int64) - records["minY"] + 1)
    assert (records["cells"] <= box).all() and (records["perimeter"] >= 2 * ((records["maxX"] - records["minX"] + 1) + (records["maxY"] - records["minY"] + 1))).all()
    if c.min_cells <= 1:                                                          # every member belongs to a kept object
        assert not dropped.any()


@pytest.mark.parametrize("name", NAMES)
def test_a_transposed_map_swaps_x_and_y_and_nothing_else(name):
    c = C.BY_NAME[name]
    a = C.reference(c)["records"]
    b = R.objects(np.ascontiguousarray(c.d.T), c.min_height, c.max_diff, c.scale, c.min_cells)["records"]
    swap = {"minX": "minY", "minY": "minX", "maxX": "maxY", "maxY": "maxX", "sumX": "sumY", "sumY": "sumX", "sumXX": "sumYY", "sumYY": "sumXX"}
    same = [f for f in R.RECORD.names if f not in ("label", "peakIndex")]     # raster indices are the transposed map's own

    def rows(records, rename):
        return sorted(tuple(int(r[rename.get(f, f)].view(np.uint32)) if f in ("peak", "low") else int(r[rename.get(f, f)]) for f in same) for r in records)
    assert rows(a, {}) == rows(b, swap)


def test_the_cases_hold_what_they_claim():
    # one object on each seam and on the corner
    c = C.BY_NAME["seams 130x35"]
    r = C.reference(c)["records"]
    assert r["cells"].tolist() == [11, 9, 16]
    assert (r["minX"][0], r["maxX"][0]) == (59, 69) and (r["minY"][1], r["maxY"][1]) == (12, 20)
    assert (r["minX"][2], r["maxX"][2], r["minY"][2], r["maxY"][2]) == (62, 65, 14, 17) and r["perimeter"].tolist() == [24, 20, 16]
    # the serpentine and the whole map: one object
    for name in ("serpentine 130x35", "whole 130x35", "whole 65x17", "whole 1x1"):
        c = C.BY_NAME[name]
        r = C.reference(c)["records"]
        assert len(r) == 1 and r["label"][0] == 0 and r["cells"][0] == int((c.d >= 1).sum())
    c = C.BY_NAME["whole 130x35"]
    assert C.reference(c)["records"]["perimeter"][0] == 2 * (130 + 35)
    tiles = {(y // C.TILE_H, x // C.TILE_W) for y, x in zip(*np.nonzero(C.BY_NAME["serpentine 130x35"].d >= 1))}
    assert len(tiles) == 3 * 3
    # the checkerboard: every object one cell, every perimeter 4, as many as the map holds
    c = C.BY_NAME["checkerboard 130x35"]
    r = C.reference(c)["records"]
    assert len(r) == (130 * 35 + 1) // 2 and (r["cells"] == 1).all() and (r["perimeter"] == 4).all() and (r["label"] == r["peakIndex"]).all()
    # the ring: its box holds the island, its perimeter counts the hole's outline
    r = C.reference(C.BY_NAME["ring 130x35"])["records"]
    assert r["cells"].tolist() == [99 - 35, 3] and r["perimeter"].tolist() == [2 * (11 + 9) + 2 * (7 + 5), 8]
    assert r["minX"][0] < r["minX"][1] and r["maxX"][1] < r["maxX"][0] and r["minY"][0] < r["minY"][1] < r["maxY"][0]
    # a finite maxDiff parts the two-level block and keeps the ramp whole
    joined, parted = (C.reference(C.BY_NAME[n])["records"] for n in ("two levels 130x35", "two levels maxDiff 0.5 130x35"))
    assert len(joined) == 2 and len(parted) == 3 and parted["cells"][:2].sum() == joined["cells"][0] and parted["cells"][2] == 130
    # minCells drops objects and the survivors are renumbered
    every, some = (C.reference(C.BY_NAME[n]) for n in ("blobs 130x35", "blobs minCells 4 130x35"))
    assert 0 < some["count"] < every["count"] and (every["records"]["cells"] < 4).any()
    assert np.array_equal(some["records"], every["records"][every["records"]["cells"] >= 4])
    assert C.reference(C.BY_NAME["blobs minCells 0 130x35"])["count"] == every["count"]
    # values
    c = C.BY_NAME["hard -inf 130x35"]
    r, bits = C.reference(c)["records"], R.S.bits(c.d)
    assert r["clipped"].sum() > 0 and (r["peak"].view(np.uint32) == 0x7F800000).any() and (r["low"].view(np.uint32) == 0xFF800000).any()
    member = R.members(c.d, c.min_height)
    assert not member[(bits == 0x7FC00001) | (bits == 0xFFC00000) | (bits == 0x7FFFFFFF) | (bits == R.INVALID)].any()
    assert member[bits == 0x7F800000].all() and member[bits == 0xFF800000].all()
    c = C.BY_NAME["hard +inf 130x35"]
    r = C.reference(c)["records"]
    assert len(r) > 0 and (r["cells"] == 1).all() and (r["clipped"] == 1).all() and (r["sumQQ"] == 0).all()    # two +inf cells do not link
    ok, q = R.quantise(np.array([256.0, 256.00003, -256.0, -256.00003, 0.001953125, 0.005859375, 0.009765625, -0.005859375], np.float32), 256.0)
    assert ok.tolist() == [True, False, True, False] + [True] * 4 and q.tolist() == [65536, 0, -65536, 0, 0, 2, 2, -2]   # ties to even
    c = C.BY_NAME["zeros 130x35"]
    r = C.reference(c)["records"]
    assert len(r) == 1 and r["peak"].view(np.uint32)[0] == 0 and r["low"].view(np.uint32)[0] == 0x80000000
    assert r["peakIndex"][0] == int(np.nonzero(R.S.bits(c.d).reshape(-1) == 0)[0][0])          # equal peaks: the smaller index
    assert C.reference(C.BY_NAME["nothing 130x35"])["count"] == 0
    # equal peaks inside larger objects
    c = C.BY_NAME["hard 0 maxDiff 1 130x35"]
    r = C.reference(c)["records"]
    holders = np.array([(R.S.bits(c.d)[C.reference(c)["ids"] == i] == p).sum() for i, p in enumerate(r["peak"].view(np.uint32))])
    assert (holders > 1).any()


def test_the_boxed_scene_gives_its_five_boxes_and_not_the_plateau():
    """from the scene's definition: the boxes of terrain_cases.BOXES stand out of the terrain, the plateau of side 2 r_max + 1 is
    ground to the filter and so is no object.  terrain_ref, fill_ref and objects_ref say so, and the cases file fixes it"""
    import terrain_cases as TC
    s = C.scene_objects()
    want, objects = s["want"], s["objects"]
    r = want["records"]
    assert want["count"] == 5 and tuple(r["cells"].tolist()) == C.SCENE_CELLS and tuple(r["perimeter"].tolist()) == C.SCENE_PERIMETERS
    boxes = sorted(TC.BOXES, key=lambda b: b[1] * objects.shape[1] + b[0])             # raster order of their first cells
    assert [b[2] ** 2 for b in boxes] == list(C.SCENE_CELLS)
    for rec, (x0, y0, side, up) in zip(r, boxes):
        assert (rec["minX"], rec["minY"], rec["maxX"], rec["maxY"]) == (x0, y0, x0 + side - 1, y0 + side - 1)
        assert rec["label"] == y0 * objects.shape[1] + x0 and abs(float(rec["peak"]) - up) < 0.3 and abs(float(rec["low"]) - up) < 0.3
        m = R.measures(rec, R.Frame(cell=1.0), 256.0)
        assert m["area"] == side * side and abs(m["meanHeight"] - up) < 0.3 and abs(m["volume"] - up * side * side) < 0.3 * side * side
        assert m["centroidX"] == x0 + (side - 1) / 2 and m["centroidY"] == y0 + (side - 1) / 2
        # a square: equal moments up to the rounding of sum / n - c c, numbers below 2^13 in double: relative 2^13 2^-52 / (1 / 12)
        assert side == 1 or abs(m["elongation"] - 1) < 1e-10
    px, py, pside, _ = TC.PLATEAU
    assert (want["ids"][py:py + pside, px:px + pside] == R.NONE).all()               # the plateau is not among them
    assert (want["ids"] != R.NONE).sum() == sum(C.SCENE_CELLS) == TC.scene()["box"].sum()


def test_the_large_map_lies_past_every_cap():
    k, (w, h) = C.caps(), C.large_size()
    assert k == dict(mask=4096, reduce=1024, finish=1024)
    tiles = ((w + C.TILE_W - 1) // C.TILE_W) * ((h + C.TILE_H - 1) // C.TILE_H)
    assert w * h > k["mask"] * 256 and tiles > k["reduce"] and (h // 2) * w // 2 > k["finish"] * 256
    assert w % C.TILE_W != 0 and w * h < 1300000
