"""The cases of include/ssrlcv_hip.h "mesh render": the smallest meshes and views at which csrc/render.hip can go wrong.
tests/test_render_cases.py proves on the reference alone (tests/render_ref.py) that each case reaches what it is named for;
tests/test_gpu_render.py holds the GPU to the reference on all of them.

Most cases are STRIPS: a grid two nodes wide whose even cell rows hold one quad each and whose odd cell rows are empty (byte 0),
so every quad has four vertices of its own and the cases place them freely.  Their camera sits at the world's origin and looks
along +z with M the identity: a point (x, y, 1) lies at pixel (x, y) exactly, W is z."""
from collections import namedtuple

import numpy as np

import dsm_cases as DC
import dsm_ref as D
import mesh_ref as M
import ortho_cases as OC
import render_ref as R

f32 = np.float32
NAN, INF = float("nan"), float("inf")
IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1)

Case = namedtuple("Case", "points grey vertex_index cells view max_extent")


def eye_view(w, h):
    return R.view(IDENTITY, (0, 0, 0), w, h)


def quad(byte, a, b, c, d, grey=(10, 90, 170, 250)):
    """one cell: its byte, the corners a, b, c, d as (x, y) or (x, y, z) with z = 1, and their greys"""
    pts = [tuple(p) + (1.0,) * (3 - len(p)) for p in (a, b, c, d)]
    return byte, pts, grey


def strip(quads, view, max_extent=8, n=None):
    """-> Case of a 2 x (2 len(quads)) node grid: quad k is cell row 2 k.  n: fewer points than the map names (a stale map)"""
    k = len(quads)
    vertex_index = np.arange(4 * k, dtype=np.uint32).reshape(2 * k, 2)
    cells = np.zeros((2 * k - 1, 1), np.uint8)
    points, grey = np.zeros((4 * k, 3), f32), np.zeros(4 * k, np.uint8)
    for q, (byte, pts, g) in enumerate(quads):
        cells[2 * q, 0] = byte
        points[4 * q:4 * q + 4] = pts          # a, b in node row 2 q; c, d in node row 2 q + 1
        grey[4 * q:4 * q + 4] = g
    if n is not None:
        points, grey = points[:n], grey[:n]
    return Case(points, grey, vertex_index, cells, view, max_extent)


def square(x, y, s, z=1.0):
    """the corners a, b, c, d of an axis-parallel square of side s at (x, y), depth z: a point (X, Y, z) lies at pixel (X / z, Y / z)"""
    return [(x * z, y * z, z), ((x + s) * z, y * z, z), (x * z, (y + s) * z, z), ((x + s) * z, (y + s) * z, z)]


def relief_case(view_size=(96, 64), grid=(64, 48), select=False):
    """a relief with a tower and a wall under an oblique camera: the near ridge hides far ground.  Joined everywhere (max_jump inf),
    so the tower's flanks are triangles several pixels long."""
    w, h = grid
    height = OC.relief(w, h, 7)
    fr = DC.axis_frame(w, h, cell=OC.CELL)
    vertex_index, cells, n = M.mesh(height, 1, INF)
    points = D.points(height, fr)
    assert len(points) == n
    centre = np.array([w * OC.CELL / 2, h * OC.CELL / 2, 0.0])
    pos = centre + (0.0, -40.0, 40.0)
    reach = max(w, h) * OC.CELL / 2
    cam = OC.camera(pos, centre - pos, view_size, 2.0 * np.arctan(1.1 * reach / 56.0))
    Mx, p, _ = OC.R.view_of_camera(cam, fr)
    grey = np.random.RandomState(3).randint(0, 256, n).astype(np.uint8)
    if select:      # every third vertex goes: the mesh follows through "disparity mesh" item 6
        kept = np.array([k for k in range(n) if k % 3 != 1], np.uint32)
        vertex_index, cells = M.select(vertex_index, cells, n, kept)
        points, grey = points[kept], grey[kept]
    return Case(points, grey, vertex_index, cells, R.view(Mx, p, *view_size), 32)


def _cases():
    c = {}
    v8 = eye_view(8, 8)
    # pixel centres exactly on the edges and corners of one triangle: T0 = (a, c, d) of a square from (1, 1) to (5, 5)
    c["one_triangle/on_centres"] = strip([quad(1, *square(1, 1, 4))], v8)
    c["one_triangle/other_diagonal"] = strip([quad(5, *square(1, 1, 4))], v8)
    # two triangles whose shared edge runs through pixel centres, at one depth (the smaller id wins) and tilted (the nearer wins)
    c["shared_edge/ad"] = strip([quad(3, *square(1, 1, 5))], v8)
    c["shared_edge/bc"] = strip([quad(7, *square(1, 1, 5))], v8)
    c["shared_edge/tilted"] = strip([quad(3, (1, 1, 1), (6 * 1.25, 1 * 1.25, 1.25), (1 * 0.75, 6 * 0.75, 0.75), (6, 6, 1))], v8)
    # coincident triangles through duplicate points: the smaller id wins whatever its greys
    c["coincident"] = strip([quad(3, *square(1, 1, 5), grey=(200, 210, 220, 230)), quad(3, *square(1, 1, 5), grey=(1, 2, 3, 4)),
                             quad(7, *square(1, 1, 5), grey=(90, 91, 92, 93))], v8)
    # a nearer quad in front of a farther one: the depth test, not the order
    c["near_hides_far"] = strip([quad(3, *square(0, 0, 7, z=2.0)), quad(3, *square(2, 2, 3, z=1.5), grey=(5, 5, 5, 5)), quad(3, *square(3, 1, 4, z=4.0))], v8)
    # corners that are not usable: each spoils the triangles that hold it and leaves the other triangle of its cell alone
    sq = square(1, 1, 5)
    for name, bad in (("w_zero", (1, 1, 0.0)), ("w_negative", (-1, -1, -1.0)), ("w_above_2p60", (0, 0, 2.0 ** 61)), ("w_tiny", (0, 0, 1e-39)),
                      ("nan", (NAN, 1, 1)), ("inf", (1, INF, 1)), ("minus_inf_z", (1, 1, -INF)), ("sx_above_2p20", (2.0 ** 20 + 1, 1, 1)),
                      ("sy_below_minus_2p20", (1, -(2.0 ** 20) - 1, 1))):
        c["unusable/" + name] = strip([quad(7, sq[0], bad, sq[2], sq[3]), quad(3, sq[0], sq[1], sq[2], bad)], v8)
    # the last usable values: W = 2^60 at the image's origin, |sx| = 2^20 (too large a box, not unusable)
    c["usable/w_2p60"] = strip([quad(7, (0, 0, 2.0 ** 60), sq[1], sq[2], sq[3])], v8)
    c["usable/sx_2p20"] = strip([quad(3, sq[0], (2.0 ** 20, 1, 1), sq[2], sq[3]), quad(3, sq[0], sq[1], (1, -(2.0 ** 20), 1), sq[3])], v8, 64)
    # a bounding box exactly at maxExtent and one unit of 1/256 pixel above it, in x and in y
    for e in (1, 8, 64):
        s, u = float(e), 1.0 / 256
        view = eye_view(e + 6, 5) if e < 64 else eye_view(70, 66)
        c["extent/%d" % e] = strip([quad(1, (1, 1), (9, 9), (1, 1 + min(s, 3.0)), (1 + s, 1 + min(s, 3.0))),
                                    quad(1, (1, 1), (9, 9), (1, 1 + min(s, 3.0)), (1 + s + u, 1 + min(s, 3.0))),
                                    quad(1, (3, 1), (9, 9), (3, 1 + s), (4, 1 + s)),
                                    quad(1, (3, 1), (9, 9), (3, 1 + s + u), (4, 1 + s + u))], view, e)
    # zero area (three points in a line, two equal points), and A < 0: the mirror image of a quad is drawn all the same
    c["zero_area"] = strip([quad(3, (1, 1), (3, 3), (2, 2), (5, 5)), quad(1, (2, 2), (0, 0), (2, 2), (6, 3)), quad(2, (1, 5), (6, 5), (0, 0), (3, 5))], v8)
    c["negative_area"] = strip([quad(3, (6, 1), (1, 1), (6, 6), (1, 6)), quad(7, (6, 1, 2), (1, 1, 2), (6, 6, 2), (1, 6, 2))], v8)
    # triangles half off and wholly off each side of the image, negative fixed-point coordinates among them
    off = []
    for dx, dy in ((-3, 2), (6, 2), (2, -3), (2, 6), (-3, -3), (6, 6)):
        off.append(quad(3, *square(dx, dy, 4.5)))                                  # half off
    for dx, dy in ((-5.5, 2), (8.25, 2), (2, -5.5), (2, 8.25), (-0.9, 3), (3, -0.9), (7.1, 7.1)):
        off.append(quad(7, *square(dx, dy, 0.8 if -1 < dx < 8 and -1 < dy < 8 else 4.5)))   # wholly off; the last three hold no centre of the image
    c["off_image"] = strip(off, v8)
    c["between_centres"] = strip([quad(3, *square(2.1, 2.1, 0.8)), quad(3, *square(2.1, 2.1, 0.9))], v8)   # on the image, no centre / one centre
    # the smallest view and an odd, flat one
    c["view_1x1"] = strip([quad(3, *square(-2, -2, 4)), quad(1, *square(-1, -1, 3, z=0.5))], eye_view(1, 1))
    c["view_65x3"] = strip([quad(7, *square(x, -1, 4.5, z=1 + x / 64.0)) for x in range(-2, 66, 3)], eye_view(65, 3))
    # every value a cell byte takes
    c["cell_bytes"] = strip([quad(b, *square(0.5 + 0.25 * k, 0.5 + 0.5 * k, 3.5, z=1 + 0.125 * k)) for k, b in enumerate((0, 1, 2, 3, 5, 6, 7))], v8)
    # a vertexIndex that is stale for n: the second quad's last two vertices lie behind the points
    c["stale_index"] = strip([quad(3, *square(1, 1, 3)), quad(3, *square(3, 3, 4))], v8, n=6)
    none = strip([quad(3, *square(1, 1, 3)), quad(7, *square(3, 3, 4))], v8)
    vi = none.vertex_index.copy()
    vi[0, 1] = vi[3, 0] = R.NONE
    c["no_vertex"] = none._replace(vertex_index=vi)
    c["no_points"] = strip([quad(3, *square(1, 1, 3))], v8, n=0)
    # grids without a cell
    one = Case(np.array([[2, 2, 1]], f32), np.array([7], np.uint8), np.zeros((1, 1), np.uint32), np.zeros((0, 0), np.uint8), v8, 8)
    c["grid_1x1"] = one
    c["grid_5x1"] = one._replace(points=np.tile(one.points, (5, 1)), grey=np.arange(5, dtype=np.uint8), vertex_index=np.arange(5, dtype=np.uint32).reshape(1, 5),
                                 cells=np.zeros((0, 4), np.uint8))
    c["grid_1x5"] = c["grid_5x1"]._replace(vertex_index=np.arange(5, dtype=np.uint32).reshape(5, 1), cells=np.zeros((4, 0), np.uint8))
    c["grid_0x0"] = one._replace(points=np.zeros((0, 3), f32), grey=np.zeros(0, np.uint8), vertex_index=np.zeros((0, 0), np.uint32))
    # the fold under an oblique camera, and the same mesh after mesh_select
    c["fold"] = relief_case()
    c["fold/selected"] = relief_case(select=True)
    c["fold/small_extent"] = c["fold"]._replace(max_extent=2)
    return c


CASES = _cases()
_REF = {}


def reference(name):
    """the reference's outputs of a case, computed once and shared: nobody writes into them"""
    if name not in _REF:
        c = CASES[name]
        _REF[name] = R.render(c.points, c.grey, c.vertex_index, c.cells, c.view, c.max_extent)
        for a in _REF[name].values():
            a.setflags(write=False)
    return _REF[name]


# ---- the rig's scene: the true heights at the cell centres, textured by the model's ortho-image, drawn into a source camera
TEXTURE_VIEWS, CHECK_VIEW = (0, 1, 2), 1     # the ortho-image of all three views, the first that sees a cell; the check in an oblique one
ORTHO_STEPS, ORTHO_BIAS = 64, 0.0
_SCENE, _CHECK = {}, {}


def scene_views():
    """the scene's views as ssrlcv_dsm_ortho_view_host makes them, restated (ortho_cases.view_of)"""
    s, fr = DC.scene(), DC.scene_frame()
    return [OC.view_of(cam, fr, img) for cam, img in zip(s["cams"], s["images"])]


def scene_model():
    """-> dict(height, frame, points, vertex_index, cells, ortho, grey): the scene's own heights, meshed and textured"""
    if not _SCENE:
        import torch
        s, fr = DC.scene(), DC.scene_frame()
        half = DC.SCENE_SIZE * s["rig"].gsd / 2.0
        jj, ii = np.mgrid[0:fr.h, 0:fr.w]
        a, b = (ii + 0.5) * float(fr.cell) - half, (jj + 0.5) * float(fr.cell) - half
        height = s["scene"].height(torch.from_numpy(a).float(), torch.from_numpy(b).float()).numpy().astype(f32)
        vertex_index, cells, n = M.mesh(height, 1, INF)
        ortho = OC.R.ortho(height, fr, [scene_views()[k] for k in TEXTURE_VIEWS], ORTHO_STEPS, ORTHO_BIAS, OC.R.FIRST)["ortho"]
        _SCENE.update(height=height, frame=fr, points=D.points(height, fr), vertex_index=vertex_index, cells=cells, ortho=ortho,
                      grey=ortho[D.bits(height) != D.INVALID_BITS])
    return _SCENE


def displaced(points, fr, cells_xy=(0, 0), cells_up=0.0):
    """the model's vertices moved by whole cells along ex, ey and ez, in float32: the texture goes with them"""
    move = (f32(cells_xy[0]) * fr.cell) * fr.ex + (f32(cells_xy[1]) * fr.cell) * fr.ey + (f32(cells_up) * fr.cell) * fr.ez
    return (np.asarray(points, f32) + move.astype(f32)).astype(f32)


def scene_check(cells_xy=(0, 0), cells_up=0.0):
    """the photo check of the scene's model, displaced, on the reference alone -> dict(points, render, residual, stats)"""
    key = (tuple(cells_xy), float(cells_up))
    if key not in _CHECK:
        m = scene_model()
        v = scene_views()[CHECK_VIEW]
        h, w = v.image.shape
        points = displaced(m["points"], m["frame"], cells_xy, cells_up)
        out = R.render(points, m["grey"], m["vertex_index"], m["cells"], R.view(v.M, v.pos, w, h), 8)
        res = R.residual(v.image, out["shade"], out["depth"])
        _CHECK[key] = dict(points=points, render=out, residual=res, stats=R.stats(res))
    return _CHECK[key]
