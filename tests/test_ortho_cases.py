"""The ortho-image cases on the numpy reference alone (no GPU): every case of tests/ortho_cases.py exercises what it claims, and the
reference itself behaves as include/ssrlcv_hip.h "ortho-image" says on inputs small enough to work out by hand."""
import numpy as np

import dsm_cases as DC
import dsm_ref as D
import ortho_cases as C
import ortho_ref as R

f32 = np.float32


def _differs(a, b):
    return int((C.reference(a)["ortho"] != C.reference(b)["ortho"]).sum()), int((C.reference(a)["seen"] != C.reference(b)["seen"]).sum())


def test_every_occlusion_case_has_occluded_and_visible_cells():
    for name, c in C.CASES.items():
        if not c.occlusion:
            continue
        r = C.reference(name)
        occluded, visible = (r["inside"] & ~r["sees"]).sum((1, 2)), r["sees"].sum((1, 2))
        assert ((occluded >= 20) & (visible >= 20)).any(), (name, occluded, visible)


def test_the_parameters_change_the_result():
    assert _differs("67x41/steps7", "67x41/steps256")[1] >= 20
    assert _differs("67x41/steps0", "67x41/steps1")[1] > 0 and _differs("67x41/steps1", "67x41/steps7")[1] >= 20
    assert not (C.reference("67x41/steps0")["inside"] & ~C.reference("67x41/steps0")["sees"]).any()      # maxSteps 0: no occlusion test
    assert _differs("67x41/grazing/bias0.0", "67x41/grazing/bias0.05")[1] >= 20                                                # bias 0 against 0.05
    assert not (C.reference("67x41/biasinf")["inside"] & ~C.reference("67x41/biasinf")["sees"]).any()    # nothing stands above +inf
    for m in ("m3", "m8", ):
        assert _differs("67x41/%s/rule0" % m, "67x41/%s/rule1" % m)[0] >= 20                               # FIRST against MEDIAN
    for name in ("67x41/m3/rule0", "67x41/m8/rule1", "257x131/m3/rule0"):
        which = C.reference(name)["which"]
        assert ((which != 0) & (which != 0xFF)).sum() >= 20, name


def test_the_cameras_are_what_they_are_called():
    r = {name.split("/")[1]: C.reference(name) for name in C.CASES if name.startswith("67x41/") and name.count("/") == 1}
    valid = D.bits(C.CASES["67x41/nadir"].height) != D.INVALID_BITS
    assert r["nadir"]["inside"][0][valid].all() and (r["nadir"]["steps"].max() < r["oblique30"]["steps"].max())
    assert not r["away"]["inside"].any()                                                 # W <= 0 everywhere
    assert r["below"]["inside"][0][valid].all() and not r["below"]["sees"].any()         # it projects, and !(dz > 0)
    part = r["partial"]["inside"][0][valid]
    assert part.sum() >= 100 and (~part).sum() >= 100                                    # the image covers part of the grid
    low, c = r["low"], C.CASES["67x41/low"]
    eye = c.views[0].eye
    jj, ii = np.mgrid[0:c.frame.h, 0:c.frame.w]
    L = np.maximum(np.abs(eye[0] - (ii + f32(0.5))), np.abs(eye[1] - (jj + f32(0.5))))
    assert ((L < 1) & low["sees"][0]).sum() >= 1 and (low["steps"][0][(L < 1)] == 0).all()   # beneath the camera: no march
    ended_by_the_camera = low["sees"][0] & (low["steps"][0] > 0) & (low["steps"][0] > L) & (low["steps"][0] < 256)
    assert ended_by_the_camera.sum() >= 20                                               # fs > L ended these marches inside the grid
    eye = C.CASES["67x41/diagonal"].views[0].eye
    assert (np.abs(eye[0] - (ii + f32(0.5))) == np.abs(eye[1] - (jj + f32(0.5)))).sum() >= 20   # |du| == |dv| exactly


def test_the_shapes_cross_tiles_and_the_salt_is_there():
    sizes = {(c.frame.w, c.frame.h) for c in C.CASES.values()}
    assert sizes == {(1, 1), (67, 41), (257, 131)}
    assert {len(c.views) for c in C.CASES.values()} >= {1, 3, 8} and {c.max_steps for c in C.CASES.values()} >= {0, 1, 7, 256}
    assert {v.image.shape for c in C.CASES.values() for v in c.views} == {(96, 96), (50, 70)}
    eight = C.CASES["67x41/m8/rule1"].views
    assert any(a is b for i, a in enumerate(eight) for b in eight[i + 1:])               # one view twice
    b = D.bits(C.CASES["67x41/salted/m3"].height)
    for special in C.SPECIALS:
        assert (b == special).sum() >= 1
    r = C.reference("67x41/salted/m3")
    odd = (b == D.INVALID_BITS) | ~np.isfinite(C.CASES["67x41/salted/m3"].height)
    assert (r["which"][odd] == 0xFF).all() and (r["seen"][odd] == 0).all() and (r["ortho"][odd] == 0).all()
    assert (r["seen"][~odd] != 0).sum() > 1000


def test_a_wall_hides_what_lies_behind_it_and_nothing_else():
    """a 1 x 9 strip, a wall of height 4 at i = 4, the camera far along +i at 45 degrees: the cells the wall's shadow covers"""
    fr = DC.axis_frame(9, 1, cell=1.0)
    z = np.zeros((1, 9), np.float32)
    z[0, 4] = 4.0
    eye = np.array([104.5, 0.5, 100.0], np.float32)   # from cell i the ray rises 100 / (104 - i) a cell
    v = R.view(np.zeros((4, 4), np.uint8), np.eye(3).reshape(9), (0, 0, 0), eye)
    ii = np.arange(9)
    vis, steps = R.march(z, ii, np.zeros(9, int), z[0], eye, 256, 0.0)
    # the ray from cell i reaches the wall after 4 - i steps at height (4 - i) 100 / (104 - i) < 4 - i: below 4 for i = 0 .. 3
    assert list(vis) == [False, False, False, False, True, True, True, True, True]
    vis7, _ = R.march(z, ii, np.zeros(9, int), z[0], eye, 2, 0.0)
    assert list(vis7) == [True, True, False, False, True, True, True, True, True]       # two steps do not reach the wall from i < 2
    assert R.march(z, ii, np.zeros(9, int), z[0], eye, 256, 4.0)[0].all()               # a bias of the wall's height
    assert v.eye.dtype == np.float32
