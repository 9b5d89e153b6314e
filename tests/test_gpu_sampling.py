"""GPU parity of the hot sampling kernels (k_polar, k_thetas, the merged expansion, k_desc_consts, k_descriptors of
csrc/keypoints.hip) OFF the default parameters and off the key points a detector finds (cases: tests/sampling_cases.py, proven on
the oracle alone by tests/test_sampling_cases.py).  Every comparison is bit for bit: the count, the order, loc / sigma / theta as
bit patterns, all 128 descriptor bytes.

Part 1 runs the plan's parameters through extract, describe, the stage calls, every developer schedule and the plain exports.
Part 2 writes hand-placed key-point lists into a plan's workspace between two stage calls (the pointers of
ssrlcv_sift_plan_keypoints; preconditions in sampling_cases.py) and holds stages 6 and 7, and the export chain on the same lists,
to the per-key-point oracle."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import sampling_cases as C

pytestmark = pytest.mark.gpu

u32, f32c, ci = ctypes.c_uint32, ctypes.c_float, ctypes.c_int
UNSUPPORTED = -4     # SSRLCV_ERR_UNSUPPORTED (include/ssrlcv_hip.h)


@pytest.fixture(scope="module")
def capi():
    from ssrlcv_amd import capi
    return capi


# ---- reporting: where a mismatch is -------------------------------------------------------------------------------------------
def _first_difference(got, want, fields):
    """-> (index, field, got value, want value) of the first record that differs in a field (floats as bit patterns), or None"""
    for i in range(min(len(got), len(want))):
        for f in fields:
            a, b = np.atleast_1d(got[f][i]), np.atleast_1d(want[f][i])
            same = np.array_equal(H.bits(a), H.bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)
            if not same:
                return i, f, got[f][i], want[f][i]
    return None


def _assert_same(got, want, fields, what, describe=None):
    d = _first_difference(got, want, fields)
    if len(got) != len(want) or d is not None:
        where = "" if d is None else "first difference at %d, field %s: got %r, want %r%s" % (
            d[0], d[1], d[2], d[3], "" if describe is None else "; " + describe(d[0]))
        raise AssertionError("%s: %d records, the oracle has %d; %s" % (what, len(got), len(want), where))


KP_FIELDS = ("octave", "blur", "loc", "intensity", "sigma", "theta")
FEATURE_FIELDS = ("parent", "loc", "sigma", "theta", "values")


def _assert_features(got, want, what, describe=None):
    _assert_same(got, want, FEATURE_FIELDS, what, describe)
    H.assert_features_equal(got, want)


def _placed_describer(expanded, ow, dw):
    """feature index of a hand-placed set -> octave, blur, index in the octave's expanded list, both window half-widths"""
    rows = [(o, i, kp) for o, exp in enumerate(expanded) for i, kp in enumerate(exp)]

    def describe(k):
        o, i, kp = rows[k]
        pw = C.geometry(o).pw
        return "octave %d, blur %d, key point %d at (%r, %r) sigma %r theta %r, orientation half-width %d, descriptor half-width %d" % (
            o, kp["blur"], i, kp["loc"][0], kp["loc"][1], kp["sigma"], kp["theta"], int(C.ori_half(kp["sigma"], ow, pw)),
            int(C.desc_half(kp["sigma"], dw, pw)))
    return describe


# ---- part 1: the plan's parameters through the hot path ----------------------------------------------------------------------------
def _plan_for(capi, image_name, c, **kw):
    w, h, _ = C.IMAGES[image_name]
    return capi.SiftPlan(w, h, c.maxo, c.thr, c.ow, c.dw, **kw)


def _extract(capi, image_name, c):
    plan = _plan_for(capi, image_name, c)
    plan.extract(capi.to_dev(C.image(image_name)))
    return plan.features_host(H.FEATURE)


@pytest.mark.parametrize("name", list(C.PLAN_CASES))
def test_plan_parameters_through_extract(capi, name):
    c = C.PLAN_CASES[name]
    want = C.oracle_features("256x192", c.maxo, c.thr, c.ow, c.dw)
    assert len(want) == c.features
    _assert_features(_extract(capi, "256x192", c), want, "%s (%s)" % (name, c.why))


@pytest.mark.parametrize("name", C.WIDE_IMAGE_CASES)
def test_plan_parameters_on_the_wide_image(capi, name):
    """other per-octave counts, more key points at the left edge"""
    c = C.PLAN_CASES[name]
    want = C.oracle_features("384x256", c.maxo, c.thr, c.ow, c.dw)
    assert len(want) > 200
    _assert_features(_extract(capi, "384x256", c), want, "%s on 384 x 256" % name)


@pytest.mark.parametrize("name", C.ENTRY_POINT_CASES)
def test_plan_parameters_through_every_entry_point(capi, name):
    """build_dog + describe, and stages 0..7 one call each, land on extract's features and on the oracle's; checkKeyPoints (stage 5)
    takes the descriptor width, so from stage 5 on the lists are the oracle's chain at that width"""
    c = C.PLAN_CASES[name]
    img_d = capi.to_dev(C.image("256x192"))
    want = C.oracle_features("256x192", c.maxo, c.thr, c.ow, c.dw)
    fused = _extract(capi, "256x192", c)
    _assert_features(fused, want, name + ", extract")
    two = _plan_for(capi, "256x192", c)
    two.build_dog(img_d)
    two.describe()
    _assert_features(two.features_host(H.FEATURE), want, name + ", build_dog + describe")
    staged = _plan_for(capi, "256x192", c)
    staged.build_dog(img_d)
    for stage in range(8):
        staged.stage(stage)
        if stage == 5:
            for o, (lst, idx) in enumerate(C.checked_lists("256x192", c.dw)):
                g, gidx, overflow = staged.keypoints(o, H.SSKEYPOINT)
                assert overflow == 0
                _assert_same(g, lst, KP_FIELDS[:5], "%s, octave %d after stage 5" % (name, o))
                assert len(lst) == 0 or np.array_equal(gidx[:5], idx), (o, gidx, idx)
    _assert_features(staged.features_host(H.FEATURE), want, name + ", stages 0..7")


def test_a_plan_re_arms_over_empty_octaves_at_the_widest_descriptor(capi, oracle_lib):
    """dw = 30 leaves octaves 2-3 without key points; a constant image leaves every octave without; then the first image again,
    all on ONE plan: the empty-octave path of the merged expansion and its control words at a non-default width"""
    c = C.PLAN_CASES["dw30"]
    want = C.oracle_features("256x192", c.maxo, c.thr, c.ow, c.dw)
    lists = C.checked_lists("256x192", c.dw)
    assert len(lists[2][0]) == 0 and len(lists[3][0]) == 0 and len(want) == c.features
    flat = np.full((192, 256), 128, np.uint8)
    want_flat = H.oracle_sift(oracle_lib, flat, c.maxo, c.thr, c.ow, c.dw)
    plan = _plan_for(capi, "256x192", c)
    for k, (img, ref) in enumerate(((C.image("256x192"), want), (flat, want_flat), (C.image("256x192"), want))):
        plan.extract(capi.to_dev(img))
        _assert_features(plan.features_host(H.FEATURE), ref, "run %d on one plan" % k)


_SCHEDULE_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import helpers as H
import sampling_cases as C
from ssrlcv_amd import capi
img = C.image("256x192")
for name in C.SCHEDULE_CASES:
    c = C.PLAN_CASES[name]
    plan = capi.SiftPlan(256, 192, c.maxo, c.thr, c.ow, c.dw)
    plan.extract(capi.to_dev(img))
    g = plan.features_host(H.FEATURE)
    o = C.oracle_features("256x192", c.maxo, c.thr, c.ow, c.dw)
    assert len(g) == len(o) == c.features, (name, len(g), len(o))
    H.assert_features_equal(g, o)
    print(name, len(g), "OK")
print("SAMPLING OK")
"""


@pytest.mark.parametrize("variant", [
    {"SSRLCV_THETAS_LANES": "1"}, {"SSRLCV_THETAS_LANES": "2"}, {"SSRLCV_THETAS_LANES": "4"},   # chunks of 8, 16, 32 samples: the walked chain starts below
    {"SSRLCV_SAMPLING_PIPELINED": "1"},
    {"SSRLCV_SAMPLING_PIPELINED": "1", "SSRLCV_SAMPLING_IRREGULAR": "1"},
], ids=lambda v: "+".join(k.replace("SSRLCV_", "") + "=" + x for k, x in v.items()))
def test_every_sampling_schedule_off_the_defaults(variant):
    """the narrowest and the widest orientation and descriptor windows under every lane count of k_thetas and the pipelined
    sampling groups (developer build, one child process per switch set)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _SCHEDULE_SCRIPT % {"root": root}], env=H.dev_env(**variant), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "SAMPLING OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_plan_create_refuses_what_the_kernels_cannot_honour(capi):
    """host-only: no launch"""
    def create(maxo, ow, dw):
        p = capi.SiftParams(maxo, 0.8, ow, dw, 0)
        handle = ctypes.c_void_p()
        rc = capi.LIB.ssrlcv_sift_plan_create(u32(256), u32(192), ctypes.byref(p), ctypes.byref(handle))
        if rc == 0:
            capi.LIB.ssrlcv_sift_plan_destroy(handle)
        else:
            assert not handle.value
        return rc
    assert create(2, 1.5, 6.0) == 0
    for maxo in (0, 5):
        assert create(maxo, 1.5, 6.0) == UNSUPPORTED, maxo
    for bad in (0.0, -0.0, -1.0, float("nan")):
        assert create(2, 1.5, bad) == UNSUPPORTED, ("dw", bad)
        assert create(2, bad, 6.0) == UNSUPPORTED, ("ow", bad)
    assert create(2, 1.5, float(np.nextafter(np.float32(30.0), np.float32(np.inf)))) == UNSUPPORTED
    assert create(2, float(np.nextafter(np.float32(5.0), np.float32(np.inf))), 6.0) == UNSUPPORTED
    assert create(2, 5.0, 30.0) == 0 and create(4, 0.1, 0.2) == 0      # the bounds themselves are admitted


# ---- the export chain (plain k_x_* kernels over caller-owned buffers), at any widths -----------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _compact(capi, fn, t, n):
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.LIB.ssrlcv_hip_compact_workspace_bytes.restype = ctypes.c_size_t
    ws = capi.dev_bytes(int(capi.LIB.ssrlcv_hip_compact_workspace_bytes(u32(max(n, 1)))))
    capi.check(fn(capi.ptr(t), u32(n), capi.ptr(cnt), capi.ptr(ws), ctypes.c_size_t(ws.numel()), capi.stream_ptr()))
    return int(cnt.item())


def _segments(idx, n):
    return [(b, int(idx[b]), int((idx[b + 1] if b < 4 else n) - idx[b])) for b in range(5)]


def _export_chain(capi, levels, geoms, lists, maxo, thr, ow, dw, oriented=False):
    """pixel_gradients, compute_thetas, the two compactions, expand_keypoints, fill_descriptors over every octave and blur segment in
    list order, with the case's lambdas -> ([expanded SSKEYPOINT[] per octave], FEATURE[])"""
    L = capi.LIB
    expanded, feats = [], []
    for o, (lst, idx) in enumerate(lists):
        w, h, pw = geoms[o]
        out_o = []
        kp_d = _dev(lst) if len(lst) else None
        for b, start, cnt in _segments(idx, len(lst)):
            if cnt <= 0:
                continue
            grad = capi.dev_bytes(8 * w * h)
            capi.check(L.ssrlcv_hip_pixel_gradients(u32(w), u32(h), capi.ptr(_dev(levels[o][b])), capi.ptr(grad), capi.stream_ptr()))
            if oriented:
                src, first, nn = kp_d, start, cnt
                out_o.append(lst[start:start + cnt])
            else:
                thetas = torch.zeros(cnt * maxo, dtype=torch.float32, device="cuda")
                nums = torch.zeros(cnt * maxo, dtype=torch.int32, device="cuda")
                capi.check(L.ssrlcv_hip_compute_thetas(u32(cnt), u32(start), u32(w), u32(h), f32c(pw), f32c(ow), capi.ptr(kp_d), capi.ptr(grad),
                                                       capi.ptr(nums), u32(maxo), f32c(thr), capi.ptr(thetas), capi.stream_ptr()))
                nt = _compact(capi, L.ssrlcv_hip_compact_thetas, thetas, cnt * maxo)
                nn = _compact(capi, L.ssrlcv_hip_compact_addresses, nums, cnt * maxo)
                assert nt == nn
                if nn == 0:
                    continue
                src, first = capi.dev_bytes(32 * nn), 0
                capi.check(L.ssrlcv_hip_expand_keypoints(u32(nn), capi.ptr(kp_d), capi.ptr(src), capi.ptr(nums), capi.ptr(thetas), capi.stream_ptr()))
                out_o.append(capi.to_host(src, H.SSKEYPOINT, nn))
            ft = torch.zeros(152 * nn, dtype=torch.uint8, device="cuda")
            capi.check(L.ssrlcv_hip_fill_descriptors(u32(nn), u32(first), u32(w), u32(h), capi.ptr(ft), f32c(pw), f32c(dw), capi.ptr(src), capi.ptr(grad),
                                                     capi.stream_ptr()))
            f = capi.to_host(ft, H.FEATURE, nn)
            f["parent"] = -1      # (Feature() default; the export kernel, like the reference's, never writes it)
            feats.append(f)
        expanded.append(np.concatenate(out_o) if out_o else np.zeros(0, H.SSKEYPOINT))
    return expanded, (np.concatenate(feats) if feats else np.zeros(0, H.FEATURE))


@pytest.mark.parametrize("name", list(C.EXPORT_CASES))
def test_export_chain_off_the_defaults(capi, name):
    """check_keypoints at the case's descriptor width on the oracle's stage-4 list == the numpy predicate; then the orientation and
    descriptor exports with the case's lambdas == OracleSift.features: the plain kernels and the hot ones are held to one answer"""
    maxo, thr, ow, dw = C.EXPORT_CASES[name]
    s = C.oracle_scale_space("256x192")
    want = C.oracle_features("256x192", maxo, thr, ow, dw)
    stage4, idx4 = s.keypoints(4)
    checked = C.checked_lists("256x192", dw)
    pos = 0
    for o in range(4):
        w, h, pw, _ = s.octave_info(o)
        l4 = stage4[pos:pos + int(idx4[o][5])]
        pos += len(l4)
        if not len(l4):
            continue
        kp_d = _dev(l4)
        for b, start, cnt in _segments(idx4[o], len(l4)):
            if cnt > 0:
                capi.check(capi.LIB.ssrlcv_hip_check_keypoints(u32(cnt), u32(start), u32(w), u32(h), f32c(pw), f32c(dw), capi.ptr(kp_d), capi.stream_ptr()))
        n = _compact(capi, capi.LIB.ssrlcv_hip_compact_keypoints, kp_d, len(l4))
        _assert_same(capi.to_host(kp_d, H.SSKEYPOINT, n), checked[o][0], KP_FIELDS[:5], "%s, check_keypoints of octave %d" % (name, o))
    levels = {o: [s.level(2, o, b) for b in range(5)] for o in range(4)}
    geoms = [s.octave_info(o)[:3] for o in range(4)]
    _, got = _export_chain(capi, levels, geoms, checked, maxo, thr, ow, dw)
    assert len(want) > 400
    _assert_features(got, want, name)


# ---- part 2: hand-placed key points on the hot kernels --------------------------------------------------------------------------------
def _inject(capi, plan, lists):
    """Overwrites the current key-point list and the state words (idx[0..4], n, hasExtrema, overflow: the first eight ints of
    OctaveState) of every octave through the device pointers of ssrlcv_sift_plan_keypoints."""
    base = plan.workspace.data_ptr()
    for o, (kps, idx) in enumerate(lists):
        lst, st = ctypes.c_void_p(), ctypes.c_void_p()
        capi.check(capi.LIB.ssrlcv_sift_plan_keypoints(plan.handle, capi.ptr(plan.workspace), ci(o), ctypes.byref(lst), ctypes.byref(st)))
        assert len(kps) <= C.CAPACITY
        state = np.zeros(8, np.int32)
        state[:5], state[5], state[6] = idx, len(kps), 1 if len(kps) else 0
        soff, loff = st.value - base, lst.value - base
        assert 0 <= soff and soff + 32 <= plan.workspace.numel() and 0 <= loff and loff + 32 * C.CAPACITY <= plan.workspace.numel()
        plan.workspace[soff:soff + 32].copy_(torch.from_numpy(state.view(np.uint8)))
        if len(kps):
            raw = np.ascontiguousarray(kps).view(np.uint8).reshape(-1).copy()
            plan.workspace[loff:loff + raw.size].copy_(torch.from_numpy(raw))
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def placed_image_d(capi):
    w, h, seed = C.PLACED_IMAGE
    return capi.to_dev(H.synthetic_image(w, h, seed=seed))


@pytest.mark.parametrize("name", list(C.SETS))
def test_hand_placed_key_points_through_the_plan(capi, placed_image_d, name):
    """build_dog, stages 0..5, the lists of all four octaves overwritten, stages 6 and 7 (an already oriented list: stages 0..6,
    overwritten, stage 7, which books from the state it finds) == the per-key-point oracle on the oracle's levels"""
    spec = C.SETS[name]
    ow, dw = C.PAIRS[spec.pair]
    lists, ref = C.build_set(name), C.reference(name)
    for o, (kps, idx) in enumerate(lists):
        C.check_preconditions(o, dw, kps, idx)
    describe = _placed_describer(ref["expanded"], ow, dw)
    plan = capi.SiftPlan(C.PLACED_IMAGE[0], C.PLACED_IMAGE[1], C.PLACED_MAXO, C.PLACED_THR, ow, dw, max_keypoints_per_octave=C.CAPACITY)
    plan.build_dog(placed_image_d)
    for stage in range(7 if spec.oriented else 6):
        plan.stage(stage)
    _inject(capi, plan, lists)
    if not spec.oriented:
        plan.stage(6)
        pos = 0
        for o in range(4):
            g, gidx, overflow = plan.keypoints(o, H.SSKEYPOINT)
            want = ref["expanded"][o]
            assert overflow == 0
            _assert_same(g, want, KP_FIELDS, "%s, octave %d after stage 6" % (name, o), lambda i, pos=pos: describe(pos + i))
            assert len(want) == 0 or np.array_equal(gidx[:5], ref["idx"][o]), (o, gidx, ref["idx"][o])
            pos += len(want)
    plan.stage(7)
    _assert_features(plan.features_host(H.FEATURE), ref["features"], name + ", stage 7", describe)


@pytest.mark.parametrize("name", list(C.SETS))
def test_hand_placed_key_points_through_the_exports(capi, name):
    """the same lists through the plain export kernels, no injection: both kernel families are held to the same answers"""
    spec = C.SETS[name]
    ow, dw = C.PAIRS[spec.pair]
    lists, ref = C.build_set(name), C.reference(name)
    describe = _placed_describer(ref["expanded"], ow, dw)
    geoms = [tuple(C.geometry(o)[:3]) for o in range(4)]
    expanded, got = _export_chain(capi, C.placed_levels(), geoms, lists, C.PLACED_MAXO, C.PLACED_THR, ow, dw, oriented=spec.oriented)
    pos = 0
    for o in range(4):
        _assert_same(expanded[o], ref["expanded"][o], KP_FIELDS, "%s, octave %d expanded" % (name, o), lambda i, pos=pos: describe(pos + i))
        pos += len(ref["expanded"][o])
    _assert_features(got, ref["features"], name + ", fill_descriptors", describe)
