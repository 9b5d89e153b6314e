"""GPU: a key-point list that outgrows the plan's capacity is truncated AT the capacity in the reference's order, the octave's bit
is set in the mask and ssrlcv_sift_plan_overflow returns SSRLCV_ERR_CAPACITY (include/ssrlcv_hip.h); a list that fits exactly is
not flagged, one record more is.  Cases: tests/overflow_cases.py, proven on the oracle alone by tests/test_overflow_cases.py.
Every comparison is bit for bit.

Every plan of this file has 4096 guard bytes of 0xA5 behind its workspace and behind its feature array; after every run both
tails must still hold 0xA5.  The lists lie in the middle of the workspace, so a record past the capacity would not reach a tail: the
first-list tests also hold the bytes directly behind the list's capacity to the fill pattern, the hand-placed expansion tests to what
a run that fits leaves there.  The device code under test: the `d >= cap` drop in stage_extrema's emit with book_extrema's clamps;
the `at < cap` drop of expand_orient_piece with its min(start, cap) blur indices and the running offset across pieces;
k_build_desc_ranges_oct0's clamp; the older per-octave hand-overs (csrc/keypoints.hip)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import overflow_cases as V
import sampling_cases as C
import test_gpu_sampling as S

pytestmark = pytest.mark.gpu

u32, f32c, ci = ctypes.c_uint32, ctypes.c_float, ctypes.c_int
TAIL, GUARD = 4096, 0xA5
NOISE, EDGE = 0.01, 12.1


@pytest.fixture(scope="module")
def capi():
    from ssrlcv_amd import capi
    return capi


# ---- plans with guard tails, and what a run left ---------------------------------------------------------------------------------
def guarded_plan(capi, name_or_size, cap, maxo=2, thr=0.8, ow=1.5, dw=6.0):
    h, w = V.image(name_or_size).shape if isinstance(name_or_size, str) else (name_or_size[1], name_or_size[0])
    plan = capi.SiftPlan(w, h, maxo, thr, ow, dw, max_keypoints_per_octave=cap, alloc=False)
    plan.workspace = torch.full((plan.workspace_bytes + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
    plan.features = torch.full((plan.max_features * 152 + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
    plan.num_features = torch.zeros(1, dtype=torch.int32, device="cuda")
    return plan


def assert_tails(plan, what):
    torch.cuda.synchronize()
    assert bool((plan.workspace[plan.workspace_bytes:] == GUARD).all()), what + ": written behind the workspace"
    assert bool((plan.features[plan.max_features * 152:] == GUARD).all()), what + ": written behind the feature array"


def overflow(capi, plan):
    """-> (return code, mask) of ssrlcv_sift_plan_overflow"""
    mask = u32(0)
    rc = capi.LIB.ssrlcv_sift_plan_overflow(plan.handle, capi.ptr(plan.workspace), ctypes.byref(mask), capi.stream_ptr())
    return int(rc), int(mask.value)


def offsets(capi, plan, o):
    """-> byte offsets in the workspace of the octave's current list and of its state words"""
    lst, st = ctypes.c_void_p(), ctypes.c_void_p()
    capi.check(capi.LIB.ssrlcv_sift_plan_keypoints(plan.handle, capi.ptr(plan.workspace), ci(o), ctypes.byref(lst), ctypes.byref(st)))
    torch.cuda.synchronize()
    base = plan.workspace.data_ptr()
    return lst.value - base, st.value - base


def octave(capi, plan, o):
    """-> (SSKEYPOINT[] of the octave, its eight state words)"""
    loff, soff = offsets(capi, plan, o)
    state = plan.workspace[soff:soff + 32].view(torch.int32).cpu().numpy().copy()
    n = int(state[5]) if int(state[6]) else 0
    assert 0 <= n and loff + 32 * n <= plan.workspace_bytes
    return capi.to_host(plan.workspace[loff:loff + 32 * max(n, 1)], H.SSKEYPOINT, n), state


def assert_nothing_behind_the_first_list(capi, plan, cap, what):
    """guarded_plan fills the whole workspace with the guard byte, and the search for extrema writes its list and nothing else of the
    list region: on a plan that has only run the first stage (0, or the fused calls' 0 + 1), the 4096 bytes behind the capacity of every octave's list (the other
    ping-pong list, first written by the stage behind) still hold it.  This is where a record past `cap` would land."""
    for o in range(4):
        loff, _ = offsets(capi, plan, o)
        behind = plan.workspace[loff + 32 * cap:loff + 32 * cap + TAIL]
        assert bool((behind == GUARD).all()), "%s, octave %d: written behind the list's capacity" % (what, o)


def features_of(capi, plan):
    """the feature array as the last run left it, overflow or not (SiftPlan.features_host raises on overflow) -> FEATURE[]"""
    torch.cuda.synchronize()
    n = int(plan.num_features.item())
    assert 0 <= n <= plan.max_features
    return capi.to_host(plan.features[:152 * max(n, 1)], H.FEATURE, n)


def assert_octave(capi, plan, o, want, stage, what):
    """the octave's list and state words == want = (SSKEYPOINT[], state words[8]); an empty list's blur indices are not held"""
    lst, st = want
    got, gst = octave(capi, plan, o)
    what = "%s, octave %d" % (what, o)
    S._assert_same(got, lst, S.KP_FIELDS if stage >= 6 else S.KP_FIELDS[:5], what)
    assert (got["discard"] == 0).all(), what
    if len(lst):
        assert np.array_equal(gst, st), (what, gst.tolist(), st.tolist())
    else:
        assert gst[7] == 0 and (gst[6] == 0 or gst[5] == 0), (what, gst.tolist())


def assert_report(capi, plan, states, what):
    rc, mask = overflow(capi, plan)
    want = V.mask_of(states)
    assert mask == want, (what, bin(mask), bin(want))
    assert rc == (V.ERR_CAPACITY if want else V.OK), (what, rc)


def run(capi, plan, name, how, stop=None):
    """how: "extract", "describe" (build_dog + describe) or "stage" (build_dog + the stage calls up to `stop`)"""
    img_d = capi.to_dev(V.image(name))
    if how != "stage" and stop is not None:
        plan.set_stop_stage(stop)
    if how == "extract":
        plan.extract(img_d)
    else:
        plan.build_dog(img_d)
        if how == "describe":
            plan.describe()
        else:
            for s in range(stop + 1):
                plan.stage(s)
    assert_tails(plan, "%s, %s" % (name, how))


# ---- a. the raw extrema list (the stage call, describe stopped at stage 0) ------------------------------------------------------------
@pytest.mark.parametrize("how", ["describe", "stage"])
@pytest.mark.parametrize("case", V.STAGED_EXTREMA, ids=lambda c: "%s-%d" % (c.image, c.cap))
def test_raw_extrema_truncate_at_the_capacity(capi, case, how):
    """every octave == truncate_extrema of the oracle's stage-0 list; the mask names the octaves that were cut, no other"""
    plan = guarded_plan(capi, case.image, case.cap)
    run(capi, plan, case.image, how, stop=0)
    what = "%s at %d, %s" % (case.image, case.cap, how)
    assert_nothing_behind_the_first_list(capi, plan, case.cap, what)
    want = [V.truncate_extrema(l, idx, case.cap) for l, idx in V.lists(case.image, 0)]
    for o in range(4):
        assert_octave(capi, plan, o, want[o], 0, what)
    assert_report(capi, plan, [st for _, st in want], what)
    cut = {0} | set(V.ALSO_OVERFLOWS.get((case.image, case.cap), {}))
    assert V.mask_of([st for _, st in want]) == (0 if "exact fit" in case.claim else sum(1 << o for o in cut))


# ---- b. the first list of the fused calls: the extrema behind the first removeNoise ---------------------------------------------------
def fused_extrema(capi, case, how):
    plan = guarded_plan(capi, case.image, case.cap)
    run(capi, plan, case.image, how, stop=1)
    what = "%s at %d, %s stopped at stage 1" % (case.image, case.cap, how)
    assert_nothing_behind_the_first_list(capi, plan, case.cap, what)
    want = [V.truncate_extrema(l, idx, case.cap) for l, idx in V.lists(case.image, 1)]
    for o in range(4):
        assert_octave(capi, plan, o, want[o], 1, what)
    assert_report(capi, plan, [st for _, st in want], what)
    assert V.mask_of([st for _, st in want]) == (0 if "exact fit" in case.claim else 1)


@pytest.mark.parametrize("how", ["extract", "describe"])
@pytest.mark.parametrize("case", V.FUSED_EXTREMA, ids=lambda c: "%s-%d" % (c.image, c.cap))
def test_fused_extrema_truncate_at_the_capacity(capi, case, how):
    fused_extrema(capi, case, how)


# ---- c. downstream of an extrema truncation ---------------------------------------------------------------------------------------------
def assert_downstream_of_cut_extrema(capi, plan, name, cap, what):
    """after a full fused extract whose octave-0 extrema were cut: the flag survives the later bookkeeping, octave 0 keeps at most
    cap records, octaves 1-3 give the oracle's features behind them -> the features"""
    rc, mask = overflow(capi, plan)
    assert (rc, mask) == (V.ERR_CAPACITY, 0b0001), (what, rc, bin(mask))
    per_octave = V.features_per_octave(name)
    kept = []
    for o, (lst, idx) in enumerate(V.lists(name, 6)):
        if o == 0:
            got, st = octave(capi, plan, 0)
            assert st[7] == 1 and st[6] == 1 and 0 < st[5] <= cap and len(got) == st[5], (what, st.tolist())
            kept.append(int(st[5]))
        else:
            assert_octave(capi, plan, o, (lst, V.state_words(idx, len(lst), 0)), 6, what)
            kept.append(len(lst))
    feats = features_of(capi, plan)
    assert len(feats) == sum(kept), (what, len(feats), kept)
    S._assert_features(feats[kept[0]:], np.concatenate(per_octave[1:]), what + ", octaves 1-3 behind octave 0's %d" % kept[0])
    return feats


def _export_stage(capi, kp_d, n, geom, dogn, ptrs, sig, stage, idx):
    """one reference launch site on a device list through the plain export kernels + discardExtrema's remove_if -> the new count"""
    L, (w, h, pw) = capi.LIB, geom
    if stage in (1, 3):
        capi.check(L.ssrlcv_hip_flag_noise(u32(n), capi.ptr(kp_d), f32c(np.float32(NOISE * 0.8) if stage == 1 else np.float32(NOISE)), capi.stream_ptr()))
    elif stage == 2:
        capi.check(L.ssrlcv_hip_refine_location(u32(n), u32(w), u32(h), f32c(float(sig[0])), f32c(float(sig[1] / sig[0])), u32(5), capi.ptr(ptrs),
                                                capi.ptr(kp_d), capi.stream_ptr()))
    else:
        for b, start, cnt in S._segments(idx, n):
            if cnt <= 0:
                continue
            if stage == 4:
                capi.check(L.ssrlcv_hip_flag_edges(u32(cnt), u32(start), u32(w), u32(h), capi.ptr(kp_d), capi.ptr(dogn[b]), f32c(EDGE), capi.stream_ptr()))
            else:
                capi.check(L.ssrlcv_hip_check_keypoints(u32(cnt), u32(start), u32(w), u32(h), f32c(pw), f32c(6.0), capi.ptr(kp_d), capi.stream_ptr()))
    return S._compact(capi, L.ssrlcv_hip_compact_keypoints, kp_d, n)


def test_downstream_of_an_extrema_truncation(capi):
    name, cap = "syn512", 4096
    plan = guarded_plan(capi, name, cap)
    run(capi, plan, name, "extract")
    assert_downstream_of_cut_extrema(capi, plan, name, cap, "syn512 at 4096, extract")
    # a write that left its list but stayed inside the workspace: the DoG levels are still the oracle's
    s = V.scale_space(name)
    for o in range(4):
        for b in range(5):
            lvl, mm = plan.level(0, o, b)
            assert np.array_equal(H.bits(lvl), H.bits(s.level(1, o, b))) and mm == s.minmax(1, o, b), (o, b)
    # octave 0's own content: the stage calls on the cut stage-0 list == the plain export kernels on the same cut list
    staged = guarded_plan(capi, name, cap)
    staged.build_dog(capi.to_dev(V.image(name)))
    w, h, pw, sig = s.octave_info(0)
    dogn = [S._dev(s.level(2, 0, b)) for b in range(5)]
    ptrs = torch.tensor([t.data_ptr() for t in dogn], dtype=torch.int64, device="cuda")
    lst, st = V.truncate_extrema(*V.lists(name, 0)[0], cap)
    assert len(lst) == cap
    idx = st[:5]
    for stage in range(6):
        staged.stage(stage)
        assert_tails(staged, "stage %d" % stage)
        if stage:
            kp_d = S._dev(lst)
            n = _export_stage(capi, kp_d, len(lst), (w, h, pw), dogn, ptrs, sig, stage, idx)
            lst = capi.to_host(kp_d, H.SSKEYPOINT, n)
            if stage == 2:      # thrust::stable_sort by blur is the caller's
                lst = lst[np.argsort(lst["blur"], kind="stable")]
            idx = C.partition_by_blur(lst)
            assert 0 < n
        got, gst = octave(capi, staged, 0)
        S._assert_same(got, lst, S.KP_FIELDS[:5], "octave 0 after stage %d: the stage call and the export kernels" % stage)
        assert np.array_equal(gst[:7], V.state_words(idx, len(lst), 1)[:7]), (stage, gst.tolist(), idx.tolist())
        assert gst[7] == 1, "the flag of stage 0 survives stage %d" % stage
        for o in (1, 2, 3):
            l_o, idx_o = V.lists(name, stage)[o]
            assert_octave(capi, staged, o, (l_o, V.state_words(idx_o, len(l_o), 0)), stage, "stage %d" % stage)
    assert overflow(capi, staged) == (V.ERR_CAPACITY, 0b0001)


# ---- d. the expansion overflows, the extrema fit ----------------------------------------------------------------------------------------
def expansion(capi, name, cap, how, lists, per_octave, maxo=2, thr=0.8):
    """lists / per_octave: the reference's stage-6 lists and features per octave"""
    plan = guarded_plan(capi, name, cap, maxo, thr)
    run(capi, plan, name, how)
    what = "%s at %d (maxOrientations %d), %s" % (name, cap, maxo, how)
    want = [V.truncate_expanded(l, idx, cap) for l, idx in lists]
    for o in range(4):
        assert_octave(capi, plan, o, want[o], 6, what)
    assert_report(capi, plan, [st for _, st in want], what)
    kept = [int(st[5]) for _, st in want]
    feats = features_of(capi, plan)
    assert len(feats) == sum(kept), (what, len(feats), kept)
    S._assert_features(feats, V.truncated_features(per_octave, kept), what)
    return kept


@pytest.mark.parametrize("how", ["extract", "describe"])
@pytest.mark.parametrize("case", V.EXPANSION, ids=lambda c: "%s-%d" % (c.image, c.cap))
def test_expansion_truncates_at_the_capacity(capi, case, how):
    kept = expansion(capi, case.image, case.cap, how, V.lists(case.image, 6), V.features_per_octave(case.image))
    assert kept == [min(case.cap, 5413), 737, 133, 18]
    if case.cap < 5413:     # = concat(oracle[:cap], oracle[5413:])
        f = V.features("syn512")
        assert np.array_equal(V.truncated_features(V.features_per_octave("syn512"), kept), np.concatenate([f[:case.cap], f[5413:]]))


def test_expansion_truncates_inside_a_key_point_of_four_orientations(capi):
    c = V.EXPANSION_MAXO4
    lists, per_octave = V.chain(c.image, V.MAXO4, V.THR4)
    kept = expansion(capi, c.image, c.cap, "extract", lists, per_octave, V.MAXO4, V.THR4)
    assert kept == [c.cap, 1049, 59, 2]


# ---- e. hand-placed lists whose expansion overflows ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def placed_image_d(capi):
    w, h, seed = C.PLACED_IMAGE
    return capi.to_dev(H.synthetic_image(w, h, seed=seed))


@pytest.mark.parametrize("name", list(V.PLACED_CUTS))
def test_hand_placed_expansion_overflow(capi, placed_image_d, name):
    """stages 0..5, the lists overwritten, stage 6 == truncate_expanded(reference); stage 7 == the truncated reference's features,
    octave 1's directly behind octave 0's 4096"""
    ow, dw = C.PAIRS[V.PLACED_PAIR]
    lists = V.placed_lists(name)
    for o, (kps, idx) in enumerate(lists):
        C.check_preconditions(o, dw, kps, idx)
    exp, per_octave, norient = V.placed_reference(name)

    def through_stage_6(lists):
        plan = guarded_plan(capi, C.PLACED_IMAGE[:2], C.CAPACITY, C.PLACED_MAXO, C.PLACED_THR, ow, dw)
        plan.build_dog(placed_image_d)
        for stage in range(6):
            plan.stage(stage)
        S._inject(capi, plan, lists)
        plan.stage(6)
        assert_tails(plan, name + ", stage 6")
        loff, _ = offsets(capi, plan, 0)
        return plan, loff, plan.workspace[loff + 32 * C.CAPACITY:loff + 32 * C.CAPACITY + TAIL].cpu().numpy()
    # where a record past the capacity would land: the bytes behind the expanded list are what the same plan holds there when the
    # list stops at the last key point whose orientations still fit (its first 256 key points, hence their orientations, are the same)
    m = int(np.searchsorted(np.cumsum(norient), C.CAPACITY, side="right"))
    fitting = [(lists[0][0][:m], C.partition_by_blur(lists[0][0][:m]))] + lists[1:]
    assert 256 < m < len(lists[0][0]) and len(exp[0][0]) - C.CAPACITY <= TAIL // 32
    fit_plan, fit_loff, fit_behind = through_stage_6(fitting)
    assert overflow(capi, fit_plan) == (V.OK, 0) and octave(capi, fit_plan, 0)[1][5] == int(norient[:m].sum()) <= C.CAPACITY
    plan, loff, behind = through_stage_6(lists)
    assert loff == fit_loff and np.array_equal(behind, fit_behind), name + ": written behind the expanded list's capacity"
    want = [V.truncate_expanded(l, idx, C.CAPACITY) for l, idx in exp]
    assert want[0][1][7] == 1 and want[1][1][7] == 0
    for o in range(4):
        assert_octave(capi, plan, o, want[o], 6, name + " after stage 6")
    assert_report(capi, plan, [st for _, st in want], name)
    plan.stage(7)
    assert_tails(plan, name + ", stage 7")
    kept = [int(st[5]) for _, st in want]
    assert kept[0] == C.CAPACITY and kept[1] == len(exp[1][0]) > 0 and kept[2:] == [0, 0]
    feats = features_of(capi, plan)
    S._assert_features(feats, V.truncated_features(per_octave, kept), name + ", stage 7")
    S._assert_features(feats[C.CAPACITY:], per_octave[1], name + ", octave 1 behind octave 0's 4096")
    assert overflow(capi, plan) == (V.ERR_CAPACITY, 0b0001)


# ---- f. a plan recovers on the next image -----------------------------------------------------------------------------------------------------
def re_arm(capi):
    name, cap = "syn512", 4096
    assert not V.capacity_fits(name, cap) and V.capacity_fits(V.FITS, cap)
    plan = guarded_plan(capi, name, cap)
    run(capi, plan, name, "extract")
    first = assert_downstream_of_cut_extrema(capi, plan, name, cap, "first run")
    first0 = octave(capi, plan, 0)
    run(capi, plan, V.FITS, "extract")
    assert overflow(capi, plan) == (V.OK, 0), "the flag of the run before is gone"
    for o, (lst, idx) in enumerate(V.lists(V.FITS, 6)):
        assert_octave(capi, plan, o, (lst, V.state_words(idx, len(lst), 0)), 6, "the image that fits")
    S._assert_features(features_of(capi, plan), V.features(V.FITS), "the image that fits, on a plan that had overflowed")
    run(capi, plan, name, "extract")
    again = assert_downstream_of_cut_extrema(capi, plan, name, cap, "third run")
    again0 = octave(capi, plan, 0)
    S._assert_features(again, first, "syn512 again: the first run's truncated features")
    S._assert_same(again0[0], first0[0], S.KP_FIELDS, "syn512 again: octave 0's list")
    assert np.array_equal(again0[1], first0[1])


def test_a_plan_re_arms_after_an_overflow(capi):
    re_arm(capi)


# ---- g. the developer schedules that change the list chain or the expansion ---------------------------------------------------------------------
def schedule_core(capi):
    """the core of (b), (d) and (f) through the fused extract"""
    for case in V.FUSED_EXTREMA:
        fused_extrema(capi, case, "extract")
    for case in V.EXPANSION:
        expansion(capi, case.image, case.cap, "extract", V.lists(case.image, 6), V.features_per_octave(case.image))
    re_arm(capi)


_SCHEDULE_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
from ssrlcv_amd import capi
import test_gpu_overflow as T
T.schedule_core(capi)
print("OVERFLOW OK")
"""


@pytest.fixture(scope="module")
def reference_cache(tmp_path_factory):
    """the references of schedule_core, computed once here and loaded by every child process"""
    d = str(tmp_path_factory.mktemp("overflow_references"))
    old = os.environ.get("SSRLCV_OVERFLOW_CACHE")
    os.environ["SSRLCV_OVERFLOW_CACHE"] = d
    for name in ("syn512", "noise256", V.FITS):
        for stage in (1, 6):
            V.lists(name, stage)
    V.features("syn512")
    V.features(V.FITS)
    yield d
    if old is None:
        del os.environ["SSRLCV_OVERFLOW_CACHE"]
    else:
        os.environ["SSRLCV_OVERFLOW_CACHE"] = old


@pytest.mark.parametrize("variant", [
    {"SSRLCV_SAMPLING_PIPELINED": "1"},        # octave 0's expansion in three pieces that continue each other
    {"SSRLCV_SAMPLING_PIPELINED": "1", "SSRLCV_SAMPLING_IRREGULAR": "1"},
    {"SSRLCV_NO_EARLY_CHAIN": "1"},
    {"SSRLCV_PRIO": "4"},                      # the older hand-overs: one k_expand_orient per octave, k_book_and_desc_ranges behind
    {"SSRLCV_SIFT_SERIAL": "1"},
    {"SSRLCV_THETAS_SPLIT": "1"},
], ids=lambda v: "+".join(k.replace("SSRLCV_", "") + "=" + x for k, x in v.items()))
def test_overflow_under_every_list_schedule(reference_cache, variant):
    """fused extrema cuts, expansion cuts and the re-arm under the developer switches that change the list chain or the expansion
    (developer build, one child process per switch set)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = H.dev_env(**variant)
    env["SSRLCV_OVERFLOW_CACHE"] = reference_cache
    r = subprocess.run([sys.executable, "-c", _SCHEDULE_SCRIPT % {"root": root}], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OVERFLOW OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the host mirror's re-run loop ----------------------------------------------------------------------------------------------------------------
def test_host_mirror_re_runs_until_the_lists_fit(tmp_path):
    """SIFT_FeatureFactory with setMaxKeyPointsPerOctave(4096) (tests/cpp/sift_rerun_test.cpp), one factory, four images in turn:
    syn512 (one re-run: 4096 -> 8192), syn512 again (the grown slot, no warning), then on a factory of its own the 512 x 512 noise
    image (two re-runs: -> 8192 -> 16384) and syn512 behind it (no warning): always the oracle's features"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(H.ROOT, "ssrlcv_amd", "host"), "_build/sift_rerun_test"])
    exe = os.path.join(H.ROOT, "ssrlcv_amd", "host", "_build", "sift_rerun_test")
    for names, warnings in ((("syn512", "syn512"), ([8192], [])), (("noise512", "syn512"), ([8192, 16384], []))):
        args = []
        for k, name in enumerate(names):
            raw, out = str(tmp_path / ("%s_%d.raw" % (name, k))), str(tmp_path / ("%s_%d.features" % (name, k)))
            V.image(name).tofile(raw)
            args += [raw, out]
        r = subprocess.run([exe, "4096", "512", "512"] + args, env=dict(os.environ, SSRLCV_LOG="1"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", r.stdout[-2000:] + r.stderr[-4000:]
        # the warnings of every image: the lines between its "Generating" line and the next
        per_image = []
        for line in r.stderr.splitlines():
            if "Generating SIFT features for image" in line:
                per_image.append([])
            elif "[warn] key-point capacity exceeded" in line:
                assert "(octave mask 1)" in line, line
                per_image[-1].append(int(line.split("re-running with ")[1].split()[0]))
        assert per_image == list(warnings), (names, r.stderr[-2000:])
        for k, name in enumerate(names):
            got = np.fromfile(args[2 * k + 1], np.uint8).view(H.FEATURE)
            S._assert_features(got, V.features(name), "%s through the host mirror (run %d)" % (name, k))
