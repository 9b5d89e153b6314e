"""Surface registration, the part that needs no GPU: the header, the loader and the binders name the entry points, the records
have their sizes, every refusal of include/ssrlcv_hip.h "surface registration" is decided on the host in the contract's order
before a buffer is looked at (the device pointers here are bogus or null, so nothing is launched), the workspace query follows the
header's formula, the host steps -- ssrlcv_register_step_host, ssrlcv_register_compose_host -- are held to float64 restatements on
the reference's own records, the C++ mirror program compiles, k_register_terms uses no scratch, and the tool and the documents
exist."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import register_cases as C
import register_ref as R
from test_dsm_host import BAD_FRAMES, BOGUS, INF, INVALID_ARG, NAN, OK, UNSUPPORTED, WORKSPACE, a256, frame

u32, f32, f64, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p
QUERY = "ssrlcv_hip_register_terms_workspace_bytes"
NAMES = [QUERY, "ssrlcv_hip_register_terms", "ssrlcv_hip_transform_points", "ssrlcv_register_step_host", "ssrlcv_register_compose_host"]


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    getattr(lb, QUERY).restype = csz
    return lb


def cpose(g=None, **change):
    from ssrlcv_amd import capi
    p = capi.RegisterPose.from_buffer_copy((R.pose() if g is None else g).tobytes())
    for k, v in change.items():     # m3=NAN, pivot1=INF
        (p.m if k[0] == "m" else p.pivot)[int(k.lstrip("mpivot"))] = v
    return p


def terms(lib, fr=True, n=1000, pose=True, prm=True, center=0.0, gate=1.0, points=BOGUS, height=BOGUS + 0x1000, cells=BOGUS + 0x2000, out=BOGUS + 0x3000,
          ws=BOGUS + 0x4000, ws_bytes=1 << 50, pose_args=None, **frame_args):
    from ssrlcv_amd import capi
    f = ctypes.byref(frame(**frame_args)) if fr else None
    g = ctypes.byref(cpose(**(pose_args or {}))) if pose else None
    p = ctypes.byref(capi.RegisterParams(center, gate)) if prm else None
    return lib.ssrlcv_hip_register_terms(vp(points), u32(n), g, vp(height), f, vp(cells), p, vp(out), vp(ws), csz(ws_bytes), vp(None))


def transform(lib, n=1000, pose=True, points=BOGUS, out=BOGUS + 0x100000, pose_args=None):
    g = ctypes.byref(cpose(**(pose_args or {}))) if pose else None
    return lib.ssrlcv_hip_transform_points(vp(points), u32(n), g, vp(out), vp(None))


def formula(n):
    """the header's: a256(288 T(n)) + a256(288 T(T(n))), T(n) = ceil(n / 4096)"""
    t = lambda k: (k + 4095) // 4096  # noqa: E731
    return a256(288 * t(n)) + a256(288 * t(t(n)))


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name), name
    assert "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4      # additions keep the number
    acc_at, reg_at, over_at = header.index("---- surface accuracy"), header.index("---- surface registration"), header.index("int ssrlcv_sift_plan_overflow")
    assert acc_at < header.index("int ssrlcv_hip_difference_stats(") < reg_at < over_at       # behind surface accuracy, before the overflow section
    accuracy = re.sub(r"\n \*\s+", " ", header[acc_at:reg_at])
    assert "shift search" in accuracy and '"surface registration"' in accuracy             # the accuracy section points here
    section = re.sub(r"\n \*\s+", " ", header[reg_at:over_at])
    for text in ("p'.r = (((m[4r] p.x) + (m[4r+1] p.y)) + (m[4r+2] p.z)) + m[4r+3]", "word for word", "T0: rs = zd - zc, rt = zc - za",
                 "T1: rs = zb - za, rt = zd - zb", "T0: rs = zb - za, rt = zc - za", "T1: rs = zd - zc, rt = zd - zb", "gu = rs / cell",
                 "G.k = (ez.k - (gu ex.k)) - (gv ey.k)", "len = sqrtf(((G.x G.x) + (G.y G.y)) + (G.z G.z))", "e = d / len", "L = p' - pivot",
                 "(L.y N.z) - (L.z N.y)", "J6 = ((L.x N.x) + (L.y N.y)) + (L.z N.z)", "fabsf(d - center) <= gate", "l + 256 r",
                 "acc[l] += acc[l + half]", "a256(288 T(n)) + a256(288 T(T(n)))", "INTEGER atomics", "no float atomics", "bit-equal run to run",
                 "2^-30", "Rodrigues", "rounded once to float", "out == points is legal", "copied bit for bit", "ssrlcv_register_pose; /* 60 bytes */",
                 "ssrlcv_register_params; /* 8 bytes */", "ssrlcv_register_terms; /* 304 bytes */", "cloud-to-cloud ICP"):
        assert text in section, text
    assert ctypes.sizeof(capi.RegisterPose) == 60 and ctypes.sizeof(capi.RegisterParams) == 8 and ctypes.sizeof(capi.RegisterTerms) == 304
    assert capi.RegisterPose.pivot.offset == 48 and capi.RegisterTerms.jtj.offset == 16 and capi.RegisterTerms.jte.offset == 240
    assert capi.RegisterTerms.ee.offset == 296 and R.RECORD.fields["jte"][1] == 240 and R.POSE.fields["pivot"][1] == 48
    sig = inspect.signature
    assert list(sig(capi.register_terms).parameters)[:7] == ["points_d", "pose", "height_d", "frame", "cells_d", "center", "gate"]
    assert list(sig(capi.transform_points).parameters)[:2] == ["points_d", "pose"]
    assert list(sig(capi.register_step).parameters) == ["terms", "dof_mask", "damping"]
    assert list(sig(capi.register_compose).parameters) == ["pose", "delta"]
    assert list(sig(pipeline.transform_cloud).parameters) == ["points", "pose"]
    assert list(sig(pipeline.surface_register).parameters) == ["points", "reference", "frame", "max_jump", "dof", "iterations", "gate", "initial", "damping"]
    defaults = {k: p.default for k, p in sig(pipeline.surface_register).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(max_jump=None, dof="rigid", iterations=8, gate=3.0, initial=None, damping=0.0)
    accuracy_params = list(sig(pipeline.surface_accuracy).parameters)
    assert accuracy_params[:6] == ["subject", "reference", "frame", "subject_frame", "want_map", "register"]
    assert sig(pipeline.surface_accuracy).parameters["register"].default is None
    assert (capi.REGISTER_SHIFT, capi.REGISTER_RIGID, capi.REGISTER_SIMILARITY) == (0x07, 0x3F, 0x7F)


def test_terms_refusals_in_the_contract_s_order(lib):
    null_all = dict(points=None, height=None, cells=None, out=None, ws=None, ws_bytes=0)
    for bad in BAD_FRAMES + [dict(w=65536, h=32768)]:
        assert terms(lib, **bad) == INVALID_ARG, bad
        assert terms(lib, n=0, **null_all, **bad) == INVALID_ARG, bad
    assert terms(lib, fr=False) == INVALID_ARG
    assert terms(lib, w=(1 << 24) + 1, h=1 << 10) == INVALID_ARG                       # w h >= 2^31 before the side
    # the pose and the parameters before the side
    long_side = dict(w=(1 << 24) + 1, h=1)
    for bad in (dict(pose=False), dict(prm=False), dict(pose_args=dict(m0=NAN)), dict(pose_args=dict(m11=INF)), dict(pose_args=dict(pivot2=-INF)),
                dict(center=NAN), dict(center=INF), dict(gate=-1.0), dict(gate=NAN), dict(gate=-INF)):
        assert terms(lib, **bad) == INVALID_ARG, bad
        assert terms(lib, **long_side, **bad) == INVALID_ARG, bad
        assert terms(lib, n=0, **null_all, **bad) == INVALID_ARG, bad
    assert terms(lib, **long_side) == UNSUPPORTED and terms(lib, w=1, h=(1 << 24) + 1, out=None) == UNSUPPORTED   # the side before the record
    assert terms(lib, out=None) == INVALID_ARG and terms(lib, n=0, out=None) == INVALID_ARG                      # the record before n = 0
    for null in ("points", "height", "cells", "ws"):
        assert terms(lib, **{null: None}) == INVALID_ARG, null
        assert terms(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null            # a NULL buffer before a short workspace
    want = getattr(lib, QUERY)(u32(1000))
    assert want == formula(1000)
    assert terms(lib, ws_bytes=want - 1) == WORKSPACE and terms(lib, ws_bytes=0) == WORKSPACE
    for legal in (dict(gate=INF), dict(gate=0.0), dict(center=-3.5), dict(w=1, h=5), dict(w=0, h=0), dict(w=1, h=1)):   # a side below 2 is legal
        assert terms(lib, ws_bytes=0, **legal) == WORKSPACE, legal                    # accepted up to the size check


def test_transform_refusals_in_the_contract_s_order(lib):
    assert transform(lib, pose=False) == INVALID_ARG and transform(lib, pose=False, n=0) == INVALID_ARG
    assert transform(lib, pose_args=dict(m7=NAN)) == INVALID_ARG and transform(lib, pose_args=dict(pivot0=INF), n=0, points=None, out=None) == INVALID_ARG
    assert transform(lib, n=0, points=None, out=None) == OK                           # nothing is looked at
    assert transform(lib, points=None) == INVALID_ARG and transform(lib, out=None) == INVALID_ARG
    for shift in (4, 12, 11988, -12, -11996):                                       # partial overlap of 1000 points of 12 bytes
        assert transform(lib, points=0x100000, out=0x100000 + shift) == INVALID_ARG, shift


def test_the_workspace_formula(lib):
    query = getattr(lib, QUERY)
    for n in (0, 1, 4096, 4097, 4096 * 4096, 4096 * 4096 + 5, (1 << 32) - 1):
        assert query(u32(n)) == formula(n), n
    assert formula(4096 * 4096 + 5) == a256(288 * 4097) + a256(288 * 2) and formula(0) == 0 and formula(1) == 1024


def record_of(rec):
    from ssrlcv_amd import capi
    return capi.RegisterTerms.from_buffer_copy(rec.tobytes())


def test_the_step_equals_numpy_s_solve_on_the_reference_s_records():
    """|delta - delta_ref|inf <= 64 cond(H) 2^-52 |delta_ref|inf, cond(H) computed here"""
    from ssrlcv_amd import capi
    records = [(name, C.terms_reference(name)) for name in ("relief/rigid", "relief/similarity/gated", "n8193", "skew_frame/gated", "n257")]
    records.append(("scene", C.scene_reference("similarity", None, False)[0]["history"][0]["terms"]))
    for name, rec in records:
        for mask in (0x07, 0x3F, 0x7F, 0x24, 0x40, 0x5B):
            for damping in (0.0, 0.5):
                idx = [k for k in range(7) if mask >> k & 1]
                Hm = R.normal_matrix(rec, damping)[np.ix_(idx, idx)]
                cond = np.linalg.cond(Hm)
                assert cond < 2.0 ** 20, (name, mask)
                want = np.zeros(7)
                want[idx] = np.linalg.solve(Hm, -np.asarray(rec["jte"])[idx])
                got = capi.register_step(record_of(rec), mask, damping)
                assert got is not None and (got[[k for k in range(7) if k not in idx]] == 0).all()
                assert np.abs(got - want).max() <= 64 * cond * 2.0 ** -52 * np.abs(want).max(), (name, hex(mask), damping, cond)
                if name == "scene" and mask == 0x7F and damping == 0.0:
                    print("cond(H) on the scene over all seven unknowns: %.1f" % cond)
                    assert 10 < cond < 1000


def test_the_step_refuses_what_it_cannot_answer(lib):
    from ssrlcv_amd import capi
    rec = record_of(C.terms_reference("n8193"))
    delta = (f64 * 7)(*[7.0] * 7)
    step = lambda r, mask, lam, d: lib.ssrlcv_register_step_host(ctypes.byref(r) if r is not None else None, u32(mask), f64(lam), d)  # noqa: E731
    for bad in ((None, 0x3F, 0.0, delta), (rec, 0x3F, 0.0, None), (rec, 0, 0.0, delta), (rec, 0x80, 0.0, delta), (rec, 0xFFFFFFFF, 0.0, delta),
                (rec, 0x3F, -0.5, delta), (rec, 0x3F, NAN, delta), (rec, 0x3F, INF, delta)):
        assert step(*bad) == INVALID_ARG, bad[1:3]
    assert step(record_of(C.terms_reference("grid_1x5")), 0x3F, 0.0, delta) == UNSUPPORTED          # used = 0
    assert step(record_of(C.terms_reference("n0")), 0x01, 0.0, delta) == UNSUPPORTED
    assert list(delta) == [7.0] * 7                                                                  # untouched on error
    assert step(rec, 0x3F, 0.0, delta) == OK and delta[6] == 0.0 and delta[0] != 7.0
    dup = C.terms_reference("n8193").copy()                 # tx twice as ty: the second pivot is 0 up to rounding
    Hm = R.normal_matrix(dup)
    Hm[1, :], Hm[:, 1] = Hm[0, :], Hm[:, 0]
    Hm[1, 1] = Hm[0, 0]
    dup["jtj"] = [Hm[i, j] for (i, j) in R.PAIRS]
    assert capi.register_step(record_of(dup), 0x3F) is None and capi.register_step(record_of(dup), 0x3D) is not None


def test_a_flat_reference_holds_no_shift_in_x_and_answers_the_mean_in_z():
    from ssrlcv_amd import capi
    c = C.flat_case()
    cells = C.M.mesh(c.height, 1, c.max_jump)[1]
    rows = R.rows(c.points, c.pose, c.height, c.frame, cells)
    rec = R.terms(c.points, c.pose, c.height, c.frame, cells)
    used = rows["used"]
    assert used.sum() > 300 and (rows["J"][used, 0] == 0).all() and (rows["J"][used, 2] == 1).all() and (rows["e"][used] == rows["d"][used]).all()
    assert rec["jtj"][0] == 0.0                                            # N.x is exactly 0: the pivot of tx is 0
    assert capi.register_step(record_of(rec), 0x05) is None                # tx | tz is refused
    assert capi.register_step(record_of(rec), 0x07) is None
    got = capi.register_step(record_of(rec), 0x04)
    d = rows["d"][used].astype(np.float64)                                 # multiples of 1/8: every sum is exact
    assert rec["jte"][2] == d.sum() and rec["jtj"][R.PAIRS.index((2, 2))] == used.sum()
    assert got.tolist() == [0.0, 0.0, -(d.sum() / used.sum()), 0.0, 0.0, 0.0, 0.0] and got[2] != 0


def near32(got, want):
    """every float32 entry is the float64 value rounded, or its float32 neighbour (tests/test_ortho_host.py assert_view's rule)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float64)
    want32 = want.astype(np.float32)
    near = (got == want32) | (got == np.nextafter(want32, np.float32(INF))) | (got == np.nextafter(want32, np.float32(-INF)))
    return near.all() and (np.abs(got.astype(np.float64) - want) <= np.abs(want) * 2.0 ** -23 + 1e-300).all()


DELTAS = [np.zeros(7), np.array([0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, 0.01, -0.02, 0.5, 0.0]),
          np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.02]), np.array([0.1, -0.2, 0.3, 0.01, -0.02, 0.5, 0.02]),
          np.array([1e-3, 2e-3, -1e-3, 1e-9, -2e-9, 1e-9, -1e-4]), np.array([0.0, 0.0, 0.0, 1e-30, 0.0, 0.0, 0.0]),
          np.array([0.5, 0.5, 0.5, 2.0, -1.5, 3.0, -0.25])]


def test_compose_is_the_float64_restatement_rounded_once():
    from ssrlcv_amd import capi
    for g in (C.IDENTITY, C.RIGID, C.SIMILARITY, C.HALF_OFF):
        for delta in DELTAS:
            out = capi.register_compose(cpose(g), delta)
            Mx, T = R.compose64(g, delta)
            assert near32(np.array(out.m[:]).reshape(3, 4)[:, :3], Mx) and near32(np.array(out.m[:]).reshape(3, 4)[:, 3], T), (g, delta)
            assert list(out.pivot) == list(cpose(g).pivot)                     # carried over
    assert bytes(capi.register_compose(cpose(C.RIGID), np.zeros(7))) == C.RIGID.tobytes()
    Rm = R.rotation((0.3, -0.2, 0.9))
    assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(Rm) - 1) < 1e-15
    assert np.allclose(R.rotation((0, 0, np.pi / 2)) @ [1, 0, 0], [0, 1, 0], atol=1e-15)


def test_a_composed_pose_applied_is_the_step_formula(lib):
    """p'' = pivot + (1 + ds) R(dw) (p' - pivot) + dt in float64, against the composed float32 pose applied in float64: the two differ
    by the rounding of the twelve entries alone"""
    from ssrlcv_amd import capi
    pts = C.TERMS["relief/rigid"].points
    pts = pts[~R.skipped(pts) & (np.abs(pts) < 100).all(1)].astype(np.float64)
    for g in (C.RIGID, C.SIMILARITY):
        c = np.asarray(g["pivot"], np.float64)
        for delta in DELTAS[1:]:
            out = np.frombuffer(bytes(capi.register_compose(cpose(g), delta)), R.POSE)[0]
            first = R.apply64(g, pts)
            want = c + (1 + delta[6]) * (first - c) @ R.rotation(delta[3:6]).T + delta[:3]
            scale = np.abs(pts).max() * 3 + np.abs(c).max() + 1
            assert np.abs(R.apply64(out, pts) - want).max() <= 4 * 2.0 ** -24 * scale * (1 + abs(delta[6])) + 1e-12
    null = lib.ssrlcv_register_compose_host
    d = (f64 * 7)(*[0.0] * 7)
    out = cpose()
    assert null(None, d, ctypes.byref(out)) == INVALID_ARG and null(ctypes.byref(cpose()), None, ctypes.byref(out)) == INVALID_ARG
    assert null(ctypes.byref(cpose()), d, None) == INVALID_ARG and null(ctypes.byref(cpose(m5=NAN)), d, ctypes.byref(out)) == INVALID_ARG
    assert null(ctypes.byref(cpose()), (f64 * 7)(0, 0, NAN, 0, 0, 0, 0), ctypes.byref(out)) == INVALID_ARG
    assert null(ctypes.byref(cpose()), (f64 * 7)(1e39, 0, 0, 0, 0, 0, 0), ctypes.byref(out)) == UNSUPPORTED and bytes(out) == bytes(cpose())


def test_the_mirror_program_compiles_and_the_class_api_names_the_calls():
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/register_test"])
    r = subprocess.run([os.path.join(host, "_build", "register_test")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    factory = open(os.path.join(host, "MeshFactory.hpp")).read()
    for member in ("Registration registerToReference(ptr::value<Unity<float3>> cloud, uint32_t dofMask = 0x3Fu, unsigned iterations = 8, float gateFactor = 3.0f",
                   "ssrlcv_hip_register_terms(", "ssrlcv_register_step_host(", "ssrlcv_register_compose_host(", "ssrlcv_hip_transform_points("):
        assert member in factory, member
    clouds = open(os.path.join(host, "PointCloudFactory.hpp")).read()
    for member in ("void transformPointCloud(ptr::value<Unity<float3>> cloud, const ssrlcv_register_pose& pose)", "void scalePointCloud(",
                   "void translatePointCloud(", "void rotatePointCloud(", "then y, then z", "ssrlcv_hip_transform_points("):
        assert member in clouds, member


def test_the_kernel_uses_no_scratch():
    """the method of tests/test_capi_symbols.py test_matcher_kernels_register_budget: the compiler's resource report"""
    csrc = os.path.join(H.ROOT, "ssrlcv_amd", "csrc")
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
                          "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(csrc, "register.hip"), "-o", os.devnull], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    kernels = {k: [v for n, v in usage.items() if k in n] for k in ("k_register_terms", "k_register_reduce", "k_transform_points")}
    for k, found in kernels.items():
        assert len(found) == 1 and found[0]["ScratchSize [bytes/lane]"] == 0 and found[0]["VGPRs Spill"] == 0, (k, found)
    t = kernels["k_register_terms"][0]
    print("k_register_terms: %d VGPRs, %d waves/SIMD, %d B of LDS a block" % (t["VGPRs"], t["Occupancy [waves/SIMD]"], t["LDS Size [bytes/block]"]))
    assert t["LDS Size [bytes/block]"] <= 32 * 1024 and t["Occupancy [waves/SIMD]"] >= 2


def test_the_documents_and_the_bench_tool_exist():
    root = H.ROOT
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "Surface registration" in design
    for kernel in ("k_register_terms", "k_register_reduce", "k_transform_points"):
        assert kernel in design, kernel
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(root, doc)).read()
        assert "ssrlcv_hip_register_terms" in text and "ssrlcv_hip_transform_points" in text and "surface_register" in text, doc
    assert "register_bench.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    assert os.path.exists(os.path.join(root, "tools", "bench_register.py"))
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "register.hip")).read()
    assert "atomicAdd(float" not in source and "unsafeAtomicAdd" not in source and "atomicAdd(double" not in source      # no float atomic
    assert '#include "mesh_lookup.h"' in source and '#include "mesh_lookup.h"' in open(os.path.join(root, "ssrlcv_amd", "csrc", "accuracy.hip")).read()
    assert "register.hip" in open(os.path.join(root, "ssrlcv_amd", "csrc", "Makefile")).read()
