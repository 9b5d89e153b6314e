"""GPU parity of the hand-overs of the key-point stage (keypoints.hip: k_orient_prologue, k_expand_orient_all).

Between the list chains and the descriptor kernel the stage runs one prologue kernel (control words, tile descriptors of
the expansions, orientation work list), the orientation kernel, and ONE expansion launch over the four octaves whose last
block also books the feature offsets and the descriptor work list.  The kernels' arithmetic is that of the staged form
(SSRLCV_PRIO=4 in the developer build); what can go wrong is state: a counter or tile descriptor that is not
cleared between calls, the block -> octave map, the per-octave "last block" test, the e / maxO arithmetic across tile
boundaries, and which of the entry points goes through which sequence.  Everything is compared with the CPU oracle, bit
for bit.

Per-octave key-point counts of the inputs on the oracle (before -> after expansion, max_orientations = 2):
  uniform noise 256^2   4578 -> 6379, 421 -> 581, 27 -> 37, 2 -> 2   (9156 elements in octave 0 = 3 look-back tiles of 4096)
  constant 128          0, 0, 0, 0
  one bright pixel      8 -> 16, 33 -> 38, 15 -> 15, 0
  synthetic 256^2 (5)   1023 -> 1387, 140 -> 191, 11 -> 14, 2 -> 3
  synthetic 64^2 (9)    39 -> 58, 3 -> 4, 0, 0
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from ssrlcv_amd import capi
    return capi


def _image(name):
    if name == "noise":
        return np.random.default_rng(1).integers(0, 256, (256, 256), dtype=np.uint8)
    if name == "const":
        return np.full((256, 256), 128, np.uint8)
    if name == "onepixel":
        img = np.zeros((256, 256), np.uint8)
        img[128, 128] = 255
        return img
    if name == "synthetic":
        return H.synthetic_image(256, 256, seed=5)
    if name == "small":
        return H.synthetic_image(64, 64, seed=9)
    raise KeyError(name)


_IMAGES = {}
_ORACLE_FEATURES = {}


def image(name):
    if name not in _IMAGES:
        _IMAGES[name] = _image(name)
    return _IMAGES[name]


def oracle_features(lib, name, max_orientations=2):
    """The oracle's features of a named image: computed once per (image, max_orientations), shared, never written to."""
    key = (name, max_orientations)
    if key not in _ORACLE_FEATURES:
        f = H.oracle_sift(lib, image(name), max_orientations=max_orientations)
        f.setflags(write=False)
        _ORACLE_FEATURES[key] = f
    return _ORACLE_FEATURES[key]


def test_one_plan_is_rearmed_between_images(capi, oracle_lib):
    """noise (several look-back tiles in octave 0) -> constant (every list empty) -> one pixel (empty last octave) ->
    synthetic -> noise on ONE plan: the prologue clears every control word and tile descriptor the call before left."""
    plan = capi.SiftPlan(256, 256)
    for name in ("noise", "const", "onepixel", "synthetic", "noise"):
        plan.extract(capi.to_dev(image(name)))
        n = plan.count()
        gf = plan.features_host(H.FEATURE)
        of = oracle_features(oracle_lib, name)
        print("%s: %d features (oracle %d)" % (name, len(gf), len(of)))
        assert n == len(gf) == len(of), (name, n, len(gf), len(of))
        if name == "const":
            assert n == 0
        else:
            assert n > 0
            H.assert_features_equal(gf, of)


@pytest.mark.parametrize("name,max_orientations,expected", [
    ("noise", 1, 5028), ("noise", 2, 6999), ("noise", 4, 7567),
    ("synthetic", 1, 1176), ("synthetic", 2, 1595), ("synthetic", 4, 1709),
])
def test_orientation_counts(capi, oracle_lib, name, max_orientations, expected):
    """Element e = key point e / maxO, orientation e % maxO: the division runs across the tile boundaries of the merged launch."""
    of = oracle_features(oracle_lib, name, max_orientations)
    assert len(of) == expected
    plan = capi.SiftPlan(256, 256, max_orientations=max_orientations)
    plan.extract(capi.to_dev(image(name)))
    assert plan.count() == expected
    H.assert_features_equal(plan.features_host(H.FEATURE), of)


def test_small_image_with_empty_octaves(capi, oracle_lib):
    """64 x 64: octaves 2 and 3 hold no key points, their blocks of the merged launch only count themselves out."""
    of = oracle_features(oracle_lib, "small")
    plan = capi.SiftPlan(64, 64)
    plan.extract(capi.to_dev(image("small")))
    assert plan.count() == len(of) == 62
    H.assert_features_equal(plan.features_host(H.FEATURE), of)


def test_entry_points_agree(capi, oracle_lib):
    """build_dog + describe (octave 0's chain on the caller's stream, tables on the side stream), the stage-at-a-time entry
    point 0..7 (everything on the caller's stream) and the fused extract (tables on the caller's stream, prologue on a side
    stream) give the same features: the oracle's."""
    img = image("synthetic")
    of = oracle_features(oracle_lib, "synthetic")
    pix = capi.to_dev(img)
    two_calls = capi.SiftPlan(256, 256)
    two_calls.build_dog(pix)
    two_calls.describe()
    staged = capi.SiftPlan(256, 256)
    staged.build_dog(pix)
    for stage in range(8):
        staged.stage(stage)
    fused = capi.SiftPlan(256, 256)
    fused.extract(pix)
    got = {}
    for label, plan in (("build_dog + describe", two_calls), ("stages 0..7", staged), ("extract", fused)):
        assert plan.count() == len(of), (label, plan.count(), len(of))
        got[label] = plan.features_host(H.FEATURE)
        H.assert_features_equal(got[label], of)
    H.assert_features_equal(got["build_dog + describe"], got["extract"])
    H.assert_features_equal(got["stages 0..7"], got["extract"])


# the image list of test_gpu_sift.py's _FEATURES_SCRIPT, every plan run twice
_VARIANT_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import helpers as H
from ssrlcv_amd import capi
lib = H.oracle()
for (w, h, seed) in [(512, 384, 5), (262, 260, 6), (640, 128, 7)]:
    img = H.synthetic_image(w, h, seed=seed)
    plan = capi.SiftPlan(w, h)
    o = H.oracle_sift(lib, img)
    for rep in range(2):
        plan.extract(capi.to_dev(img))
        g = plan.features_host(H.FEATURE)
        assert plan.count() == len(g) == len(o) and len(g) > 100, (w, h, rep, len(g), len(o))
        H.assert_features_equal(g, o)
print("FEATURES OK")
"""


@pytest.mark.parametrize("variant", [
    {"SSRLCV_PRIO": "4"},                                    # bit 2 = the staged sequence: memsets, tables on the side stream, four expansions
    {"SSRLCV_SIFT_SERIAL": "1"},                             # no side streams: both new kernels on the caller's stream
    {"SSRLCV_NO_EARLY_CHAIN": "1"},                          # octave 0's chain on the caller's stream of a fused extract
    {"SSRLCV_PRIO": "4", "SSRLCV_SAMPLING_PIPELINED": "1"},  # the pipelined pieces keep the per-octave expansion kernel
], ids=lambda v: "+".join(k.replace("SSRLCV_", "") + "=" + x for k, x in v.items()))
def test_glue_variants_in_child_processes(variant):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _VARIANT_SCRIPT % {"root": root}], env=H.dev_env(**variant), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "FEATURES OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
