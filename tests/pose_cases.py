"""The pose LM terms' cases off the fixture: their scene, their reference and the bound on the sums.  Shared by
tests/test_pose_cases.py (which proves on the CPU oracle alone that the cases test something) and
tests/test_gpu_pose_edges.py (which holds csrc/pose.hip to that reference).  No GPU, no torch.

The reference is built from oracle_pose_match_terms: the float32 residual f[3] and Jacobian J[3][3] of every match.  The
kernel and the oracle spell out the same rounding sequence, so these are the device's own per-match values (the `single`
case holds that bit for bit) and only the order of the sums is the kernel's own.  A sum of float32 terms t_i in ANY order
whose longest chain of additions is d lies within gamma_d * sum |t_i| of the exact sum, gamma_d = d u / (1 - d u),
u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2): the bound is derived from the
launch shape (chain_depth), not measured."""
import numpy as np

import helpers as H
from pointcloud_cases import same, wave_partials  # noqa: F401  (same: bits, or NaN on both sides)

U = 2.0 ** -24
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))     # k_pose_terms' jtj[0..5]: (i, j) of the rotation block
NAMES = tuple("JTJ[%d][%d]" % p for p in PAIRS) + ("JTf[0]", "JTf[1]", "JTf[2]", "cost")
PITCH_ENTRIES = (1, 3, 4, 7)                                # the sums the pitch column of J enters
TRUE_POSE = (0.01, -0.02, 0.015, 0.3, 0.02, -0.01)           # target relative to query (tests/test_pose.py)
OFF = (0.004, -0.006, 0.003)                                 # "off pose": residuals and JTf far from noise
ASYM_SIZES = (2, 63, 64, 65, 255, 256, 257, 2000, 13534)     # a wave, a block, a block and one, many blocks
STRIDE_N = 262144 + 65599                                    # second pass of the grid-stride loop: 256 blocks and 63 lanes
SINGLE_N = 64
NONFINITE_AT, NONFINITE_N = 37, 100


# ---- launch shape -> bound ------------------------------------------------------------------------------------------------
def pose_blocks(n):
    """csrc/pose.hip pose_blocks"""
    return min(max((n + 255) // 256, 1), 1024)


def chain_depth(n, k):
    """The longest chain of float32 additions a term passes through in k_pose_terms (k = 3: JTJ and JTf add three products
    a match) or in either kernel's cost sum (k = 1).  csrc/pose.hip: pose_blocks() blocks of 256 threads; a thread adds k
    terms for every match of its grid-stride loop (m += gridDim.x * blockDim.x), the wave butterfly adds 6 levels, and every
    wave (4 a block) adds its value atomically in any order.  Whoever changes the launch shape changes this."""
    blocks = pose_blocks(n)
    passes = -(-n // (256 * blocks))
    return k * passes + 6 + 4 * blocks


def gamma(d):
    return d * U / (1.0 - d * U)


def bounds(n, absum):
    """absum[10] -> the bound of each of the 10 sums of n matches"""
    g = np.array([gamma(chain_depth(n, 3))] * 9 + [gamma(chain_depth(n, 1))])
    return g * absum


# ---- scene ---------------------------------------------------------------------------------------------------------------
def sym_cameras():
    cams = np.zeros(2, H.CAMERA)
    cams["foc"], cams["size"] = 0.16, 1024
    cams["dpix"] = 0.16 * np.tan(0.2) / 512
    cams["fov"] = 0.4
    return cams


def asym_cameras():
    cams = np.zeros(2, H.CAMERA)
    cams["foc"] = (0.16, 0.12)
    cams["dpix"] = ((6.0e-5, 6.6e-5), (5.0e-5, 4.6e-5))
    cams["size"] = ((1280, 960), (1000, 1100))
    cams["fov"] = 0.4
    return cams


def _rot(a):
    x, y, z = a
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx], [-sy, cy * sx, cy * cx]])


def scene(n, cams, true_pose, seed, noise=0.3):
    """MATCH[n]: seeded 3-D points at depth 8 to 12 in front of the query camera, projected into both cameras (the target at
    true_pose relative to the query), both projections disturbed by N(0, noise) pixels"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(8, 12, n)], 1)
    tp = np.asarray(true_pose, np.float64)
    local = (pts - tp[3:]) @ _rot(tp[:3])                    # R^T (p - t)
    m = np.zeros(n, H.MATCH)
    m["kp1_parent"] = 1
    for key, p, c in (("kp0_loc", pts, cams[0]), ("kp1_loc", local, cams[1])):
        scale = float(c["foc"]) / c["dpix"].astype(np.float64)
        centre = c["size"].astype(np.float64) / 2
        m[key] = p[:, :2] / p[:, 2:3] * scale + centre + rng.normal(0.0, noise, (n, 2))
    return m


def _off(true_pose):
    p = np.array(true_pose, np.float64)
    p[:3] += OFF
    return p.astype(np.float32)


_CACHE = {}


def case(name):
    """-> dict(matches, pose (float32[6], where the terms are evaluated), cams); computed once, never modified"""
    if name not in _CACHE:
        _CACHE[name] = _make(name)
    return _CACHE[name]


def _make(name):
    kind, _, arg = name.partition(":")
    if kind == "single":
        cams = asym_cameras()
        return dict(matches=scene(SINGLE_N, cams, TRUE_POSE, 11), pose=_off(TRUE_POSE), cams=cams)
    if kind == "asym_off":
        cams, n = asym_cameras(), int(arg)
        return dict(matches=scene(n, cams, TRUE_POSE, 100 + n), pose=_off(TRUE_POSE), cams=cams)
    if kind == "sym_true":
        cams = sym_cameras()
        return dict(matches=scene(2000, cams, TRUE_POSE, 21), pose=np.array(TRUE_POSE, np.float32), cams=cams)
    if kind == "big_angles":
        cams, true = asym_cameras(), (-1.2, 0.4, 2.5) + TRUE_POSE[3:]
        pose = np.array(true, np.float64)
        pose[:3] += (0.003, -0.003, 0.003)
        return dict(matches=scene(2000, cams, true, 31), pose=pose.astype(np.float32), cams=cams)
    if kind == "stride":
        cams = asym_cameras()
        return dict(matches=scene(STRIDE_N, cams, TRUE_POSE, 41), pose=_off(TRUE_POSE), cams=cams)
    if kind == "outside":
        cams = asym_cameras()
        m = scene(257, cams, TRUE_POSE, 51).copy()
        # plain numbers to the ray model: shift whole matches (both key points keep seeing one 3-D point only roughly,
        # which is all the terms need) outside the image, below zero and out to 1e6
        m["kp0_loc"][0::4] -= 2000.0
        m["kp1_loc"][1::4] += 3000.0
        m["kp0_loc"][2::16] = (1e6, -1e6)
        m["kp1_loc"][6::16] = (-1e6, 1e6)
        return dict(matches=m, pose=_off(TRUE_POSE), cams=cams)
    if kind == "nonfinite":
        # both key points at the image centres and zero angles: both rays are (0, 0, 1) exactly, the closest-point
        # quotients are 0 / 0
        if arg == "alone":
            cams = sym_cameras()
            m = np.zeros(1, H.MATCH)
            at = 0
        else:
            # an asym-style set: the true angles are -OFF, so that zero angles are off pose by OFF
            cams = asym_cameras()
            true = tuple(-a for a in OFF) + TRUE_POSE[3:]
            m = scene(NONFINITE_N, cams, true, 61).copy()
            at = NONFINITE_AT
        m["kp1_parent"] = 1
        m["kp0_loc"][at] = cams["size"][0] / 2.0
        m["kp1_loc"][at] = cams["size"][1] / 2.0
        return dict(matches=m, pose=np.array((0, 0, 0) + TRUE_POSE[3:], np.float32), cams=cams)
    raise KeyError(name)


FINITE_CASES = (("single",) + tuple("asym_off:%d" % n for n in ASYM_SIZES)
                + ("sym_true", "big_angles", "stride", "outside"))
NONFINITE_CASES = ("nonfinite:alone", "nonfinite:set")
SUM_CASES = FINITE_CASES[1:]                                 # `single` is run one match at a time


def is_asymmetric(name):
    return name != "sym_true"


# ---- reference -----------------------------------------------------------------------------------------------------------
def products(f, J):
    """float32 (n, 3), (n, 3, 3) -> float32 (10, n, 3): the terms of the 10 sums in the kernel's order, J[r][a] J[r][b] for
    the six pairs, J[r][a] f[r], and the per-match cost (f0^2 + f1^2) + f2^2 (as one term: [9, :, 0], the rest +0)"""
    f, J = np.ascontiguousarray(f, np.float32), np.ascontiguousarray(J, np.float32)
    out = np.zeros((10,) + f.shape, np.float32)
    with np.errstate(all="ignore"):
        for k, (a, b) in enumerate(PAIRS):
            out[k] = J[:, :, a] * J[:, :, b]
        for a in range(3):
            out[6 + a] = J[:, :, a] * f
        sq = f * f
        out[9, :, 0] = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    assert out.dtype == np.float32
    return out


def sums(prod):
    """-> (S, absum): float64 sums of the float32 terms and of their absolute values, per entry.  S is `exact` where every
    term is finite, NaN or an infinity otherwise."""
    p = prod.astype(np.float64).reshape(10, -1)
    with np.errstate(invalid="ignore"):
        return p.sum(1), np.abs(p).sum(1)


def one_match_sums(prod):
    """float32 (10, n, 3) -> float32 (n, 10): what a launch over match m alone returns, ((0 + p0) + p1) + p2.  Every other
    addend of the butterfly and the atomic is +0, so no order enters."""
    s = np.zeros((10, prod.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            s = s + prod[:, :, r]
    assert s.dtype == np.float32
    return np.ascontiguousarray(s.T)


def reference(lib, name, cams=None, n=None):
    """-> dict(f, J, prod, S, absum, bound, n) of a case (of its first n matches; with other cameras: the mutants)"""
    key = ("ref", name)
    if cams is None and n is None and key in _CACHE:
        return _CACHE[key]
    c = case(name)
    m = c["matches"] if n is None else c["matches"][:n]
    cm = c["cams"] if cams is None else cams
    with np.errstate(all="ignore"):
        f, J = H.oracle_pose_match_terms(lib, m, c["pose"], cm[0:1], cm[1:2])
    ref = reference_of(f, J)
    if cams is None and n is None:
        _CACHE[key] = ref
    return ref


def reference_of(f, J):
    prod = products(f, J)
    S, absum = sums(prod)
    return dict(f=f, J=J, prod=prod, S=S, absum=absum, bound=bounds(len(f), absum), n=len(f))


def got10(jtj, jtf, cost):
    """capi.pose_lm_terms' (JTJ[6, 6], JTf[6], cost) -> float32[10] in the order of NAMES"""
    return np.array([jtj[j, i] for i, j in PAIRS] + list(jtf[:3]) + [cost], np.float32)


def ratios(got, ref):
    """|got - exact| / bound per entry (0 where both vanish: a sum of zeros has bound 0 and is exactly 0)"""
    miss = np.abs(np.asarray(got, np.float64) - ref["S"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(miss == 0, 0.0, miss / ref["bound"])


def agrees(got, S, bound):
    """one sum the device returned against its reference: NaN for NaN, the same infinity for an infinity, else within bound"""
    got = float(got)
    if np.isnan(S):
        return np.isnan(got)
    if np.isinf(S):
        return got == S
    return bool(np.isfinite(got) and abs(got - S) <= bound)


# ---- the kernel's order of summation in numpy ------------------------------------------------------------------------------
def simulate(prod, seed=0):
    """float32 (10, n, 3) -> float32[10]: k_pose_terms' sums in numpy.  Thread t adds its matches t, t + T, ... (T = 256
    blocks) product by product, a wave's 64 threads go through the wave_sum butterfly, and the waves' values are added
    one by one in a seeded random order, as the atomics may arrive."""
    n = prod.shape[1]
    T = 256 * pose_blocks(n)
    passes = -(-n // T)
    padded = np.zeros((10, passes * T, 3), np.float32)
    padded[:, :n] = prod
    acc = np.zeros((10, T), np.float32)
    for p in range(passes):
        for r in range(3):
            acc = acc + padded[:, p * T:(p + 1) * T, r]
    assert acc.dtype == np.float32
    part = wave_partials(acc)                                # (10, T / 64)
    order = np.random.default_rng(seed).permutation(part.shape[1])
    total = np.zeros(10, np.float32)
    for w in order:
        total = total + part[:, w]
    assert total.dtype == np.float32
    return total
