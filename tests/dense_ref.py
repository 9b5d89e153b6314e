"""The dense-SIFT reference: items 1-5 of the contract in include/ssrlcv_hip.h ("dense SIFT") taken literally, as a chain of
the per-kernel exports over a numpy-built key-point list.  The exports are independent kernels, pinned to the CPU oracle by
tests/test_gpu_kernel_exports.py on the sparse path's key points; nothing here calls ssrlcv_hip_sift_dense_u8.  The chain
shares sift_sampling.h with dense.hip, so tests/test_gpu_dense.py holds the chain itself, level L included, to the CPU
oracle's dense SIFT (tests/dense_cases.py) at every case it runs: dense parameters leave the range the sparse path reaches."""
import ctypes

import numpy as np
import torch

import helpers as H

u32, f32, csz = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t


def grid(w, h, stride=1, sigma=1.6, ori_width=1.5, desc_width=6.0):
    """-> (margin, nx, ny, wo, wd): the contract's formulas, in the float32 arithmetic the kernels use for their windows."""
    s = np.float32(sigma)
    wo = int(np.ceil(s * np.float32(3.0) * np.float32(ori_width)))
    wd = int(np.ceil(s * np.float32(desc_width)))
    m = max(wo, wd)
    nx = (w - 2 - 2 * m) // stride + 1 if w - 2 - 2 * m >= 0 else 0
    ny = (h - 2 - 2 * m) // stride + 1 if h - 2 - 2 * m >= 0 else 0
    if nx == 0 or ny == 0:
        nx = ny = 0
    return m, nx, ny, wo, wd


def keypoints(w, h, stride=1, sigma=1.6, ori_width=1.5, desc_width=6.0):
    m, nx, ny, _, _ = grid(w, h, stride, sigma, ori_width, desc_width)
    kp = np.zeros(nx * ny, H.SSKEYPOINT)
    ys, xs = np.mgrid[0:ny, 0:nx]
    kp["loc"][:, 0] = (m + xs * stride).reshape(-1)
    kp["loc"][:, 1] = (m + ys * stride).reshape(-1)
    kp["sigma"] = np.float32(sigma)
    kp["theta"] = -1.0
    return kp


class Chain:
    """The composed exports with every buffer allocated up front, so that run() only launches (tools/bench_dense.py times it);
    run() synchronises once, to learn the compacted count the way the reference's host code does."""

    def __init__(self, capi, pixels, stride=1, sigma=1.6, max_orientations=2, thr=0.8, ori_width=1.5, desc_width=6.0):
        self.capi = capi
        img = np.ascontiguousarray(pixels, np.uint8)
        self.h, self.w = img.shape
        self.maxo, self.thr, self.ow, self.dw = max_orientations, thr, ori_width, desc_width
        self.kp = keypoints(self.w, self.h, stride, sigma, ori_width, desc_width)
        self.n = len(self.kp)
        self.pix_d = torch.from_numpy(img).cuda()
        self.kp_d = capi.to_dev(self.kp) if self.n else capi.dev_bytes(32)
        px = self.w * self.h
        self.level = torch.empty(px, dtype=torch.float32, device="cuda")
        self.mm = torch.empty(2, dtype=torch.float32, device="cuda")
        self.grad = capi.dev_bytes(8 * px)
        slots = max(self.n * self.maxo, 1)
        self.thetas = torch.empty(slots, dtype=torch.float32, device="cuda")
        self.nums = torch.empty(slots, dtype=torch.int32, device="cuda")
        self.oriented = capi.dev_bytes(32 * slots)
        self.features = capi.dev_bytes(152 * slots)
        self.features.fill_(0xff)  # parent = -1: fill_descriptors leaves it as it is, like the reference's kernel
        capi.LIB.ssrlcv_hip_compact_workspace_bytes.restype = csz
        self.compact_ws = capi.dev_bytes(int(capi.LIB.ssrlcv_hip_compact_workspace_bytes(u32(slots))))
        self.counts = torch.zeros(2, dtype=torch.int32, device="cuda")

    def run(self):
        """-> count; the records are in self.features"""
        capi, L, w, h, n = self.capi, self.capi.LIB, self.w, self.h, self.n
        st = capi.stream_ptr
        capi.check(L.ssrlcv_hip_u8_to_f32(capi.ptr(self.pix_d), capi.ptr(self.level), csz(w * h), st()))
        capi.check(L.ssrlcv_hip_minmax(capi.ptr(self.level), csz(w * h), capi.ptr(self.mm), st()))
        capi.check(L.ssrlcv_hip_normalize(capi.ptr(self.level), csz(w * h), capi.ptr(self.mm), st()))
        capi.check(L.ssrlcv_hip_pixel_gradients(u32(w), u32(h), capi.ptr(self.level), capi.ptr(self.grad), st()))
        if n == 0:
            return 0
        capi.check(L.ssrlcv_hip_compute_thetas(u32(n), u32(0), u32(w), u32(h), f32(1.0), f32(self.ow), capi.ptr(self.kp_d),
                                               capi.ptr(self.grad), capi.ptr(self.nums), u32(self.maxo), f32(self.thr),
                                               capi.ptr(self.thetas), st()))
        cws, cbytes = capi.ptr(self.compact_ws), csz(self.compact_ws.numel())
        capi.check(L.ssrlcv_hip_compact_thetas(capi.ptr(self.thetas), u32(n * self.maxo), capi.ptr(self.counts[0:1]), cws, cbytes, st()))
        capi.check(L.ssrlcv_hip_compact_addresses(capi.ptr(self.nums), u32(n * self.maxo), capi.ptr(self.counts[1:2]), cws, cbytes, st()))
        nt, nn = self.counts.tolist()  # the one synchronisation: expand_keypoints / fill_descriptors take the count by value
        assert nt == nn, (nt, nn)
        capi.check(L.ssrlcv_hip_expand_keypoints(u32(nn), capi.ptr(self.kp_d), capi.ptr(self.oriented), capi.ptr(self.nums),
                                                 capi.ptr(self.thetas), st()))
        capi.check(L.ssrlcv_hip_fill_descriptors(u32(nn), u32(0), u32(w), u32(h), capi.ptr(self.features), f32(1.0), f32(self.dw),
                                                 capi.ptr(self.oriented), capi.ptr(self.grad), st()))
        return nn


def dense_ref(capi, pixels, **kw):
    """-> (FEATURE records, normalised level L as (h, w) float32)"""
    c = Chain(capi, pixels, **kw)
    n = c.run()
    torch.cuda.synchronize()
    feats = capi.to_host(c.features, H.FEATURE, n)
    return feats, c.level.cpu().numpy().reshape(c.h, c.w).copy()
