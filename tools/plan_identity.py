#!/usr/bin/env python3
"""Planning identity of two builds of libltxmi.so (CPU only: the queries are pure host arithmetic, no device is touched).

    python tools/plan_identity.py PARENT.so BRANCH.so [--conv 18000] [--gemm 4000] [--seed 0]

One seeded list of argument sets, valid and invalid (misaligned pointers, bad algo, refused shapes, NULLs), goes through
ltxmi_conv3d_route / ltxmi_conv3d_workspace_bytes / ltxmi_conv3d_fuses_post_norm and ltxmi_gemm_kernel_id of both
libraries; every returned value, status and error text must be equal.  Pointers are made-up addresses: nothing reads them.
Exit status 0 when all are equal.  Needs the ltxmi package importable (its ctypes struct definitions; it loads the default build)."""
import argparse
import ctypes
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ltx-video-gpupoor_amd"))
from ltxmi import _lib  # noqa: E402   (the struct definitions)

Gemm, Conv, Info = _lib.GemmArgs, _lib.Conv3dArgs, _lib.Conv3dRouteInfo


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.ltxmi_last_error.restype = ctypes.c_char_p
    lib.ltxmi_conv3d_route.restype = ctypes.c_int
    lib.ltxmi_conv3d_route.argtypes = [ctypes.POINTER(Conv), ctypes.POINTER(Info)]
    lib.ltxmi_conv3d_workspace_bytes.restype = ctypes.c_int64
    lib.ltxmi_conv3d_workspace_bytes.argtypes = [ctypes.POINTER(Conv)]
    lib.ltxmi_conv3d_fuses_post_norm.restype = ctypes.c_int
    lib.ltxmi_conv3d_fuses_post_norm.argtypes = [ctypes.POINTER(Conv)]
    lib.ltxmi_gemm_kernel_id.restype = ctypes.c_int
    lib.ltxmi_gemm_kernel_id.argtypes = [ctypes.POINTER(Gemm)]
    return lib


def ptr(r, p_null=0.0, p_odd=0.03):
    if r.random() < p_null:
        return None
    a = r.randrange(1, 1 << 20) * 256
    if r.random() < p_odd:
        a += r.choice([2, 4, 8, 6])
    return a


def conv_set(r):
    a = Conv()
    a.x, a.w, a.y = ptr(r, p_null=0.01), ptr(r, p_null=0.01), ptr(r, p_null=0.01)
    a.bias = ptr(r, p_null=0.05)
    a.B = r.choice([1, 1, 1, 2, 3, 0])
    a.T = r.choice([1, 2, 3, 4, 7, 9, 13, 25, 49, 97, 0])
    a.H = r.choice([1, 4, 7, 8, 16, 17, 32, 48, 64, 128, 129])
    a.W = r.choice([1, 6, 15, 16, 24, 33, 48, 96, 127, 192])
    a.Cin = r.choice([64, 128, 128, 256, 512, 512, 1024, 1024, 2048, 96, 32, 3])
    a.Cout = r.choice([8, 48, 64, 128, 128, 256, 512, 1024, 2048, 4096, 100, 24])
    a.causal, a.pad_replicate = r.randrange(2), r.randrange(2)
    a.d2s = int(r.random() < 0.3)
    if r.random() < 0.4:
        a.residual, a.res_channels = ptr(r), r.choice([128, 256, 512, 1024, 96, 8, 0, 12])
    if r.random() < 0.3:
        a.add = ptr(r)
    a.stride_t, a.stride_hw = r.choice([0, 1, 1, 1, 2, 3]), r.choice([0, 1, 1, 1, 2])
    a.tpad, a.out_T = r.choice([0, 0, 0, 1, 2]), r.choice([0, 0, 0, 0, 5])
    a.kernel_t, a.time_pad_zeros = r.choice([0, 3, 3, 1, 2]), int(r.random() < 0.2)
    a.algo = r.choice([0, 0, 0, 1, 2, 3, 4, 5, -1])
    if r.random() < 0.4:
        a.post_norm = r.choice([1, 1, 1, 2])
        if r.random() < 0.7:
            a.post_scale, a.post_shift = ptr(r), (ptr(r) if r.random() < 0.9 else None)
        a.post_eps = r.choice([1e-6, 1e-8, 0.0, -1.0])
    if r.random() < 0.3:
        a.y_norm = ptr(r)
    if r.random() < 0.6:
        a.workspace = ptr(r, p_odd=0.05)
        a.workspace_bytes = r.choice([1 << 34, 1 << 30, 1 << 24, 4096, 0, -1])
    elif r.random() < 0.1:
        a.workspace_bytes = 4096
    if r.random() < 0.6:          # most sets: what a caller sends -- the interesting differences are between accepted plans
        a.x, a.w, a.y, a.bias = (r.randrange(1, 1 << 20) * 256 for _ in range(4))
        a.B, a.T = r.choice([1, 1, 2]), max(a.T, 1)
        a.Cin = r.choice([64, 128, 256, 512, 1024, 2048])
        a.Cout = r.choice([48, 128, 256, 512, 1024, 2048, 4096])
        a.stride_t, a.stride_hw, a.tpad, a.out_T, a.kernel_t = r.choice([0, 1]), r.choice([0, 1]), 0, 0, r.choice([0, 3])
        a.algo = r.choice([0, 0, 0, 0, 1, 2, 3, 4])
        a.res_channels = r.choice([128, 256, 512, 1024])
        if a.d2s:
            a.add = None
        if a.post_norm:
            a.post_norm, a.post_eps = 1, 1e-6
            a.post_shift = (r.randrange(1, 1 << 20) * 256) if a.post_scale else None
        elif a.y_norm:
            a.y_norm = None
        if a.workspace:
            a.workspace, a.workspace_bytes = r.randrange(1, 1 << 20) * 256, r.choice([1 << 34, 1 << 34, 1 << 24, 0])
        else:
            a.workspace_bytes = 0
    return a


def gemm_set(r):
    a = Gemm()
    a.A, a.W, a.C = ptr(r, p_null=0.01), ptr(r, p_null=0.01), ptr(r, p_null=0.01)
    a.bias = ptr(r, p_null=0.3)
    a.M = r.choice([1, 100, 256, 300, 767, 768, 1024, 4992, 5000, 8192, 14976, 0])
    a.N = r.choice([8, 64, 256, 264, 2048, 4104, 6144, 8192, 100, 32768])
    a.K = r.choice([64, 128, 192, 2048, 8192, 100, 0])
    a.lda = a.K + r.choice([0, 0, 0, 8, 64, 4, -64])
    a.ldw = a.K + r.choice([0, 0, 0, 8, 3])
    a.ldc = a.N + r.choice([0, 0, 0, 4, 8, 2, 1 << 20])
    a.epilogue = r.choice([0, 0, 1, 2, 3, 3, 4, -1])
    if r.random() < 0.6:
        a.residual, a.ldr = ptr(r, p_odd=0.1), a.N + r.choice([0, 0, 4, 8, -8, 1 << 20])
    if r.random() < 0.4:
        a.gate_table = ptr(r)
        a.gate_temb = ptr(r, p_null=0.1)
        a.gate_ld, a.rows_per_group = r.choice([0, 12288, 6, 4]), r.choice([1, 4992, 0, 32])
    a.algo = r.choice([0, 0, 0, 0, 128, 256, 64, 1])
    if r.random() < 0.25:
        a.rowsumsq = ptr(r, p_odd=0.1)
        a.rowsumsq_cols = r.choice([64, 192, 2048, 100, 0, 1 << 20])
        a.rowsumsq_ld = r.choice([1, 3, 32, 96, 1 << 20])
    if r.random() < 0.25:
        a.a_kblock = r.choice([64, 128, 256, 512, 100, -64])
        a.a_kblock_stride = r.choice([64, 4992 * 256, 1 << 30, 1 << 36, 4])
    if r.random() < 0.6:          # most sets: what a caller sends
        a.A, a.W, a.C = (r.randrange(1, 1 << 20) * 256 for _ in range(3))
        a.M, a.K = max(a.M, 1), r.choice([64, 128, 192, 2048, 8192])
        a.N = r.choice([8, 64, 256, 264, 2048, 4104, 6144, 8192])
        a.lda, a.ldw, a.ldc = a.K + r.choice([0, 0, 64]), a.K, a.N + r.choice([0, 0, 4, 8])
        a.epilogue, a.algo = r.choice([0, 0, 1, 2, 3, 3]), r.choice([0, 0, 0, 128, 256])
        if a.epilogue == 3:
            a.residual, a.ldr = r.randrange(1, 1 << 20) * 256 + r.choice([0, 0, 8]), a.N + r.choice([0, 0, 4])
            if a.gate_table:
                a.gate_temb, a.gate_ld, a.rows_per_group = r.randrange(1, 1 << 20) * 256, 12288, r.choice([1, 32, 4992])
        if a.rowsumsq:
            a.epilogue, a.rowsumsq_cols, a.rowsumsq_ld = 0, r.choice([64, 192, 256]), r.choice([4, 32])
        if a.a_kblock:
            a.a_kblock, a.a_kblock_stride = r.choice([64, 128]), r.choice([4992 * 256, 1 << 20])
            a.lda = a.a_kblock
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--conv", type=int, default=18000)
    ap.add_argument("--gemm", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    libs = [load(p) for p in (a.parent, a.branch)]
    r = random.Random(a.seed)
    bad, ok_sets, err_sets, routes = 0, 0, 0, {}

    def err(lib):
        return lib.ltxmi_last_error() or b""

    for i in range(a.conv):
        c = conv_set(r) if i else None                      # the first set: a NULL struct
        res = []
        for lib in libs:
            info = Info()
            rc = lib.ltxmi_conv3d_route(ctypes.byref(c) if c is not None else None, ctypes.byref(info))
            e = err(lib) if rc else b""
            res.append((rc, info.route, info.epilogue, info.ksplit, info.swap_hw, info.finalize_blocks, e,
                        lib.ltxmi_conv3d_workspace_bytes(ctypes.byref(c) if c is not None else None),
                        lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(c) if c is not None else None)))
        if res[0] != res[1]:
            bad += 1
            print("conv set %d differs:\n  %r\n  %r" % (i, res[0], res[1]))
        ok_sets += res[0][0] == 0
        err_sets += res[0][0] != 0
        routes[res[0][1]] = routes.get(res[0][1], 0) + 1
    print("conv3d: %d argument sets (%d accepted: routes %s; %d refused with an error), %d differ" %
          (a.conv, ok_sets, {k: v for k, v in sorted(routes.items()) if k >= 0}, err_sets, bad))
    gbad, ids = 0, {}
    for i in range(a.gemm):
        g = gemm_set(r) if i else None
        res = []
        for lib in libs:
            rc = lib.ltxmi_gemm_kernel_id(ctypes.byref(g) if g is not None else None)
            res.append((rc, err(lib) if rc < 0 else b""))
        if res[0] != res[1]:
            gbad += 1
            print("gemm set %d differs:\n  %r\n  %r" % (i, res[0], res[1]))
        ids[res[0][0]] = ids.get(res[0][0], 0) + 1
    print("gemm: %d argument sets (kernel ids / statuses %s), %d differ" % (a.gemm, dict(sorted(ids.items())), gbad))
    return 1 if bad or gbad else 0


if __name__ == "__main__":
    sys.exit(main())
