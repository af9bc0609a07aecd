#!/usr/bin/env python3
"""A/B several builds of libltxmi.so on the hot GEMM shapes inside ONE process (alternating launches on the same tensors,
so clocks / box / data are common to all arms); the first library is the reference of the ratios and of a bit-equality check.
    python tools/ab_gemm.py [--algo {0,128,256}] [--pair2] [--reps N] [--markdown] path/to/libA.so path/to/libB.so [libC.so ...]
--algo sets ltxmi_gemm_args.algo: by shape the big shapes all land on the persistent kernel, so a change in the two tile kernels
shows only with 128 or 256.  --pair2 times ltxmi_gemm_pair2_bf16 instead, with a second pair of K2 = 128 (one group; three
groups of 2048 columns on the 6144-column shapes).  Give the first library twice (a copy of the file) and the second arm's
largest deviation from 1.000 is the noise of the method on that day; the last line of the output collects, per arm, its lowest
ratio, its largest deviation and the shapes whose bits differ from the first arm's."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from ltxmi import _lib  # noqa: E402

K2 = 128


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.ltxmi_gemm_bf16.restype = ctypes.c_int32
    lib.ltxmi_gemm_bf16.argtypes = [ctypes.POINTER(_lib.GemmArgs), ctypes.c_void_p]
    lib.ltxmi_gemm_pair2_bf16.restype = ctypes.c_int32           # every arm has it, whichever entry point is timed
    lib.ltxmi_gemm_pair2_bf16.argtypes = [ctypes.POINTER(_lib.GemmArgs), ctypes.POINTER(_lib.GemmPair), ctypes.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--algo", type=int, choices=(0, 128, 256), default=0)
    ap.add_argument("--pair2", action="store_true")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--reps", type=int, default=7, help="timed windows of 10 launches per arm and shape, after one untimed (median taken)")
    opt = ap.parse_args()
    libs = [load(p) for p in opt.libs]
    names = [os.path.basename(p) for p in opt.libs]
    shapes = [(14976, 8192, 2048, 1, "ff1"), (14976, 2048, 8192, 3, "ff2"), (14976, 6144, 2048, 0, "qkv"),
              (14976, 6144, 2048, 6, "qkv+ss"), (14976, 2048, 2048, 6, "q2+ss"),
              (14976, 2048, 2048, 3, "to_out"), (14976, 2048, 2048, 7, "to_out gated"), (14976, 2048, 8192, 7, "ff2 gated"),
              (4992, 8192, 2048, 1, "ff1 B1"), (8192, 8192, 8192, 0, "8k^3"),
              # small M: the 128x128 tile kernel in the product -- the adaLN table, the text K/V projection, a 768-row one
              (3, 12288, 2048, 0, "adaLN"), (256, 4096, 2048, 0, "text kv"), (768, 2048, 2048, 0, "M768")]
    stream = torch.cuda.current_stream().cuda_stream
    if opt.markdown:
        print("| shape | M x N x K | epi | " + " | ".join(f"{n} ms | x" for n in names) + " |")
        print("|---|---|---|" + "---|---|" * len(names))
    ratios, differs = [[] for _ in libs], [[] for _ in libs]
    for (M, N, K, epi, name) in shapes:
        a = (torch.randn(M, K, device="cuda") * 0.5).to(torch.bfloat16)
        w = (torch.randn(N, K, device="cuda") * K ** -0.5).to(torch.bfloat16)
        b = torch.randn(N, device="cuda").to(torch.bfloat16)
        out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        res = torch.randn(M, N, device="cuda").to(torch.bfloat16)
        g = _lib.GemmArgs()
        g.A, g.lda, g.W, g.ldw, g.bias, g.C, g.ldc = a.data_ptr(), K, w.data_ptr(), K, b.data_ptr(), out.data_ptr(), N
        g.M, g.N, g.K, g.epilogue, g.algo = M, N, K, (0 if epi == 6 else 3 if epi == 7 else epi), opt.algo
        if epi == 6:                                 # plain epilogue + row sums of squares over the first 2048 columns
            ss = torch.empty(M, 32, device="cuda", dtype=torch.float32)
            g.rowsumsq, g.rowsumsq_cols, g.rowsumsq_ld = ss.data_ptr(), 2048, 32
        if epi in (3, 7):
            g.residual, g.ldr = res.data_ptr(), N
        if epi == 7:                                 # x + (table + temb[batch element]) * (A W^T + b): attn1.to_out / ff.net.2 of a block
            g.epilogue = 3
            gtab = torch.randn(N, device="cuda").to(torch.bfloat16)
            gemb = torch.randn(3, 6 * N, device="cuda").to(torch.bfloat16)
            g.gate_table, g.gate_temb, g.gate_ld, g.rows_per_group = gtab.data_ptr(), gemb.data_ptr() + 2 * 2 * N, 6 * N, M // 3
        if opt.pair2:
            groups = 3 if N == 6144 else 1
            a2 = (torch.randn(M, groups * K2, device="cuda") * 0.5).to(torch.bfloat16)
            w2 = (torch.randn(N, K2, device="cuda") * K2 ** -0.5).to(torch.bfloat16)
            pr = _lib.GemmPair()
            pr.A2, pr.lda2, pr.W2, pr.ldw2, pr.K2, pr.group_cols = a2.data_ptr(), groups * K2, w2.data_ptr(), K2, K2, (2048 if groups == 3 else 0)
            run = lambda lib: lib.ltxmi_gemm_pair2_bf16(ctypes.byref(g), ctypes.byref(pr), stream)
        else:
            run = lambda lib: lib.ltxmi_gemm_bf16(ctypes.byref(g), stream)
        times = [[] for _ in libs]
        ref = None
        for rep in range(opt.reps + 1):
            for i, lib in enumerate(libs):
                for _ in range(3):
                    assert run(lib) == 0
                if rep == 0:
                    if ref is None:
                        ref = out.clone()
                    elif not torch.equal(ref, out):
                        differs[i].append(name)
                        print(f"  !! {names[i]} differs from {names[0]}: max {float((ref.float() - out.float()).abs().max()):.4g}")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    run(lib)
                e1.record()
                torch.cuda.synchronize()
                if rep > 0:
                    times[i].append(e0.elapsed_time(e1) / 10)
        med = [sorted(t)[len(t) // 2] for t in times]
        for i, m in enumerate(med):
            ratios[i].append(med[0] / m)
        if opt.markdown:
            print(f"| {name} | {M}x{N}x{K} | {epi} | " + " | ".join(f"{m:.4f} | {med[0] / m:.3f}" for m in med) + " |", flush=True)
        else:
            print(f"{name:7s} {M}x{N}x{K} epi{epi}: " + " | ".join(f"{n} {m:.4f} ms {2.0 * M * N * K / m / 1e9:7.1f} TF x{med[0] / m:.3f}" for n, m in zip(names, med)),
                  flush=True)
    print("\n" + "; ".join(f"arm {i + 1} ({n}): lowest x{min(r):.3f}, largest deviation {max(abs(x - 1.0) for x in r):.3f}, "
                           f"bits differ on {differs[i] or 'no shape'}" for i, (n, r) in enumerate(zip(names, ratios)) if i))


if __name__ == "__main__":
    main()
