#!/usr/bin/env python3
"""hipEvent timings for the log-sum-exp output and the merge kernel (profiles/r05_attn_lse.md):
  * ltxmi_attention_merge_bf16 at the config-2 shape (B 3, N 4992, H 32, head_dim 64), n = 2 and 8, as a fraction of the HBM
    roofline for its algorithmic bytes: (n + 1) bf16 outputs + (n + 1) fp32 lse tensors, each moved once;
  * every attention kernel id with the lse output on against off (alternating launches on the same tensors).
    python tools/attn_lse_time.py [HBM GB/s, default 8000 -- the MI355X's peak]
Buffers are rotated so that no launch finds its inputs in the 256 MB last-level cache."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from ltxmi import ops  # noqa: E402

DEV, BF = "cuda", torch.bfloat16


def time_ms(fns, iters, reps=7):
    """Median over reps of the mean time of iters launches, for each of fns in turn (interleaved: common clocks)."""
    times = [[] for _ in fns]
    for rep in range(reps + 1):
        for i, fn in enumerate(fns):
            fn(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for j in range(iters):
                fn(j)
            e1.record()
            torch.cuda.synchronize()
            if rep > 0:
                times[i].append(e0.elapsed_time(e1) / iters)
    return [sorted(t)[len(t) // 2] for t in times], [(min(t), max(t)) for t in times]


def merge_times(peak_gbs):
    B, N, H, dh = 3, 4992, 32, 64
    for n in (2, 8):
        sets = max(2, int(600e6 // ((n + 1) * B * N * H * dh * 2)) + 1)          # > 256 MB of distinct data in rotation
        outs = [[torch.randn(B, N, H, dh, device=DEV).to(BF) for _ in range(n)] for _ in range(sets)]
        lses = [[torch.randn(B, H, N, device=DEV) for _ in range(n)] for _ in range(sets)]
        dst = [torch.empty(B, N, H, dh, device=DEV, dtype=BF) for _ in range(sets)]
        dl = [torch.empty(B, H, N, device=DEV) for _ in range(sets)]
        (med,), ((lo, hi),) = time_ms([lambda j: ops.attention_merge(outs[j % sets], lses[j % sets], out=dst[j % sets], lse=dl[j % sets])], 20)
        nbytes = (n + 1) * (B * N * H * dh * 2 + B * H * N * 4)
        gbs = nbytes / med / 1e6
        print(f"merge n={n}: {med * 1e3:7.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}), {nbytes / 1e6:.1f} MB -> {gbs:6.0f} GB/s = "
              f"{100 * gbs / peak_gbs:4.1f} % of {peak_gbs:.0f} GB/s", flush=True)


def lse_on_off():
    # (B, H, Lq, Lk, dh, bias, k token stride or None = contiguous): one shape per kernel id
    shapes = {0: (1, 191, 256, 512, 64, False, None), 1: (1, 191, 256, 512, 64, True, None),
              2: (1, 512, 256, 512, 64, False, 5000000), 3: (3, 32, 4992, 4992, 64, False, None),
              4: (1, 127, 256, 1024, 128, False, None), 5: (1, 127, 256, 1024, 128, True, None),
              6: (1, 12, 32760, 32760, 128, False, None), 7: (3, 32, 4992, 256, 64, True, None)}
    for kid, (B, H, Lq, Lk, dh, bias, ks) in shapes.items():
        q = torch.randn(B, Lq, H, dh, device=DEV).to(BF)
        v = torch.randn(B, Lk, H, dh, device=DEV).to(BF)
        if ks is None:
            k = torch.randn(B, Lk, H, dh, device=DEV).to(BF)
        else:
            k = torch.as_strided(torch.zeros(B * Lk * ks, dtype=BF, device=DEV), (B, Lk, H, dh), (Lk * ks, ks, dh, 1))
            k.copy_(torch.randn(B, Lk, H, dh, device=DEV))
        kb = torch.randn(B, Lk, device=DEV) if bias else None
        assert ops.attention_kernel_id(B, H, Lq, Lk, dh, bias, k.stride(1), v.stride(1)) == kid
        out = torch.empty(B, Lq, H, dh, device=DEV, dtype=BF)
        lse = torch.empty(B, H, Lq, device=DEV)
        iters = 3 if kid == 6 else 10
        (off, on), spans = time_ms([lambda j: ops.attention(q, k, v, out=out, key_bias=kb),
                                    lambda j: ops.attention(q, k, v, out=out, key_bias=kb, lse=lse)], iters)
        print(f"kernel {kid} B{B} H{H} Lq{Lq} Lk{Lk} dh{dh}: lse off {off * 1e3:9.1f} us (min {spans[0][0] * 1e3:.1f} max {spans[0][1] * 1e3:.1f})  "
              f"on {on * 1e3:9.1f} us (min {spans[1][0] * 1e3:.1f} max {spans[1][1] * 1e3:.1f})  on/off {on / off:.4f}", flush=True)
        del q, k, v, out


if __name__ == "__main__":
    peak = float(sys.argv[1]) if len(sys.argv) > 1 else 8000.0
    merge_times(peak)
    lse_on_off()
