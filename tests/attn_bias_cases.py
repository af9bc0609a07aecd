"""Key-bias attention cases shared by the CPU and the GPU tests -- TEST INFRASTRUCTURE ONLY.

``ltxmi_attention_fwd_bf16`` takes an additive per-key bias.  Callers write "this key is masked" with many different
values (-10000, the most negative half / bfloat16 / float32, -1e30, -inf); what they all MEAN is that the key is not
there.  ``masked_truth`` states that meaning directly -- softmax attention in float64 over the kept keys only, the
masked ones physically removed -- and so contains no sentinel value at all.  tests/test_attn_bias_cases.py pins that
the reference's eager branch (oracle.dit.sdpa_nhd) means the same for every value of ``MASK_VALUES``; the GPU tests of
tests/test_gpu_attention_bias.py then hold the kernels to it.

The patterns are builders of ``keep`` ([B, Lk] bool, True = the key takes part).  Every builder keeps at least one key
per batch row: a row with every key removed is outside the contract (torch's own SDPA returns NaN for it with -inf)."""
import math

import torch

MASK_VALUES = [-10000.0, -65504.0, -1e30, float(torch.finfo(torch.bfloat16).min), float(torch.finfo(torch.float32).min),
               -math.inf]


def value_id(v):
    return {MASK_VALUES[0]: "m10000", MASK_VALUES[1]: "f16min", MASK_VALUES[2]: "m1e30", MASK_VALUES[3]: "bf16min",
            MASK_VALUES[4]: "f32min", MASK_VALUES[5]: "minf"}[v]


def _checked(keep):
    assert keep.dtype == torch.bool and keep.dim() == 2
    assert bool(keep.any(-1).all()), "a pattern must keep at least one key per batch row"
    return keep


def tail(B, Lk, lens=None):
    """Prompt lengths: row b keeps its first lens[b] keys.  Default: two thirds of the keys, ONE key, ten keys, ..."""
    if lens is None:
        lens = [Lk - Lk // 3, 1, min(10, Lk)]
    keep = torch.zeros(B, Lk, dtype=torch.bool)
    for b in range(B):
        n = lens[b % len(lens)]
        assert 1 <= n <= Lk
        keep[b, :n] = True
    return _checked(keep)


def head(B, Lk, ns=None):
    """A left-padded prompt: row b has its first ns[b] keys off.  Default: the whole first 64-key tile, a multiple of
    64 plus one (whole tiles and the first key of the next), everything but the last key."""
    assert Lk > 64
    if ns is None:
        ns = [64, 64 * max(1, (Lk - 2) // 64) + 1, Lk - 1]
    keep = torch.ones(B, Lk, dtype=torch.bool)
    for b in range(B):
        n = ns[b % len(ns)]
        assert 64 <= n < Lk
        keep[b, :n] = False
    return _checked(keep)


def middle_tile(B, Lk):
    """Keys 64 .. 127 (the second 64-key tile) off in every row."""
    assert Lk > 64
    keep = torch.ones(B, Lk, dtype=torch.bool)
    keep[:, 64:128] = False
    return _checked(keep)


def holes(B, Lk, seed=0):
    """Seeded Bernoulli(0.5) per key, with one (seeded) key per row forced on."""
    g = torch.Generator().manual_seed(1000 + seed)
    keep = torch.rand(B, Lk, generator=g) < 0.5
    on = torch.randint(0, Lk, (B,), generator=g)
    keep[torch.arange(B), on] = True
    return _checked(keep)


def ragged_only(B, Lk):
    """Lk not a multiple of 64: only keys of the last, partial tile are kept (all of them, its last, its first, ...)."""
    assert Lk % 64 != 0 and Lk > 64
    t0 = Lk - Lk % 64
    keep = torch.zeros(B, Lk, dtype=torch.bool)
    for b in range(B):
        if b % 3 == 0:
            keep[b, t0:] = True
        elif b % 3 == 1:
            keep[b, Lk - 1] = True
        else:
            keep[b, t0] = True
    return _checked(keep)


PATTERNS = {"tail": tail, "head": head, "middle_tile": middle_tile, "holes": holes, "ragged_only": ragged_only}


def patterns_for(Lk):
    """Names of the patterns that exist at this key count."""
    names = ["tail", "holes"]
    if Lk > 64:
        names += ["head", "middle_tile"]
        if Lk % 64 != 0:
            names.append("ragged_only")
    return names


def bias_from(keep, value, soft=None):
    """The additive fp32 [B, Lk] bias a caller would write: ``value`` on the masked keys, 0 (or ``soft``) on the kept."""
    bias = torch.zeros(keep.shape, dtype=torch.float32)
    if soft is not None:
        bias = soft.to(torch.float32).clone()
    bias[~keep] = value
    return bias


def masked_truth(q, k, v, keep, soft=None, scale=None):
    """softmax(q k^T scale [+ soft]) v in float64 on the CPU over the KEPT keys only (K / V indexed by keep[b], per batch
    row).  q [B, Lq, H, dh], k / v [B, Lk, H, dh], keep [B, Lk] bool, soft: optional finite [B, Lk] bias -> [B, Lq, H, dh]."""
    B, Lq, H, dh = q.shape
    scale = 1.0 / math.sqrt(dh) if scale is None else scale
    keep = keep.cpu()
    out = torch.empty(B, Lq, H, v.shape[-1], dtype=torch.float64)
    for b in range(B):
        idx = keep[b].nonzero()[:, 0]
        assert idx.numel() > 0
        qq, kk, vv = q[b].cpu().double(), k[b].cpu().double()[idx], v[b].cpu().double()[idx]
        s = torch.einsum("qhd,khd->hqk", qq, kk) * scale
        if soft is not None:
            sb = soft[b].cpu().double()[idx]
            assert bool(torch.isfinite(sb).all())
            s = s + sb
        out[b] = torch.einsum("hqk,khd->qhd", s.softmax(-1), vv)
    return out
