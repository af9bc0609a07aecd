"""Cases, float64 truth, bound and bf16 emulation for ``ltxmi_attention_relbias_bf16`` -- TEST INFRASTRUCTURE ONLY, shared by
tests/test_t5_cpu.py (which pins the bound on the CPU) and tests/test_gpu_t5_kernels.py (which holds the kernel to it).

The bound, per output element e of a query row with float64 softmax weights w_j and result O_e = sum_j w_j v_je:

    |got_e - O_e|  <=  U |O_e|  +  2 (U + S) A_e,        A_e = sum_j w_j |v_je|,   U = 2^-8,   S = 2^-10

  * U |O_e|: the output's rounding to bf16 (8 significant bits, round to nearest: half a unit in the last place <= 2^-8 |x|);
  * 2 U A_e: the P V term.  The kernel multiplies bf16(p_j), relative error <= U each, so the numerator sum_j p_j v_je is off by
    at most U sum_j p_j |v_je| and the denominator sum_j p_j by at most U sum_j p_j; after the division both are <= U A_e
    (|O_e| <= A_e).  The kernel sums the ROUNDED p_j for the denominator, so in practice most of this cancels;
  * 2 S A_e: what is left of fp32 -- the 64-term score sums of bf16 products (logits of magnitude ~1e2..1e3: a few 1e-5
    absolute), the product x log2(e) and its exponent argument (<= 2^-24 x 2000 = 1.2e-4) and exp2 itself; each is a relative
    error of a weight, together well below 2^-10, on numerator and denominator alike.
Nothing in it is taken from the kernel's output."""
import math

import torch

U, S = 2.0 ** -8, 2.0 ** -10
F32_MIN = float(torch.finfo(torch.float32).min)

# name, B, H, Lq, Lk, value written on masked keys (None: no key bias), valid keys per batch row
CASES = [
    ("L1", 1, 1, 1, 1, None, None),
    ("L24_one_valid_key", 2, 3, 24, 24, -math.inf, (24, 1)),
    ("L63_f32min", 1, 3, 63, 63, F32_MIN, (40,)),
    ("L64_m10000", 2, 1, 64, 64, -10000.0, (64, 33)),
    ("L65_minf", 1, 3, 65, 65, -math.inf, (64,)),
    ("L256_f32min", 2, 3, 256, 256, F32_MIN, (200, 256)),
    ("L257_m10000", 1, 1, 257, 257, -10000.0, (130,)),
    ("L512_minf", 1, 3, 512, 512, -math.inf, (511,)),
    ("L512_nomask", 2, 1, 512, 512, None, None),
    ("Lq100_Lk200_minf", 2, 3, 100, 200, -math.inf, (200, 77)),
]


def case_id(c):
    return c[0]


def rel_table(H, Lq, Lk):
    """fp32 [H, Lq + Lk - 1 + 5] and the centre: a value of its own for every (head, offset), of the logits' order of
    magnitude, NOT symmetric in the offset and different per head -- a negated offset, a centre off by one or a head mix-up
    moves whole softmax rows.  The row is longer than needed and the centre sits past Lq - 1: the stride and the centre are
    the caller's."""
    center = Lq - 1 + 3
    d = torch.arange(-center, Lk + 2, dtype=torch.float64)
    h = torch.arange(H, dtype=torch.float64)[:, None]
    tab = 60.0 * torch.sin(0.61 * d[None] + 1.3 * h) + 0.9 * d[None] * (1.0 - 0.5 * h) + 7.0 * h
    return tab.to(torch.float32).contiguous(), center


def make_inputs(case, seed=0):
    """q / k / v as strided slices of ONE packed bf16 [B, Lmax, 3 H 64] buffer (rows past Lq / Lk unused), the key bias and
    the keep mask.  q and k are drawn at 4 sigma: logits of standard deviation 128, reaching several hundred."""
    name, B, H, Lq, Lk, value, valid = case
    g = torch.Generator().manual_seed(1234 + seed + 7 * Lq + Lk)
    Lm = max(Lq, Lk)
    packed = torch.randn(B, Lm, 3, H, 64, generator=g)
    packed[:, :, :2] *= 4.0
    packed = packed.to(torch.bfloat16)
    keep = torch.ones(B, Lk, dtype=torch.bool)
    bias = None
    if value is not None:
        for b in range(B):
            keep[b, valid[b % len(valid)]:] = False
        bias = torch.zeros(B, Lk, dtype=torch.float32)
        bias[~keep] = value
    rel, center = rel_table(H, Lq, Lk)
    return dict(packed=packed, keep=keep, key_bias=bias, rel=rel, center=center, value=value)


def views(packed, Lq, Lk):
    return packed[:, :Lq, 0], packed[:, :Lk, 1], packed[:, :Lk, 2]


def _logits(q, k, rel, center, key_bias, scale, negate_offset, dt):
    B, Lq, H, _ = q.shape
    Lk = k.shape[1]
    s = torch.einsum("bqhd,bkhd->bhqk", q.to(dt), k.to(dt)) * scale
    off = torch.arange(Lk)[None, :] - torch.arange(Lq)[:, None]
    if negate_offset:
        off = -off
    s = s + rel.to(dt)[:, (center + off).clamp(0, rel.shape[1] - 1)][None]
    if key_bias is not None:
        kb = key_bias.to(dt)
        s = s + torch.where(kb <= -1e30, torch.full_like(kb, -math.inf), kb)[:, None, None, :]
    return s


def truth(q, k, v, rel, center, key_bias=None, scale=1.0, negate_offset=False):
    """float64: (O [B, Lq, H, 64], A = sum_j w_j |v_j|).  A key whose bias is at or below -1e30 is not there (-inf); a
    finite bias such as -10000 is simply added."""
    w = _logits(q, k, rel, center, key_bias, scale, negate_offset, torch.float64).softmax(-1)
    vd = v.double()
    return torch.einsum("bhqk,bkhd->bqhd", w, vd), torch.einsum("bhqk,bkhd->bqhd", w, vd.abs())


def bound(o_true, a_true):
    return U * o_true.abs() + 2.0 * (U + S) * a_true


def emulate(q, k, v, rel, center, key_bias=None, scale=1.0):
    """The kernel's arithmetic with torch on the CPU: fp32 scores from the bf16 operands, fp32 bias adds and maximum, p
    rounded to bf16, the row sum over the rounded p, fp32 P V, one division, one rounding."""
    x = _logits(q, k, rel, center, key_bias, scale, False, torch.float32)
    p = torch.exp(x - x.amax(-1, keepdim=True)).to(torch.bfloat16).float()
    o = torch.einsum("bhqk,bkhd->bqhd", p, v.float()) / p.sum(-1).permute(0, 2, 1)[..., None]
    return o.to(torch.bfloat16)


def worst_excess(got, o_true, a_true):
    """max over elements of |got - truth| / bound (<= 1: inside)."""
    return float(((got.double() - o_true).abs() / bound(o_true, a_true).clamp_min(1e-300)).max())
