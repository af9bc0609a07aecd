"""The attention OUTPUT of every kernel behind ``ltxmi_attention_fwd_bf16`` -- TEST INFRASTRUCTURE ONLY.

Two instruments, shared by tests/test_attn_output_cases.py (CPU: pins this module) and tests/test_gpu_attention_output.py.

A. Exact witnesses, bit equality.
   ``selector``: keys k_j = b sigma_j, sigma_j in {+-1}^dh, queries q_i = a sigma_pi(i): row i's score with key pi(i) is
   a b sqrt(dh) (57 .. 60 nats), every other key at least 20 nats below, so softmax is one-hot to far below half a bf16 ulp
   and O[b, i, h] == v[b, pi(i), h] bit for bit, whatever reference the kernel takes P against.  It sees pairing of key and
   value rows, the V^T image at every key position, row -> lane -> store, head / batch offsets, strides, the segmented
   store, the redo hand-over.  It cannot see the normaliser or any weight below ~2^-30.
   ``uniform``: q = 0, v small non-zero integers: every key that takes part weighs the same (or an exact power of two with
   a ``ln 2^e`` bias) and O == bf16(sum_j w_j v_j / sum_j w_j), sums exact in fp32.  A zero-filled padding key has exactly a
   real key's score here: it sees the ragged mask, a key counted twice or dropped, the matrix-pipe row sum.  It cannot see
   which key went with which value.

B. A per-row figure against float64: fig = ||O_row - truth_row||_2 / ||mag_row||_2 with mag = sum_j p_j |v_j|, bounded by
   MARGIN x the largest figure of ``restate`` -- the documented arithmetic of the kernel's family in plain torch fp32 with
   the kernels' bf16 roundings -- on the same inputs.  It sees RoPE / scale / rescale errors the witnesses have no scores
   for; it cannot see an error below the bf16 roundings of P (one padding key of weight 1 / Lk at Lk >= 333).

``DEFECTS`` are planted into ``restate`` by the CPU test to prove each instrument rejects what it is there for."""
import math
from collections import namedtuple

import torch

import attn_bias_cases as bias_cases

BF = torch.bfloat16
LOG2E = 1.4426950408889634
MARGIN = 2.0

Case = namedtuple("Case", "kid B H dh Lq Lk bias")

# what each kernel id does to a score (csrc/attention*.hip): fold = q x softmax_scale x log2(e) rounded to bf16 (3: only
# when q is finished on load, where that is q's ONE rounding; 4: always, a second rounding); ref = what P = 2^(s - ref) is
# taken against: the running maximum per 64-key tile ("running"; 4 keeps it on a 1/4-bit grid, rounded up), 0 ("zero"), the
# row's maximum over the first two key tiles ("first128": exact form for two tiles, fixed from then on), all keys ("row").
FAMILY = {0: ("running", False), 1: ("running", False), 2: ("running", False), 3: ("zero", "on_load"),
          4: ("grid", True), 5: ("running", False), 6: ("first128", False), 7: ("row", False)}

# (a, b) of the selector per head_dim; REDO_AMPLITUDE takes every item of ids 3 / 6 out of the steady form's +-100 bits
AMPLITUDE = {64: (2.5, 3.0), 128: (2.0, 2.5)}
REDO_AMPLITUDE = (4.0, 8.0)


def _pairs(kid, B, H, dh, pairs, bias=False):
    return [Case(kid, B, H, dh, lq, lk, bias if isinstance(bias, bool) else bool(i % 2 == bias)) for i, (lq, lk) in enumerate(pairs)]


# Lq x Lk grids per kernel id: every Lq and every Lk of the id's edge list once, not the full product (small Lq goes with
# small Lk: the selector needs Lq >= its stratified key set).  64-key tiles everywhere; query tiles of 128 rows (ids 0 / 1 /
# 4 / 5), 256 rows (2, 3, 6), 128-row iterations over row groups (7); ids 3 and 6 run a ring of four key tiles
CASES = {
    0: _pairs(0, 2, 3, 64, [(1, 1), (31, 64), (33, 129), (128, 63), (129, 65), (200, 333)]),
    1: _pairs(1, 2, 3, 64, [(1, 1), (31, 64), (33, 129), (128, 63), (129, 65), (200, 333)], True),
    2: _pairs(2, 1, 256, 64, [(257, 65), (300, 130), (512, 65)]),
    3: _pairs(3, 2, 48, 64, [(257, 1), (300, 63), (512, 64), (257, 65), (300, 192), (512, 193), (257, 256), (300, 257),
                             (512, 321), (300, 449)]),
    4: _pairs(4, 2, 2, 128, [(1, 1), (33, 64), (129, 65), (257, 200), (257, 1029)]),
    5: _pairs(5, 2, 2, 128, [(1, 1), (33, 64), (129, 65), (257, 200), (257, 1029)], True),
    6: _pairs(6, 1, 64, 128, [(257, 1024), (300, 1025), (512, 1087), (257, 1089), (300, 1100)]),
    # the short-key kernel takes a bias or none: odd grid entries run without
    7: _pairs(7, 2, 3, 64, [(1024, 1), (1025, 63), (1151, 64), (1153, 65), (1300, 128), (1024, 129), (1025, 192),
                            (1151, 193), (1153, 255), (1300, 256)], 0),
}
ALL_CASES = [c for kid in sorted(CASES) for c in CASES[kid]]


def case_id(c):
    return f"id{c.kid}-B{c.B}H{c.H}d{c.dh}-q{c.Lq}k{c.Lk}" + ("-bias" if c.bias else "")


def kv_strides(c):
    """Token strides (elements) of k and v the case runs with: contiguous, except id 2, which exists only where the
    pipelined kernel's 2 GiB span is exceeded -- k's rows are put (Lk + 256) x stride x 2 >= 2^31 bytes apart."""
    dense = c.H * c.dh
    if c.kid != 2:
        return dense, dense
    ks = -(-(1 << 30) // (c.Lk + 256))
    return (ks + 7) // 8 * 8, dense


def expected_id(B, H, Lq, Lk, dh, has_bias, ks, vs):
    """attn_select (csrc/attention.hip) restated; the CPU test holds it against ltxmi_attention_kernel_id on every case."""
    wg256 = B * H * ((Lq + 255) // 256)
    rows = Lk + 4 * 64
    span_ok = (rows * ks + dh) * 2 < (1 << 31) and (rows * vs + dh) * 2 < (1 << 31)
    if dh == 128:
        if not has_bias and wg256 >= 128 and Lk >= 1024 and span_ok:
            return 6
        return 5 if has_bias else 4
    if Lk <= 256 and Lq >= 1024:
        return 7
    if not has_bias and wg256 >= 192 and span_ok:
        return 3
    if not has_bias and wg256 >= 512:
        return 2
    return 1 if has_bias else 0


def steady_tiles(c):
    """Work items of a pipelined-kernel case (ids 3, 6): 256 query rows each."""
    return c.B * c.H * ((c.Lq + 255) // 256)


# ------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def stratified_keys(Lk):
    """The keys a selector with fewer queries than keys must still select: 0, 63, 64, Lk - 1, the first and last key of
    every 64-key tile and every key of the last ragged tile."""
    s = {0, Lk - 1}
    for t0 in range(0, Lk, 64):
        s.update((t0, min(t0 + 63, Lk - 1)))
    if Lk % 64:
        s.update(range(Lk - Lk % 64, Lk))
    return sorted(s)


def selector_pi(Lq, Lk, seed):
    """pi [Lq]: every key when Lq >= Lk (a permutation, repeated), the stratified set plus seeded others otherwise; rows
    Lq - 1 and (Lq - 1) ^ 1 select different keys where there are two keys."""
    g = _gen(seed)
    if Lq >= Lk:
        return torch.randperm(Lk, generator=g).repeat(-(-Lq // Lk))[:Lq]
    must = torch.tensor(stratified_keys(Lk))
    assert must.numel() <= Lq, f"Lq {Lq} cannot cover the {must.numel()} stratified keys of Lk {Lk}"
    for _ in range(16):
        pi = torch.cat([must, torch.randint(0, Lk, (Lq - must.numel(),), generator=g)])[torch.randperm(Lq, generator=g)]
        if ((Lq - 1) ^ 1) >= Lq or pi[Lq - 1] != pi[(Lq - 1) ^ 1]:
            return pi
    raise AssertionError("no selector permutation found")


def selector(c, seed=0, amplitude=None, a_div=1.0):
    """-> q, k, v (bf16, CPU), pi.  a_div: the queries' amplitude divided by it (a caller's softmax_scale multiplied)."""
    a, b = amplitude or AMPLITUDE[c.dh]
    g = _gen(7000 + seed)
    sigma = (torch.randint(0, 2, (c.B, c.Lk, c.H, c.dh), generator=g) * 2 - 1).float()
    pi = selector_pi(c.Lq, c.Lk, 7100 + seed)
    k = (b * sigma).to(BF)
    q = (a / a_div * sigma[:, pi]).to(BF)
    assert torch.equal(q.float(), a / a_div * sigma[:, pi])            # amplitudes exact in bf16
    mag = (128 + torch.randint(0, 128, sigma.shape, generator=g)).float() / 128          # [1, 2), exact in bf16
    v = (mag * (torch.randint(0, 2, sigma.shape, generator=g) * 2 - 1)).to(BF)
    return q, k, v, pi


# seeds of ``uniform`` per case (default 0) for which no quotient -- plain, under every keep pattern, under the power-of-two
# bias -- lies within 2^-18 of a bf16 rounding tie; tests/test_attn_output_cases.py asserts the condition
UNIFORM_SEED = {(6, 257, 1089): 1}


def uniform(c, seed=None):
    """-> q = 0, k (N(0, 1): irrelevant to the scores, present in memory), v in +-{1..4} (bf16, CPU)."""
    seed = UNIFORM_SEED.get((c.kid, c.Lq, c.Lk), 0) if seed is None else seed
    g = _gen(7200 + seed)
    q = torch.zeros(c.B, c.Lq, c.H, c.dh, dtype=BF)
    k = torch.randn(c.B, c.Lk, c.H, c.dh, generator=g).to(BF)
    shape = (c.B, c.Lk, c.dh)
    # signs: per element, except on every eighth channel, which has one sign per (batch, channel): its sums grow with Lk
    # (~2.5 Lk, exact in fp32 up to 4 x 1100).  The zero-mean sums stay below 2^8 at every Lk, so their quotients move by
    # less than a bf16 ulp when ONE key in 1029 is added and would not see it; the one-signed ones do.
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    sign[..., 1::8] = sign[:, :1, 1::8]
    base = (1 + torch.randint(0, 4, shape, generator=g)) * sign
    # head h: the base values rotated by h channels, under a seeded sign -- different memory per head, the same B x dh
    # quotients up to sign (with B x H x dh independent ones, 8192 at 64 heads of 128, no seed keeps every quotient 2^-18
    # away from a tie: a quotient by an odd n >= 1024 is that close whenever its numerator hits one of two residues mod n)
    hs = torch.randint(0, 2, (c.H,), generator=g) * 2 - 1
    v = torch.stack([hs[h] * base.roll(h, -1) for h in range(c.H)], dim=2).to(BF)
    return q, k, v


def keep_patterns(c):
    """(name, keep [B, Lk] bool) for every pattern of attn_bias_cases.patterns_for(Lk); ``head`` with the prefix lengths
    that exist at this key count (its default list needs Lk >= 66)."""
    for name in bias_cases.patterns_for(c.Lk):
        if name == "head":
            ns = sorted({n for n in (64, 64 * max(1, (c.Lk - 2) // 64) + 1, c.Lk - 1) if 64 <= n < c.Lk})
            yield name, bias_cases.head(c.B, c.Lk, ns)
        else:
            yield name, bias_cases.PATTERNS[name](c.B, c.Lk)


def pow2_bias(c, seed=0):
    """fp32 [B, Lk] of ln 2^e, e in {-3 .. 0}, key 0 of every row at e = 0 -> (bias, e)."""
    e = -torch.randint(0, 4, (c.B, c.Lk), generator=_gen(7300 + seed))
    e[:, 0] = 0
    return (e.double() * math.log(2.0)).float(), e


def uniform_truth(v, keep=None, e=None):
    """(bf16 truth [B, 1, H, dh] -- every query row's value --, float64 quotient, divisor [B]): sum_j w_j v_j / sum_j w_j,
    w = 2^e on the kept keys."""
    B, Lk = v.shape[:2]
    w = torch.ones(B, Lk, dtype=torch.float64) if e is None else torch.exp2(e.double())
    if keep is not None:
        w = w * keep.double()
    x = torch.einsum("bk,bkhd->bhd", w, v.double()) / w.sum(-1)[:, None, None]
    return x.float().to(BF)[:, None], x, w.sum(-1)


def tie_distance(x):
    """How far (relative) each float64 value is from a bf16 rounding tie; inf for 0 and for values exact in bf16."""
    m, _ = torch.frexp(x.abs())
    t = m * 256.0                                                       # 8 significant bits: [128, 256)
    frac = t - t.floor()
    d = (frac - 0.5).abs() / t
    return torch.where((x == 0) | (frac == 0), torch.full_like(d, math.inf), d)


def uniform_is_decidable(x, denom):
    """The uniform witness's condition: no quotient within 2^-18 (relative) of a bf16 rounding tie.  A quotient EXACTLY on a
    tie is allowed where the divisor ``denom`` [B] is a power of two: numerator, reciprocal and product are then exact in
    fp32, and round-to-nearest-even decides the tie the same way everywhere."""
    d = tie_distance(x)
    m, _ = torch.frexp(denom.double())
    exact_ok = (m == 0.5).view(-1, *([1] * (x.dim() - 1))) & (d == 0)
    return bool((d[~exact_ok] > 2.0 ** -18).all())


FAMILIES = ("plain", "offset", "peaked", "late_max")


def family_inputs(c, family, seed=0):
    """Instrument B's inputs (bf16, CPU).  late_max: the "late" and "redo" spike rows of
    test_attention_pipelined_kernel_steady_form_and_redo (a maximum arriving in the last key tile; scores hundreds of nats
    above the rest: ids 3 and 6 redo that work item), where the case has the rows and keys for them."""
    g = _gen(7400 + seed)
    q = torch.randn(c.B, c.Lq, c.H, c.dh, generator=g).to(BF)
    k = torch.randn(c.B, c.Lk, c.H, c.dh, generator=g).to(BF)
    v = torch.randn(c.B, c.Lk, c.H, c.dh, generator=g)
    if family == "offset":
        v = v + 100.0
    if family == "peaked":
        q, k = (q.float() * 2.5).to(BF), (k.float() * 2.5).to(BF)
    if family == "late_max":
        r5, r40, r100 = min(5, c.Lq - 1), min(40, c.Lq - 1), min(100, c.Lq - 1)
        k[:, max(c.Lk - 30, 0)] = q[:, r5] * 2.0
        k[:, c.Lk // 2] = q[:, r40] * 1.5
        if c.Lk > 70:
            # ~ +320 nats for row 100, three quarters down the keys (past the 128 keys id 6 takes its fixed reference from)
            k[:, (3 * c.Lk) // 4] = q[:, r100] * (40.0 if c.dh == 64 else 30.0)
    return q, k, v.to(BF)


def soft_bias(c, seed=0):
    """A finite fp32 [B, Lk] key bias with a removed tail on batch row 0 (more than one key)."""
    bias = torch.randn(c.B, c.Lk, generator=_gen(7500 + seed))
    if c.Lk > 2:
        bias[0, c.Lk - c.Lk // 3:] = -math.inf
    return bias


def q_on_load_inputs(q_want, kind, seed=0, per_sample=False):
    """Raw q, weight and RoPE tables whose finished q is ``q_want`` [B, Lq, H, dh] up to its one rounding -- for the
    selector.  kind "cos": weight 1, cos = +-1, sin = 0 (raw = q_want x cos x norm); kind "sin": cos = 0, sin = +-1: the
    rotation is the pair swap with its sign, out[2i] = -x[2i+1] sin, out[2i+1] = x[2i] sin.  The raw rows are scaled by a
    seeded power of two per row, which the RMS factor takes out again (|q_want| is constant, so rstd is exact up to eps and
    fp32 rounding: the CPU test checks the finished q).  -> raw bf16 [B*Lq, D], weight bf16 [D], cos, sin bf16 [rows, D],
    period."""
    B, Lq, H, dh = q_want.shape
    D = H * dh
    g = _gen(7600 + seed)
    rows = B * Lq if per_sample else Lq
    sgn = (torch.randint(0, 2, (rows, D // 2), generator=g) * 2 - 1).float().repeat_interleave(2, -1)
    tab = sgn.view(-1, Lq, D).expand(B, Lq, D)
    want = q_want.float().reshape(B, Lq, D)
    amp = float(want.abs().max())
    assert bool((want.abs() == amp).all())
    unit = want / amp                                                   # +-1: RMS 1
    if kind == "cos":
        raw, cos, sin = unit * tab, sgn, torch.zeros_like(sgn)
    else:
        # out[2i] = -x[2i+1] s, out[2i+1] = x[2i] s  =>  x[2i] = out[2i+1] s, x[2i+1] = -out[2i] s   (s = +-1)
        ev, od = unit[..., 0::2], unit[..., 1::2]
        s = tab[..., 0::2]
        raw = torch.stack((od * s, -ev * s), dim=-1).reshape(B, Lq, D)
        cos, sin = torch.zeros_like(sgn), sgn
    row_scale = torch.exp2(torch.randint(-2, 3, (B, Lq, 1), generator=g).float())
    raw = (raw * row_scale).reshape(B * Lq, D).to(BF)
    weight = torch.full((D,), amp, dtype=BF)
    return raw, weight, cos.to(BF), sin.to(BF), rows


def random_q_on_load(c, seed=0, per_sample=False):
    """Instrument B's q-on-load inputs: raw q 1.7 N(0, 1), weight 1 + 0.1 N, random angles."""
    D = c.H * c.dh
    g = _gen(7700 + seed)
    raw = (torch.randn(c.B * c.Lq, D, generator=g) * 1.7).to(BF)
    weight = (1.0 + 0.1 * torch.randn(D, generator=g)).to(BF)
    rows = c.B * c.Lq if per_sample else c.Lq
    ang = torch.rand(rows, D // 2, generator=g) * 6.28
    return raw, weight, ang.cos().repeat_interleave(2, -1).to(BF), ang.sin().repeat_interleave(2, -1).to(BF), rows


def partial_sums(raw):
    """The projection GEMM's per-64-column partial sums of squares, fp32 [rows, D / 64]."""
    return raw.float().reshape(raw.shape[0], -1, 64).pow(2).sum(-1).contiguous()


def finish_q(raw, weight, eps, cos, sin, B, Lq, H, dh, dtype=torch.float64, rope_flip=None):
    """q as the model defines it (oracle/dit.py: RMSNorm over all H dh channels, x weight, then apply_rotary_emb's
    ``x cos + rot sin`` with rot = (-x_odd, x_even) interleaved), written out in ``dtype`` -- not through ops.rmsnorm_rope_.
    rope_flip = (head, pair): planted defect, the sign of sin on that one channel pair."""
    D = H * dh
    x = raw.to(dtype)
    x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * weight.to(dtype)
    if cos is not None:
        c_, s_ = cos.to(dtype), sin.to(dtype)
        if rope_flip is not None:
            s_ = s_.clone()
            ch = rope_flip[0] * dh + 2 * rope_flip[1]
            s_[:, ch:ch + 2] = -s_[:, ch:ch + 2]
        x = x.view(B, Lq, D)
        c_, s_ = c_.view(-1, Lq, D), s_.view(-1, Lq, D)
        t1, t2 = x[..., 0::2], x[..., 1::2]
        rot = torch.stack((-t2, t1), dim=-1).reshape(x.shape)
        x = x * c_ + rot * s_
    return x.reshape(B, Lq, H, dh)


# ------------------------------------------------------------------ truth and figure
def truth(q, k, v, bias=None, scale=None, device=None):
    """float64 softmax attention over the same inputs, per head on ``device`` -> (O [B, Lq, H, dh], mag = sum_j p_j |v_j|),
    float64 on that device.  bias fp32 / float64 [B, Lk]; keys at or below -1e30 are removed."""
    B, Lq, H, dh = q.shape
    scale = 1.0 / math.sqrt(dh) if scale is None else scale
    device = q.device if device is None else device
    out = torch.empty(B, Lq, H, dh, dtype=torch.float64, device=device)
    mag = torch.empty_like(out)
    for b in range(B):
        kb = None
        if bias is not None:
            kb = bias[b].to(device).double()
            kb = kb.masked_fill(kb <= -1e30, -math.inf)
        for h in range(H):
            s = (q[b, :, h].to(device).double() @ k[b, :, h].to(device).double().T) * scale
            if kb is not None:
                s = s + kb
            p = s.softmax(-1)
            vv = v[b, :, h].to(device).double()
            out[b, :, h] = p @ vv
            mag[b, :, h] = p @ vv.abs()
    return out, mag


def figure(o, truth_o, mag):
    """fig[b, i, h] = ||O_row - truth_row||_2 / ||mag_row||_2 (float64)."""
    d = o.to(truth_o.device).double() - truth_o
    return d.norm(dim=-1) / mag.norm(dim=-1)


# ------------------------------------------------------------------ restatement
DEFECTS = ("drop_last_key", "extra_zero_key", "last_key_twice", "swap_v_rows", "swap_out_rows", "rope_sign", "bias_shift",
           "rowsum_scale", "scale_2pct")


def _bf(x):
    return x.to(BF).float()


def restate(kid, q, k, v, bias=None, scale=None, on_load=None, force_exact=False, defect=None):
    """The documented arithmetic of kernel ``kid`` in plain torch fp32 with bf16 roundings where the kernel has them:
    ONE rounding of the finished / folded q (two for id 4's fold of an on-load q), P rounded to bf16 against the family's
    reference, an fp32 row sum of the rounded P, ONE rounding of O.  Left out: the hardware exp2 (~2^-22), the order of the
    sums, the fp32 rounding of the rescales.  on_load = (raw [B*Lq, D], weight, eps, cos, sin): q finished here in fp32.
    Runs on the inputs' device.  -> O bf16 [B, Lq, H, dh]."""
    ref, fold = FAMILY[kid]
    if force_exact and ref in ("zero", "first128"):
        ref = "running"
    if on_load is not None:
        raw, weight, eps, cos, sin = on_load
        B, H, dh = k.shape[0], k.shape[2], k.shape[3]
        Lq = raw.shape[0] // B
        q32 = finish_q(raw, weight, eps, cos, sin, B, Lq, H, dh, dtype=torch.float32,
                       rope_flip=(H - 1, 3) if defect == "rope_sign" else None)
    else:
        q32 = q.float()
    B, Lq, H, dh = q32.shape
    scale = 1.0 / math.sqrt(dh) if scale is None else scale
    if defect == "scale_2pct":
        scale = scale * 1.02
    c = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))    # the kernels' fp32 product
    fold = fold is True or (fold == "on_load" and on_load is not None)
    if fold:
        q32 = _bf(_bf(q32) * c) if (kid == 4 and on_load is not None) else _bf(q32 * c)
    else:
        q32 = _bf(q32)
    k32, v32 = k.float(), v.float()
    kb = None if bias is None else bias.float().clone()
    if defect == "bias_shift" and kb is not None:
        kb = torch.roll(kb, 1, dims=1)
    if defect == "drop_last_key":
        k32, v32, kb = k32[:, :-1], v32[:, :-1], None if kb is None else kb[:, :-1]
    if defect == "extra_zero_key":                                      # a padding key that takes part: k = 0 (score 0), v = 0
        k32, v32 = torch.cat([k32, torch.zeros_like(k32[:, :1])], 1), torch.cat([v32, torch.zeros_like(v32[:, :1])], 1)
        kb = None if kb is None else torch.cat([kb, torch.zeros_like(kb[:, :1])], 1)
    if defect == "last_key_twice":
        k32, v32 = torch.cat([k32, k32[:, -1:]], 1), torch.cat([v32, v32[:, -1:]], 1)
        kb = None if kb is None else torch.cat([kb, kb[:, -1:]], 1)
    if defect == "swap_v_rows":
        j0 = 64 * ((v32.shape[1] - 2) // 64)                            # the first two keys of the last tile that has two
        v32 = v32.clone()
        v32[:, [j0, j0 + 1]] = v32[:, [j0 + 1, j0]]
    Lk = k32.shape[1]
    s = torch.einsum("bqhd,bkhd->bhqk", q32, k32)                       # bits if folded, raw otherwise
    s = s if fold else s * c
    if kb is not None:
        kb2 = (kb.to(q32.device) * float(torch.tensor(LOG2E, dtype=torch.float32))).clamp_min(-1e30)
        s = s + kb2.masked_fill(kb2 <= -1e30, -math.inf)[:, None, None, :]
    dev = q32.device
    acc = torch.zeros(B, H, Lq, dh, device=dev)
    l = torch.zeros(B, H, Lq, 1, device=dev)
    if ref in ("zero", "row"):
        m = torch.zeros(B, H, Lq, 1, device=dev) if ref == "zero" else s.max(-1, keepdim=True).values
        p = _bf(torch.exp2(s - m))
        l = p.sum(-1, keepdim=True)
        acc = torch.einsum("bhqk,bkhd->bhqd", p, v32)
    else:
        m = torch.full((B, H, Lq, 1), -math.inf, device=dev)
        for t, k0 in enumerate(range(0, Lk, 64)):
            st = s[..., k0:k0 + 64]
            mt = st.max(-1, keepdim=True).values
            if ref == "first128" and t >= 2:
                m_new = m
            elif ref == "grid":
                # kept on a 1/4-bit grid, rounded up; moves only when a score of the tile exceeds it
                base = torch.where(torch.isinf(m), torch.zeros_like(m), m)
                moved = (mt > base) | torch.isinf(m)
                m_new = torch.where(moved, base + torch.ceil((mt - base) * 4.0) * 0.25, base)
            else:
                m_new = torch.maximum(m, mt)
            alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - m_new))
            # (a tile whose keys are all removed while the row has seen none yet: the kernels clamp, P = 0)
            p = _bf(torch.exp2(st - torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)))
            l = l * alpha + p.sum(-1, keepdim=True)
            acc = acc * alpha + torch.einsum("bhqk,bkhd->bhqd", p, v32[:, k0:k0 + 64])
            m = m_new
    if defect == "rowsum_scale":
        l = l * (1.0 + 2.0 ** -6)
    o = (acc * (1.0 / l)).permute(0, 2, 1, 3).to(BF)
    if ref in ("zero", "first128"):
        # the steady form's range check (attn_out_of_range): a row sum or accumulator at or above 2^100 (or not finite), or a
        # row sum below 2^-100, sends the row's whole 256-row work item through the exact form again
        out = (~torch.isfinite(l)) | (l >= 2.0 ** 100) | (l < 2.0 ** -100) | ~(acc.abs() < 2.0 ** 100).all(-1, keepdim=True)
        tiles = out[..., 0].unflatten(-1, (-1, 256)) if Lq % 256 == 0 else \
            torch.nn.functional.pad(out[..., 0], (0, -Lq % 256)).unflatten(-1, (-1, 256))
        redo = tiles.any(-1, keepdim=True).expand_as(tiles).flatten(-2)[..., :Lq]           # [B, H, Lq]
        if bool(redo.any()):
            exact = restate(kid, q, k, v, bias, scale, on_load, True, defect)
            o = torch.where(redo.permute(0, 2, 1)[..., None], exact, o)
    if defect == "swap_out_rows":
        i = Lq - 1
        o = o.clone()
        o[:, [i, i ^ 1]] = o[:, [i ^ 1, i]]
    return o.contiguous()


def defect_applies(defect, c):
    if defect in ("drop_last_key", "swap_v_rows"):
        return c.Lk >= 2
    if defect == "swap_out_rows":
        return c.Lq >= 2 and ((c.Lq - 1) ^ 1) < c.Lq and c.Lk >= 2
    if defect == "bias_shift":
        return c.bias and c.Lk >= 2
    return True


# The restatement's largest row figure per (kernel id, family), measured on the CPU over CASES with seed 0 and pinned by
# tests/test_attn_output_cases.py (re-measured there; a change of the restatement or of the inputs shows as a change here).
# The GPU bound is NOT taken from this table: it is MARGIN x the restatement's maximum on each case's own inputs.
MEASURED_RESTATEMENT_MAX = {
    (0, "plain"): 0.000465, (0, "offset"): 0.00148, (0, "peaked"): 0.00227, (0, "late_max"): 0.00244,
    (1, "plain"): 0.000833, (1, "offset"): 0.00167, (1, "peaked"): 0.00232, (1, "late_max"): 0.00246,
    (2, "plain"): 0.00111, (2, "offset"): 0.00176, (2, "peaked"): 0.00247, (2, "late_max"): 0.00247,
    (3, "plain"): 0.000731, (3, "offset"): 0.00146, (3, "peaked"): 0.00283, (3, "late_max"): 0.00244,
    (4, "plain"): 0.000361, (4, "offset"): 0.000903, (4, "peaked"): 0.0123, (4, "late_max"): 0.0384,
    (5, "plain"): 0.000665, (5, "offset"): 0.00162, (5, "peaked"): 0.0024, (5, "late_max"): 0.00248,
    (6, "plain"): 0.000322, (6, "offset"): 0.000976, (6, "peaked"): 0.00235, (6, "late_max"): 0.00255,
    (7, "plain"): 0.000693, (7, "offset"): 0.00171, (7, "peaked"): 0.00259, (7, "late_max"): 0.00277,
}


def shrunk(c, heads=2):
    """The case with at most ``heads`` heads: what the CPU runs (the arithmetic of a row does not depend on the head count;
    the kernel id is given to ``restate``, not selected)."""
    return c._replace(H=min(c.H, heads))


def pin_cases(kid):
    """The cases MEASURED_RESTATEMENT_MAX is measured on: the first and the last of the id's grid, two heads."""
    return [shrunk(CASES[kid][0]), shrunk(CASES[kid][-1])]


def restatement_figures(c, family, seed=0):
    """Row figures of the restatement on one case's family inputs (CPU) -> float64 [B, Lq, H]."""
    q, k, v = family_inputs(c, family, seed)
    bias = soft_bias(c, seed) if c.bias else None
    t, mag = truth(q, k, v, bias)
    return figure(restate(c.kid, q, k, v, bias), t, mag)


def measure_restatement():
    """{(kernel id, family): the restatement's largest row figure over pin_cases}; what MEASURED_RESTATEMENT_MAX records."""
    return {(kid, fam): max(float(restatement_figures(c, fam).max()) for c in pin_cases(kid))
            for kid in sorted(CASES) for fam in FAMILIES}
