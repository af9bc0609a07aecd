"""Key-bias attention on a real MI355X with the mask values callers really write.

``ltxmi_attention_fwd_bf16`` takes an additive per-key bias; include/ltxmi.h and ``pay_attention`` promise it for
arbitrary additive masks.  Three kernels take a bias: the short-key kernel (id 7, attention_cross.hip) and the
register-staged kernels at head_dim 64 and 128 (ids 1 and 5, attention.hip).  Here each of them meets every mask pattern
of tests/attn_bias_cases.py (padded tail, left padding that masks whole leading key tiles, a masked middle tile, random
holes, only the ragged last tile kept) with every value in use for "masked": -10000, the most negative half / bfloat16 /
float32, -1e30 and -inf.

Truth is ``attn_bias_cases.masked_truth``: float64 softmax attention with the masked keys REMOVED, on the same seeded
bf16 inputs (tests/test_attn_bias_cases.py pins that this is what the reference computes for every value).  Tolerances
are those of tests/test_gpu_kernels.py (``check``, REL_L2, MAXREL): nothing new.  Every case first asserts the kernel id
it means to exercise.  A NaN is a wrong answer here, not a fault: ``check`` reports it as "non-finite output".

What these cases found before the kernels clamped the staged bias (ATTN_BIAS_FLOOR, csrc/attention.h): 70 of the 220
failed, every one with "non-finite output" -- kernel 7 with bfloat16 min, float32 min and -inf under every pattern (the
bias is staged as bf16 hi + lo of bias / scale: -inf - -inf), kernels 1 and 5 with the same three values under ``head``
and ``ragged_only`` (every key seen so far at -inf: running maximum -inf, x - m = -inf + inf)."""
import functools
import math

import pytest
import torch

import attn_bias_cases as cases
from test_gpu_kernels import BF, DEV, MAXREL, REL_L2, attn_truth, check, rnd

pytestmark = pytest.mark.gpu

INF = math.inf
F32MIN = float(torch.finfo(torch.float32).min)
BF16MIN = float(torch.finfo(torch.bfloat16).min)


# ------------------------------------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=4)
def _inputs(B, H, Lq, Lk, dh, packed):
    """Seeded bf16 q / k / v on the host and on the device.  packed: k / v are the strided halves of one
    [B, Lk, 2, H, dh] projection buffer, as the DiT's cross-attention hands them over."""
    q = rnd(B, Lq, H, dh, seed=300)
    if packed:
        kv = rnd(B, Lk, 2, H, dh, seed=301)
        kvd = kv.to(DEV)
        return q, kv[:, :, 0], kv[:, :, 1], q.to(DEV), kvd[:, :, 0], kvd[:, :, 1]
    k, v = rnd(B, Lk, H, dh, seed=301), rnd(B, Lk, H, dh, seed=302)
    return q, k, v, q.to(DEV), k.to(DEV), v.to(DEV)


def _rows(Lq, band=None):
    """Query rows that are compared: all of them up to 2100 rows, else the first and the last band (the last one ragged)."""
    if band is not None:
        return torch.cat([torch.arange(0, band), torch.arange(Lq - band, Lq)])
    if Lq <= 2100:
        return torch.arange(Lq)
    return torch.cat([torch.arange(0, 160), torch.arange(Lq - 140, Lq)])


_TRUTH = {}


def _truth(shape, pattern, keep, band=None):
    """masked_truth of a (shape, pattern) on the compared rows: the same for every mask value, computed once."""
    key = (shape, pattern, band)
    if key not in _TRUTH:
        if len(_TRUTH) >= 8:
            _TRUTH.clear()
        B, H, Lq, Lk, dh, packed = shape
        q, k, v = _inputs(*shape)[:3]
        _TRUTH[key] = cases.masked_truth(q[:, _rows(Lq, band)], k, v, keep)
    return _TRUTH[key]


def _run(kid, shape, pattern, value, band=None, keep=None):
    from ltxmi import ops
    B, H, Lq, Lk, dh, packed = shape
    q, k, v, qd, kd, vd = _inputs(*shape)
    assert ops.attention_kernel_id(B, H, Lq, Lk, dh, True, kd.stride(1), vd.stride(1)) == kid
    if keep is None:
        keep = cases.PATTERNS[pattern](B, Lk)
    bias = cases.bias_from(keep, value)
    out = ops.attention(qd, kd, vd, key_bias=bias.to(DEV))
    what = f"kernel {kid} B{B} H{H} Lq{Lq} Lk{Lk} dh{dh} {pattern} {value}"
    e = check(out[:, _rows(Lq, band).to(DEV)], _truth(shape, pattern, keep, band), what=what)
    print(f"{what}: rel L2 {e:.3e}")
    return out


def _cases(kid, shape):
    B, H, Lq, Lk, dh, packed = shape
    return [pytest.param(kid, shape, p, v, id=f"id{kid}-Lq{Lq}-Lk{Lk}-dh{dh}-{p}-{cases.value_id(v)}")
            for p in cases.patterns_for(Lk) for v in cases.MASK_VALUES]


DIT = (3, 32, 4992, 256, 64, True)                    # the DiT's T5 cross-attention
WAN = (1, 12, 32760, 512, 128, False)                 # the Wan 1.3B text cross-attention


# ------------------------------------------------------------------------------- every pattern x every value
@pytest.mark.parametrize("kid,shape,pattern,value",
                         _cases(7, DIT)
                         + _cases(7, (2, 8, 1500, 200, 64, True)) + _cases(7, (2, 8, 1500, 130, 64, True))    # ragged last key tile
                         + _cases(1, (3, 4, 300, 256, 64, False))      # below the short-key kernel's row threshold
                         + _cases(1, (3, 4, 1023, 256, 64, False))     # the two sides of the dispatch boundary of id 7:
                         + _cases(1, (3, 4, 1024, 257, 64, False))     # one row short, one key over
                         + _cases(5, (3, 4, 300, 256, 128, False)))
def test_attention_masked_keys_are_removed(kid, shape, pattern, value):
    """Every mask pattern x every mask value, per bias-taking kernel, against the float64 truth without the masked keys."""
    _run(kid, shape, pattern, value)


@pytest.mark.parametrize("value", cases.MASK_VALUES, ids=cases.value_id)
def test_attention_whole_leading_tiles_masked_long_keys(value):
    """Kernel 1 on a long, ragged key sequence (17 tiles) with whole multiples of 64 leading keys off: the running maximum
    has seen nothing but masked keys for 8 and for 16 tiles when the first kept key arrives."""
    shape = (2, 4, 640, 1029, 64, False)
    _run(1, shape, "head_512_1024", value, keep=cases.head(2, 1029, ns=[512, 1024]))


@pytest.mark.parametrize("value", cases.MASK_VALUES, ids=cases.value_id)
def test_attention_wan_text_cross_attention_padded_prompt(value):
    """Kernel 5 at the Wan 1.3B text cross-attention shape [1, 32760, 12, 128] x 512 keys with a padded prompt tail: the
    first and the last 64 query rows."""
    _run(5, WAN, "tail", value, band=64)


def test_attention_wan_text_cross_attention_without_bias():
    """The same call without a bias (kernel 4) against the oracle, first and last 64 rows."""
    from ltxmi import ops
    B, H, Lq, Lk, dh, _ = WAN
    q, k, v, qd, kd, vd = _inputs(*WAN)
    assert ops.attention_kernel_id(B, H, Lq, Lk, dh, False, kd.stride(1), vd.stride(1)) == 4
    out = ops.attention(qd, kd, vd)
    rows = _rows(Lq, 64)
    e = check(out[:, rows.to(DEV)], attn_truth(q[:, rows], k, v), what="Wan text cross-attention, no bias")
    print(f"Wan text cross-attention, no bias: rel L2 {e:.3e}")


def test_attention_short_key_kernel_masked_keys_with_q_norm_on_load():
    """Kernel 7 finishing q on load (RMSNorm factor per row x weight) with a left-padded -inf mask: against the float64
    truth on the fp32-normalised q."""
    from ltxmi import ops
    shape = (2, 8, 1500, 200, 64, True)
    B, H, Lq, Lk, dh, _ = shape
    D = H * dh
    _, k, v, _, kd, vd = _inputs(*shape)
    assert ops.attention_kernel_id(B, H, Lq, Lk, dh, True, kd.stride(1), vd.stride(1)) == 7
    qraw = rnd(B * Lq, D, seed=310, scale=1.7)
    wq = (1.0 + 0.1 * rnd(D, seed=311).float()).to(BF)
    ss = qraw.float().reshape(B * Lq, D // 64, 64).pow(2).sum(-1).contiguous()
    rstd = ops.rowsumsq_rstd(ss.to(DEV), D, 1e-6)
    keep = cases.head(B, Lk)
    out = ops.attention(qraw.to(DEV).view(B, Lq, H, dh), kd, vd, key_bias=cases.bias_from(keep, -INF).to(DEV),
                        q_norm=(rstd, wq.to(DEV), 1e-6))
    q32 = qraw.float()
    qn = (q32 * torch.rsqrt(q32.pow(2).mean(-1, keepdim=True) + 1e-6) * wq.float()).view(B, Lq, H, dh)
    check(out, cases.masked_truth(qn, k, v, keep), what="kernel 7, q finished on load, -inf head mask")


# ----------------------------------------------------------------------------------------------- mixed bias
KERNEL_SHAPES = [pytest.param(7, (2, 8, 1500, 200, 64, True), id="id7"), pytest.param(1, (3, 4, 300, 256, 64, False), id="id1"),
                 pytest.param(5, (3, 4, 300, 256, 128, False), id="id5")]


@pytest.mark.parametrize("kid,shape", KERNEL_SHAPES)
def test_attention_soft_bias_beside_minus_inf(kid, shape):
    """A finite soft bias (seeded normal, one row scaled by 30) on the kept keys together with -inf on the masked ones:
    the soft part is still honoured to the usual tolerance."""
    from ltxmi import ops
    B, H, Lq, Lk, dh, _ = shape
    q, k, v, qd, kd, vd = _inputs(*shape)
    assert ops.attention_kernel_id(B, H, Lq, Lk, dh, True, kd.stride(1), vd.stride(1)) == kid
    keep = cases.holes(B, Lk, seed=3)
    soft = torch.randn(B, Lk, generator=torch.Generator().manual_seed(4))
    soft[0] *= 30.0
    out = ops.attention(qd, kd, vd, key_bias=cases.bias_from(keep, -INF, soft).to(DEV))
    e = check(out, cases.masked_truth(q, k, v, keep, soft=soft), what=f"kernel {kid}: soft bias + -inf")
    print(f"kernel {kid}: soft bias + -inf: rel L2 {e:.3e}")


# ------------------------------------------------------------------------------------------ shift invariance
@pytest.mark.parametrize("const", [-10000.0, 500.0])
@pytest.mark.parametrize("kid,shape", KERNEL_SHAPES)
def test_attention_constant_bias_is_no_bias(kid, shape, const):
    """One constant on ALL keys -- the finite "everything discarded" row, which the reference turns into the plain softmax --
    equals the float64 truth without a bias."""
    from ltxmi import ops
    B, H, Lq, Lk, dh, _ = shape
    q, k, v, qd, kd, vd = _inputs(*shape)
    assert ops.attention_kernel_id(B, H, Lq, Lk, dh, True, kd.stride(1), vd.stride(1)) == kid
    out = ops.attention(qd, kd, vd, key_bias=torch.full((B, Lk), const, device=DEV))
    truth = cases.masked_truth(q, k, v, torch.ones(B, Lk, dtype=torch.bool))
    e = check(out, truth, rel_l2=REL_L2, maxrel=MAXREL, what=f"kernel {kid}: constant bias {const}")
    print(f"kernel {kid}: constant bias {const}: rel L2 {e:.3e}")


# -------------------------------------------------------------------------------------- sentinel equivalence
@pytest.mark.parametrize("pattern", ["tail", "head"])
@pytest.mark.parametrize("kid,shape", [pytest.param(7, DIT, id="id7")] + KERNEL_SHAPES[1:])
def test_attention_mask_values_give_identical_bits(kid, shape, pattern):
    """-10000, finfo.min and -inf on the same masked keys give bit-identical outputs (secondary to the float64 truth above).
    Derivation: a masked key's P is exp2(<= -14000) = 0 exactly in fp32 with any of them (the scores of these seeded inputs
    are far above -10000), the kept keys carry bias 0 with any of them, and the row maximum is taken over kept keys or
    wiped by a rescale factor of exactly 0 when the first kept key arrives."""
    outs = {v: _run(kid, shape, pattern, v) for v in (-10000.0, BF16MIN, F32MIN, -INF)}
    for v in (BF16MIN, F32MIN, -INF):
        assert torch.equal(outs[v], outs[-10000.0]), f"kernel {kid} {pattern}: {v} differs from -10000"


# ---------------------------------------------------------------------------------------------- seam, model
@pytest.mark.parametrize("value", [BF16MIN, -INF], ids=cases.value_id)
@pytest.mark.parametrize("kid,shape", KERNEL_SHAPES[:2])
def test_pay_attention_with_dtype_min_and_minus_inf_masks(kid, shape, value):
    """The seam with a bf16 [B, 1, 1, Lk] mask as ``masked_fill`` / ``get_extended_attention_mask`` write it."""
    from ltxmi import ops, pay_attention
    B, H, Lq, Lk, dh, _ = shape
    q, k, v, qd, kd, vd = _inputs(*shape)
    assert ops.attention_kernel_id(B, H, Lq, Lk, dh, True, kd.stride(1), vd.stride(1)) == kid
    for pattern in ("tail", "head"):
        keep = cases.PATTERNS[pattern](B, Lk)
        mask = torch.zeros(B, 1, 1, Lk, dtype=BF).masked_fill(~keep[:, None, None, :], value)
        assert float(mask.float().min()) == value
        out = pay_attention([qd, kd, vd], attention_mask=mask.to(DEV))
        check(out, cases.masked_truth(q, k, v, keep), what=f"pay_attention kernel {kid} {pattern} {value}")


def test_transformer_minus_inf_bias_equals_the_zero_one_mask():
    """Transformer3DModel.forward on the small config of test_gpu_model.py::test_transformer_small: the 2-D 0/1 mask
    (converted to 0 / -10000 inside) and the equivalent 3-D bias with -inf give bit-identical outputs (the derivation of
    test_attention_mask_values_give_identical_bits)."""
    from test_gpu_model import _Holder, build_model, dit_case
    grid, B, T = (3, 5, 7), 3, 40
    cfg, sd32, x, enc, mask, ts, frac = dit_case(2, 64, 2, grid, B, T)
    assert 0 < int(mask.sum()) < mask.numel()
    m = build_model(cfg, sd32)
    fc = m.precompute_freqs_cis(frac.to(DEV))
    bias3 = torch.zeros(B, 1, T, dtype=BF).masked_fill(mask[:, None, :] == 0, -INF)

    def run(em):
        with torch.no_grad():
            return m(x.to(DEV), freqs_cis=fc, encoder_hidden_states=enc.to(DEV), encoder_attention_mask=em.to(DEV),
                     timestep=ts.to(DEV), latent_shape=grid, ltxv_model=_Holder(), return_dict=False)[0]
    a, b = run(mask), run(bias3)
    assert torch.isfinite(b.float()).all(), "non-finite output with the -inf bias"
    assert torch.equal(a, b)
