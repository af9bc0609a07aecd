"""The truth the key-bias GPU tests use, checked on the CPU against the reference's eager branch.

``attn_bias_cases.masked_truth`` removes the masked keys.  The reference adds a bias and runs a softmax
(oracle.dit.sdpa_nhd restates its eager branch).  For every mask pattern and every value callers use for "masked"
-- -10000, the most negative half / bfloat16 / float32, -1e30, -inf -- the two must agree: the output is finite and
within 1e-5 relative L2 (the tolerance of tests/test_oracle_golden.py; fp32 arithmetic against float64).  With that
pinned, "key removed" IS the reference's meaning of every value in the table and the GPU tests may use it as truth."""
import pytest
import torch

import attn_bias_cases as cases

RTOL = 1e-5
SHAPES = [(2, 2, 70, 200, 64), (3, 1, 33, 130, 128)]          # B, H, Lq, Lk, dh


def _qkv(B, H, Lq, Lk, dh):
    g = torch.Generator().manual_seed(7)
    return [torch.randn(B, L, H, dh, generator=g).to(torch.bfloat16) for L in (Lq, Lk, Lk)]


@pytest.mark.parametrize("value", cases.MASK_VALUES, ids=cases.value_id)
@pytest.mark.parametrize("pattern", list(cases.PATTERNS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_treats_every_mask_value_as_key_removed(shape, pattern, value):
    from oracle import dit
    B, H, Lq, Lk, dh = shape
    assert pattern in cases.patterns_for(Lk)
    q, k, v = _qkv(*shape)
    keep = cases.PATTERNS[pattern](B, Lk)
    bias = cases.bias_from(keep, value)
    out = dit.sdpa_nhd(q.float(), k.float(), v.float(), bias[:, None, None, :]).double()
    assert torch.isfinite(out).all(), "non-finite output from the reference's eager branch"
    truth = cases.masked_truth(q, k, v, keep)
    err = float((out - truth).norm() / truth.norm())
    assert err <= RTOL, f"{pattern} {value}: rel L2 {err:.3e} > {RTOL}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_honours_a_soft_bias_beside_minus_inf(shape):
    """The mixed case of the GPU tests: a finite bias on the kept keys (one row scaled by 30), -inf on the others."""
    from oracle import dit
    B, H, Lq, Lk, dh = shape
    q, k, v = _qkv(*shape)
    keep = cases.holes(B, Lk, seed=1)
    soft = torch.randn(B, Lk, generator=torch.Generator().manual_seed(8))
    soft[0] *= 30.0
    bias = cases.bias_from(keep, -float("inf"), soft)
    out = dit.sdpa_nhd(q.float(), k.float(), v.float(), bias[:, None, None, :]).double()
    assert torch.isfinite(out).all()
    truth = cases.masked_truth(q, k, v, keep, soft=soft)
    err = float((out - truth).norm() / truth.norm())
    assert err <= RTOL, f"rel L2 {err:.3e} > {RTOL}"


def test_builders_keep_a_key_per_row_and_reject_an_empty_row():
    for Lk in (130, 200, 256, 257, 1029):
        for name in cases.patterns_for(Lk):
            keep = cases.PATTERNS[name](3, Lk)
            assert keep.shape == (3, Lk) and bool(keep.any(-1).all()), (name, Lk)
    assert "ragged_only" not in cases.patterns_for(256)
    h = cases.head(3, 256)
    assert [int((~r).sum()) for r in h] == [64, 193, 255] and bool(h[2, 255])
    assert not bool(cases.middle_tile(1, 200)[0, 64:128].any())
    assert int(cases.tail(3, 256).sum(-1)[1]) == 1
    assert not bool(cases.ragged_only(3, 200)[:, :192].any())
    with pytest.raises(AssertionError):
        cases.tail(1, 16, lens=[0])
    with pytest.raises(AssertionError):
        cases._checked(torch.zeros(2, 8, dtype=torch.bool))
