"""tests/mxl_cases.py on the CPU: the split and the concatenation are each other's inverse on bytes and scale bytes, a two-pair
call restated in float64 is mx8_cases' truth of the concatenation, the totals K1 + K2 that mx8_cases' SLACK was not measured at
do not exceed it, and a rank padded with zeros contributes exact zeros."""
import pytest
import torch

import mx8_cases as mc
import mxl_cases as lc

SMALL = [c for c in lc.CASES if (c["M"], c["N"]) == (300, 288) and c["K1"] <= 384] + lc.GROUP_CASES


@pytest.mark.parametrize("c", SMALL, ids=lc.case_id)
def test_split_and_concatenation_are_inverse(c):
    ds = lc.make(c)
    s = lc.split(c, ds)
    G, K2 = c["groups"], c["K2"]
    assert s["a"][0].shape == (c["M"], c["K1"]) and s["a2"][0].shape == (c["M"], G * K2) and s["w2"][0].shape == (c["N"], K2)
    assert s["a2"][1].shape == (c["M"], G * K2 // 32) and s["w2"][1].shape == (c["N"], K2 // 32)
    for g in range(G):
        aq, a_s, wq, w_s = lc.concatenation(c, s, g)
        assert torch.equal(aq.view(torch.uint8)[:, c["K1"]:], ds[g]["aq"].view(torch.uint8)[:, c["K1"]:])
        assert torch.equal(a_s[:, c["K1"] // 32:], ds[g]["a_scales"][:, c["K1"] // 32:])
        assert torch.equal(aq.view(torch.uint8)[:, :c["K1"]], ds[0]["aq"].view(torch.uint8)[:, :c["K1"]])
        assert torch.equal(wq.view(torch.uint8), ds[0]["wq"].view(torch.uint8)) and torch.equal(w_s, ds[0]["w_scales"])
    if G > 1:       # the groups' slices hold different data and different scales
        k2, b2 = K2, K2 // 32
        u8 = s["a2"][0].view(torch.uint8)
        for g in range(1, G):
            assert not torch.equal(u8[:, :k2], u8[:, g * k2:(g + 1) * k2])
            assert not torch.equal(s["a2"][1][:, :b2], s["a2"][1][:, g * b2:(g + 1) * b2])
    if c["family"] == "row_scales":       # the two pairs' scale words of a row differ: a pair reading the other's would show
        assert not torch.equal(s["a"][1][:, :4], s["a2"][1][:, :4]) and not torch.equal(s["w"][1][:, :4], s["w2"][1][:, :4])


@pytest.mark.parametrize("c", SMALL, ids=lc.case_id)
def test_two_pair_restatement_is_the_truth_of_the_concatenation(c):
    """De-quantising the pairs one by one and concatenating is de-quantising the concatenation (equal float64 values), so the
    fp32 restatement of a two-pair call IS mx8_cases.restate on the concatenation; and the sum of the two float64 products is
    that concatenation's product to float64 rounding."""
    ds = lc.make(c)
    s = lc.split(c, ds)
    for g in range(c["groups"]):
        aq, a_s, wq, w_s = lc.concatenation(c, s, g)
        k2, b2 = c["K2"], c["K2"] // 32
        a_parts = torch.cat([mc.dequantize(*s["a"]), mc.dequantize(s["a2"][0][:, g * k2:(g + 1) * k2], s["a2"][1][:, g * b2:(g + 1) * b2])], 1)
        w_parts = torch.cat([mc.dequantize(*s["w"]), mc.dequantize(*s["w2"])], 1)
        d = dict(ds[0], a=mc.dequantize(aq, a_s), w=mc.dequantize(wq, w_s))
        assert torch.equal(a_parts, d["a"]) and torch.equal(w_parts, d["w"])
        for epi in ("none", "gelu"):
            assert torch.equal(mc.restate(dict(d, a=a_parts, w=w_parts), epi).view(torch.int16), mc.restate(d, epi).view(torch.int16))
        acc, mag = mc.product(d)
        acc2, mag2 = lc.two_pair_truth(c, s, g)
        assert bool(((acc2 - acc).abs() <= 2.0 ** -48 * mag).all()) and bool(((mag2 - mag).abs() <= 2.0 ** -48 * mag).all())


def test_slack_covers_the_new_totals():
    """Totals of K that mx8_cases.SLACK_CASES does not hold are measured here; none may exceed what its SLACK rests on."""
    new = [k for k in lc.SLACK_CASES if k not in set(mc.SLACK_CASES)]
    assert {K for _, _, K in new} >= {384, 512, 2176}
    worst = mc.measure_excess(cases=new)
    for epi, m in worst.items():
        print(f"{epi}: measured {m:.3e} ({m / 2.0 ** -24:.2f} x 2^-24), limit {mc.MEASURED_EXCESS_BY_EPI[epi]:.3e}")
        assert m <= mc.MEASURED_EXCESS_BY_EPI[epi], (epi, m)


@pytest.mark.parametrize("r", [16, 128, 144])
def test_zero_padded_rank_blocks_are_exact_zeros(r):
    """down [r, K] and up [N, r] padded to a multiple of 128: the padding quantises to scale byte 0 and element bytes 0,
    de-quantises to exact zeros, and the padded product is the unpadded one."""
    g = torch.Generator().manual_seed(7)
    down, up = torch.randn(r, 256, generator=g).to(mc.BF), torch.randn(96, r, generator=g).to(mc.BF)
    dp, upad = lc.pad_rank(down, up)
    R = dp.shape[0]
    assert R % 128 == 0 and R - r < 128
    dq, dsb = mc.quantize(dp)
    uq, usb = mc.quantize(upad)
    assert bool((dq.view(torch.uint8)[r:] == 0).all()) and bool((dsb[r:] == 0).all())
    assert bool((mc.dequantize(dq, dsb)[r:] == 0).all())
    assert bool((usb[:, (r + 31) // 32:] == 0).all())          # the blocks of `up` wholly inside the padding
    assert bool((uq.view(torch.uint8)[:, r:] == 0).all()) and bool((mc.dequantize(uq, usb)[:, r:] == 0).all())
    # a zero activation block (T's padded columns): x . 0-rows = 0 exactly, and MX(0) is byte 0 / element 0
    x = torch.randn(5, 256, generator=g, dtype=torch.float64)
    t = x @ mc.dequantize(dq, dsb).T
    assert bool((t[:, r:] == 0).all()) and bool((mc.scale_bytes_real(t)[:, (r + 31) // 32:] == 0).all())
