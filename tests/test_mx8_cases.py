"""tests/mx8_cases.py pinned on the CPU: the exponent rule and the element rounding of the restated MX-FP8 quantiser against
values written out by hand, the two readings of the rule (bf16 bits / frexp) against each other, the measured GEMM slack, and
the condition on the cases -- the fp32 restatement alone meets every metric the GPU file applies."""
import pytest
import torch

import gemm_cases as gc
import mx8_cases as mc

BF, F64 = torch.bfloat16, torch.float64


def _block(amax, fill=0.0):
    x = torch.full((1, 32), fill, dtype=F64)
    x[0, 3] = amax
    return x.to(BF)


@pytest.mark.parametrize("amax,e,elem", mc.WITNESSES, ids=lambda v: f"{v:g}")
def test_exponent_rule_witnesses(amax, e, elem):
    x = _block(amax)
    q, s = mc.quantize(x)
    assert int(s[0, 0]) == (0 if amax == 0 else e + 127)
    assert float(q[0, 3].float()) == elem
    # the smallest e with amax * 2^-e <= 448, unless the clamp holds it
    a = float(x[0, 3].to(F64))
    if a > 0 and -127 < e < 127:
        assert a * 2.0 ** -e <= 448 < a * 2.0 ** -(e - 1)
    # -amax gives the same byte and the negated element
    q2, s2 = mc.quantize(-x)
    assert int(s2[0, 0]) == int(s[0, 0]) and float(q2[0, 3].float()) == -elem


def test_rule_names_the_issue_spells_out():
    w = {a: (e, q) for a, e, q in mc.WITNESSES}
    assert w[448.0] == (0, 448.0) and w[450.0] == (1, 224.0) and w[1.0] == (-8, 256.0) and w[0.0][1] == 0.0
    assert w[3e38][0] == 120 and w[2.0 ** -130][0] == -127            # 3e38 and a bf16 subnormal


def test_no_block_saturates_and_the_two_readings_agree():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(64, 256, generator=g) * 10.0 ** (torch.rand(64, 1, generator=g) * 70 - 35)).to(BF)
    x[5] = 0
    x[6, :32] = torch.tensor(2.0 ** -131).to(BF)
    q, s = mc.quantize(x)
    assert torch.equal(s, mc.scale_bytes_real(x))
    qa = q.float().abs().reshape(64, 8, 32).amax(dim=-1)
    assert float(qa.max()) <= 448 and bool(((qa >= 224) | (s == 0)).all())       # the block's amax lands in [224, 448] (byte 0: clamped)
    assert bool((s[5] == 0).all()) and bool((q[5].view(torch.uint8) == 0).all())
    # de-quantised, a block is within half an e4m3 ulp of its amax of the input
    err = (mc.dequantize(q, s) - x.to(F64)).abs().reshape(64, 8, 32)
    amax = x.to(F64).abs().reshape(64, 8, 32).amax(dim=-1, keepdim=True)
    assert bool((err <= amax * 2.0 ** -4 + 2.0 ** -136).all())


def test_element_rounding_ties_and_subnormals():
    """amax 256 -> e = 0, the elements are RNE(x): e4m3 spacing 2^-9 below 2^-6 (subnormals), 2 in [16, 32), 16 in [128, 256)."""
    vals = [2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -9, 2.0 ** -10 * 0.99, 2.0 ** -10 * 1.01, 17.0, 19.0, 21.0, 1.0625, 1.1875,
            240.0, 232.0, 248.0, 0.4375, 2.0 ** -6 - 2.0 ** -10]
    want = [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 0.0, 2.0 ** -9, 16.0, 20.0, 20.0, 1.0, 1.25,
            240.0, 224.0, 256.0, 0.4375, 2.0 ** -6]
    x = torch.zeros(1, 32, dtype=F64)
    x[0, :len(vals)] = torch.tensor(vals, dtype=F64)
    x[0, 31] = 256.0
    for sign in (1.0, -1.0):
        xb = (sign * x).to(BF)
        q, s = mc.quantize(xb)
        assert int(s[0, 0]) == 127
        assert q[0, :len(vals)].float().tolist() == [sign * w for w in want]
    q, _ = mc.quantize((-x).to(BF))
    assert int(q.view(torch.uint8)[0, 0]) == 0x80                     # -2^-10 rounds to -0


def test_witness_rows_carry_their_amax():
    x = mc.witness_rows(64)
    _, s = mc.quantize(x)
    for i, (amax, e, _) in enumerate(mc.WITNESSES):
        assert s[i].tolist() == [0 if amax == 0 else e + 127] * 2, (i, amax)
    assert s[-1].tolist() == [127, 127] and s[-2].tolist() == [127, 127]


def test_probe_is_exact_and_asymmetric():
    for one_hot in ("a", "w"):
        aq, a_s, wq, w_s, want = mc.probe(70, 96, 128, one_hot)
        assert not torch.equal(want[:64, :64], want[:64, :64].T)
        assert len(set(a_s[3].tolist())) == 4 and len(set(w_s[:, 1].tolist())) == 11       # a scale of its own per block and row
        assert float((want.float() != 0).float().mean()) > 0.9


def test_slack_is_measured():
    got = mc.measure_excess()
    print("measured excess:", {k: f"{v:.3e}" for k, v in got.items()})
    for epi, v in got.items():
        assert v <= mc.MEASURED_EXCESS_BY_EPI[epi] * 1.001, (epi, v)
        assert v >= mc.MEASURED_EXCESS_BY_EPI[epi] * 0.5, (epi, v)                          # the pin is the measurement, not a roomy bound
    assert mc.SLACK == 4.0 * max(mc.MEASURED_EXCESS_BY_EPI.values())


@pytest.mark.parametrize("case", mc.SLACK_CASES, ids=lambda c: f"{c[0]}-{c[1]}-K{c[2]}")
def test_restatement_alone_meets_every_metric(case):
    family, epi, K = case
    M, N = mc.SLACK_MN
    d = mc.make(family, M, N, K, epi)
    acc, mag = mc.product(d)
    t, m = mc.epilogue_op(d, epi, acc, mag)
    gc.compare(mc.restate(d, epi), t, m, what=f"restate {family} {epi} K={K}", slack=mc.SLACK)
    if epi in mc.MX_EPIS:
        # the MX-output form: the restated quantiser on the fp32 restatement's values
        v = mc.epilogue_op(d, epi, *mc.product(d, torch.float32))[0]
        s = mc.scale_bytes_real(v)
        f = mc.mx_out_figures(mc.quantize_elements(v, s), s, t, m)
        assert f["scale_bad"] == 0 and f["elem"] <= 1.0, f


def test_case_tables():
    assert {c["shape"] for c in mc.GEMM_CASES} == {mc.SMALL, mc.BIG, (1, 288, 256), (1, 4096, 8192)}
    assert {(c["family"], c["epi"]) for c in mc.GEMM_CASES if c["shape"] in (mc.SMALL, mc.BIG)} == \
        {(f, e) for f in mc.FAMILIES for e in mc.EPIS}
    for c in mc.GEMM_CASES + mc.MXOUT_CASES:
        assert c["shape"][1] % 32 == 0 and c["shape"][2] % 128 == 0
