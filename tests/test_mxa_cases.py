"""tests/mxa_cases.py held on the CPU: its two restatements against tests/mx8_cases.py (``restate``, ``quantize``) and against
tests/norm_cases.py's float64 truth, and the case tables against what the issue of this feature names."""
import pytest
import torch

import mx8_cases as mc
import mxa_cases as xc
import norm_cases as nc


def test_case_tables():
    assert len(xc.RSS_CASES) == 6 * 2 * 2 and {c["shape"] for c in xc.RSS_CASES} == set(xc.RSS_SHAPES)
    for (M, N, K), cols in xc.RSS_SHAPES.items():
        assert K % 128 == 0 and N % 32 == 0 and all(c % 64 == 0 and 0 < c <= N for c in cols)
    # the sums cross a 256-column tile boundary and stop inside a tile; a ragged N tile holds no whole block
    assert 256 < 320 < 512 and 544 % 256 == 32 and 288 % 256 == 32
    assert len(xc.NORM_CASES) == 3 * 4 * 2 * 2
    assert all(D % 32 == 0 and D <= 8192 for D in xc.NORM_D) and [D > 2048 for D in xc.NORM_D] == [False, False, True, True]
    assert 37 % 13 and 300 % 13


@pytest.mark.parametrize("c", xc.RSS_EXACT_CASES, ids=xc.rss_exact_id)
def test_exact_row_sums_are_exact(c):
    """The condition of the exact row sums: integer outputs of magnitude <= 15, sums that fp32 holds; and the shapes reach the
    blocks their comments name."""
    (M, N, K), cols = c["shape"], c["cols"]
    assert K == 128 and N % 32 == 0 and cols % 64 == 0 and 0 < cols <= N
    d = xc.rss_exact(c)
    assert xc.rss_exact_ok(d)
    assert d["sums"].shape == (M, cols // 64) and (d["bias"] is not None) == c["bias"]
    assert float(d["truth"].abs().max()) == (15 if c["bias"] else 7)
    # element by element, by hand
    for m, b in ((0, 0), (M - 1, cols // 64 - 1)):
        assert float(d["sums"][m, b]) == sum(int(v) ** 2 for v in d["truth"][m, 64 * b:64 * b + 64].tolist())
    # no block sums to zero: a block the kernel left at zero cannot pass
    assert float(d["sums"].min()) > 0


def test_exact_row_sum_shapes():
    assert set(xc.RSS_EXACT_SHAPES) == {(300, 2336, 128), (257, 64, 128)} and len(xc.RSS_EXACT_CASES) == 8
    assert xc.RSS_EXACT_SHAPES[(300, 2336, 128)] == (64, 2048, 2304) and xc.RSS_EXACT_SHAPES[(257, 64, 128)] == (64,)
    # 10 N-tiles in bands of 8: 2048 columns are the first band, 2304 end with the ninth tile, the tenth holds 32 columns
    assert -(-2336 // 256) == 10 and 2048 == 8 * 256 and 2304 == 9 * 256 and 2336 - 2304 == 32


@pytest.mark.parametrize("family", xc.RSS_FAMILIES)
def test_row_sum_restatement(family):
    M, N, K = 300, 288, 256
    d = mc.make(family, M, N, K, "none")
    c, ss = xc.gemm_rowsumsq_restate(d, 256)
    # the output is mx8_cases' restatement of the plain GEMM, bit for bit; without the bias it is that of a zero bias
    assert torch.equal(c.view(torch.int16), mc.restate(d, "none").view(torch.int16))
    c0, ss0 = xc.gemm_rowsumsq_restate(d, 64, bias=False)
    assert torch.equal(c0.view(torch.int16), mc.restate(dict(d, bias=torch.zeros_like(d["bias"])), "none").view(torch.int16))
    # the sums, element by element, of what was stored
    for m, b in ((0, 0), (299, 3), (150, 1)):
        want = sum(float(v) ** 2 for v in c[m, 64 * b:64 * b + 64].tolist())
        assert abs(float(ss[m, b]) - want) <= 1e-12 * want
    assert ss.shape == (M, 4) and ss0.shape == (M, 1) and ss.dtype == mc.F64
    # and they are the float64 truth's to the bf16 rounding of the elements: 2 * 2^-9 relative on a sum of squares, plus the
    # restatement's own slack on each element
    t, mag = mc.epilogue_op(d, "none", *mc.product(d))
    tt = (t[:, :256] ** 2).reshape(M, 4, 64).sum(-1)
    lim = 2.0 ** -8 * tt + 2 * ((t.abs() * mag)[:, :256]).reshape(M, 4, 64).sum(-1) * mc.SLACK
    assert bool(((ss - tt).abs() <= lim).all()), float(((ss - tt).abs() / lim).max())


@pytest.mark.parametrize("kind", xc.NORM_KINDS)
@pytest.mark.parametrize("rpg", xc.NORM_RPG)
def test_norm_quantise_restatement(kind, rpg):
    c = dict(rows=37, D=2080, kind=kind, rpg=rpg)
    x, table, temb = xc.norm_inputs(c)
    y, q, s = xc.norm_quant_restate(x, kind, table, temb, rpg)
    sc_t, sc_e, sh_t, sh_e = xc.modulation_views(table, temb, c["D"])
    args = (x, kind, xc.EPS, sc_t, nc.group_rows(sc_e, rpg, 37), sh_t, nc.group_rows(sh_e, rpg, 37))
    truth, mag = nc.norm_modulate_op(*args)
    # y is the truth rounded once; norm_cases' own comparison holds it
    nc.compare(y, truth, mag, what=f"norm_quant_restate {kind}")
    assert torch.equal(y.view(torch.int16), truth.to(mc.BF).view(torch.int16))
    # (q, scales) is mx8_cases.quantize of y, and de-quantised it is y to half an e4m3 ulp (2^-4 relative, 2^(e - 10) absolute)
    wq, ws = mc.quantize(y)
    assert torch.equal(s, ws) and torch.equal(q.view(torch.uint8), wq.view(torch.uint8))
    e = (s.to(torch.int32) - 127).repeat_interleave(32, dim=-1)
    err = (mc.dequantize(q, s) - y.to(mc.F64)).abs()
    assert bool((err <= torch.maximum(2.0 ** -4 * y.to(mc.F64).abs(), torch.ldexp(torch.ones_like(err), e - 10))).all())
    if rpg == 13:          # the groups are used: rows 12 and 13 take different modulation rows
        assert not torch.equal(nc.group_rows(sc_e, rpg, 37)[12], nc.group_rows(sc_e, rpg, 37)[13])


def test_witness_inputs_keep_the_scale_rule_at_its_edges():
    """Under a zero modulation the RMS norm multiplies a witness row by one factor: the row's block amax and the half-amax
    element keep their ratio, and the all-zero witness row stays zero (byte 0)."""
    D = 64
    x, table, temb = xc.witness_inputs(D)
    y, q, s = xc.norm_quant_restate(x, "rms", table, temb, 1)
    zero_row = [i for i, (amax, _, _) in enumerate(mc.WITNESSES) if amax == 0.0][0]
    assert bool((s[zero_row] == 0).all()) and bool((q[zero_row].view(torch.uint8) & 0x7f == 0).all())
    assert bool((table == 0).all()) and bool((temb == 0).all()) and x.shape[0] == len(mc.WITNESSES) + 2
    # every non-zero row is normalised to RMS 1: the amax of a block is then at most sqrt(D)
    nz = [i for i in range(x.shape[0]) if i != zero_row and float(x[i].double().abs().max()) > 1e-30]
    assert float(y[nz].double().abs().max()) <= D ** 0.5 * (1 + 2.0 ** -8)
