"""ltxmi_gemm_mx8_pair2 (include/ltxmi_mx_lora.h) on a real MI355X (cases: tests/mxl_cases.py, pinned on the CPU by
tests/test_mxl_cases.py).

  bit-identity  ops.gemm_mx8(..., a2=, w2=) equals ops.gemm_mx8 on the materialised concatenation [Aq | A2q_g], [Wq | W2q] bit for
                bit (bytes and scale bytes for the MX output), for every epilogue and output form, written into a view inside a
                buffer of NaN patterns (every output written, nothing outside it touched);
  row sums      with rowsumsq, C and the sums equal those of the row-sum GEMM on the concatenation bit for bit;
  groups        per group the column slice equals the concatenated call with that group's slice of A2;
  truth         the same outputs against the float64 truth of the concatenation with mx8_cases' figures and bounds -- no
                tolerance of this file's own;
  zero pairs    a zero W2q or a zero A2q (scale bytes 0) gives the bits of the one-pair call."""
import pytest
import torch

import gemm_cases as gc
import mx8_cases as mc
import mxl_cases as lc
from test_gpu_mx8_kernels import _epi

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _kw(d, epi, M, N):
    """The epilogue's keywords of ops.gemm_mx8 (the gate in place is set by the caller: it needs the output)."""
    kw = dict(bias=d["bias"], epilogue=_epi(epi))
    if epi == "gate":
        kw.update(gate_table=d["gate_table"], gate_temb=d["gate_temb"], rows_per_group=d["rows_per_group"])
    return kw


def _run(ops, operands, d, epi, mx, M, N, pair=None, **extra):
    """One call into guarded outputs -> the output view(s); asserts the guards."""
    kw = dict(_kw(d, epi, M, N), **extra)
    if pair:
        kw.update(pair)
    if mx:
        qbuf, qv = mc.guarded(M, N, 16, "e4m3", DEV)
        sbuf, sv = mc.guarded(M, N // 32, 5, "scale", DEV)
        ops.gemm_mx8(*operands, mx_out=True, out=(qv, sv), **kw)
        torch.cuda.synchronize()
        assert mc.guard_figures(qbuf, qv, "e4m3") == (0, 0) and mc.guard_figures(sbuf, sv, "scale") == (0, 0), \
            "(bytes never written, bytes changed outside the output views)"
        return qv, sv
    buf, out = mc.guarded(M, N, 8, "bf16", DEV)
    if epi in ("gate", "residual"):
        out.copy_(d["residual"])                  # in place, as the block's FF2 and to_out run
        kw["residual"] = out
    ops.gemm_mx8(*operands, out=out, **kw)
    torch.cuda.synchronize()
    assert mc.guard_figures(buf, out, "bf16") == (0, 0), "(outputs never written, elements changed outside the output view)"
    return out


def _same(got, want, what):
    if isinstance(got, tuple):
        assert torch.equal(got[1], want[1]), what + ": scale bytes differ"
        assert torch.equal(got[0], want[0]), what + ": element bytes differ"
    else:
        bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
        assert bad.numel() == 0, (what, bad.shape[0], bad[:4].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


@pytest.mark.parametrize("c", lc.CASES, ids=lc.case_id)
def test_two_pair_call_is_the_concatenated_call_and_meets_its_truth(c):
    from ltxmi import ops
    M, N = c["M"], c["N"]
    acc = None
    for epi, mx in lc.FORMS:
        d = lc.make(c, epi, DEV)[0]
        s = lc.split(c, [d])
        cat = lc.concatenation(c, s, 0)
        pair = dict(a2=s["a2"], w2=s["w2"])
        got = _run(ops, s["a"] + s["w"], d, epi, mx, M, N, pair)
        want = _run(ops, cat, d, epi, mx, M, N)
        what = f"{lc.case_id(c)} {epi} {'mx' if mx else 'bf16'}"
        _same(got, want, what)
        if acc is None:       # the operands are the same for every epilogue of a case: one float64 product
            acc = mc.product(d) + (mc.trunc_mag(d), d["aq"].view(torch.uint8).clone(), d["wq"].view(torch.uint8).clone())
        assert torch.equal(acc[3], d["aq"].view(torch.uint8)) and torch.equal(acc[4], d["wq"].view(torch.uint8)), \
            "the shared product belongs to other operands"
        truth, mag = mc.epilogue_op(d, epi, acc[0], mc.eff_mag(acc[1], acc[2]))
        if mx:
            assert bool((got[0] & 0x7f != 0x7f).all()), "a NaN element"
            f = mc.mx_out_figures(got[0], got[1], truth, mag)
            print(f"{what}: scale blocks outside the rule {f['scale_bad']}, worst value error {f['elem']:.3f} of its limit")
            assert f["scale_bad"] == 0 and f["elem"] <= 1.0, f
        else:
            gc.compare(got, truth, mag, what=what, slack=mc.SLACK)


def _sums(M, N):
    return mc.guarded(M, (N + 63) // 64, 3, "f32", DEV)


@pytest.mark.parametrize("c", lc.RSS_CASES, ids=lc.case_id)
def test_row_sums_are_those_of_the_concatenated_call(c):
    from ltxmi import ops
    M, N, cols = c["M"], c["N"], c["cols"]
    d = lc.make(c, "none", DEV)[0]
    s = lc.split(c, [d])
    sb1, s1 = _sums(M, N)
    sb2, s2 = _sums(M, N)
    got = _run(ops, s["a"] + s["w"], d, "none", False, M, N, dict(a2=s["a2"], w2=s["w2"]), rowsumsq=s1, rowsumsq_cols=cols)
    want = _run(ops, lc.concatenation(c, s, 0), d, "none", False, M, N, rowsumsq=s2, rowsumsq_cols=cols)
    _same(got, want, lc.case_id(c))
    assert torch.equal(sb1, sb2), "the sums (or what lies around them) differ"
    left, outside = mc.guard_figures(sb1, s1[:, :cols // 64], "f32")
    assert (left, outside) == (0, 0), "(sums never written, values changed at or past rowsumsq_cols or outside the view)"


@pytest.mark.parametrize("c", lc.GROUP_CASES, ids=lc.case_id)
def test_groups_read_their_own_columns_of_the_second_activation(c):
    from ltxmi import ops
    M, N, G, cols = c["M"], c["N"], c["groups"], c["cols"]
    gcols = lc.group_cols(c)
    ds = lc.make(c, "none", DEV)
    d = ds[0]
    s = lc.split(c, ds)
    u8 = s["a2"][0].view(torch.uint8)
    assert all(not torch.equal(u8[:, :c["K2"]], u8[:, g * c["K2"]:(g + 1) * c["K2"]]) for g in range(1, G))
    pair = dict(a2=s["a2"], w2=s["w2"], a2_group_cols=gcols)
    rss = {}
    if cols:
        sb1, s1 = _sums(M, N)
        rss = dict(rowsumsq=s1, rowsumsq_cols=cols)
    got = _run(ops, s["a"] + s["w"], d, "none", False, M, N, pair, **rss)
    for epi, mx in (("gelu", True), ("gelu", False)):
        outs = (_run(ops, s["a"] + s["w"], d, epi, mx, M, N, pair), )
        for g in range(G):
            want = _run(ops, lc.concatenation(c, s, g), d, epi, mx, M, N)
            sl = slice(g * gcols, (g + 1) * gcols)
            if mx:
                _same((outs[0][0][:, sl], outs[0][1][:, sl.start // 32:sl.stop // 32]),
                      (want[0][:, sl], want[1][:, sl.start // 32:sl.stop // 32]), f"{lc.case_id(c)} group {g} mx")
            else:
                _same(outs[0][:, sl], want[:, sl], f"{lc.case_id(c)} group {g} gelu")
    acc = None
    for g in range(G):
        sl = slice(g * gcols, (g + 1) * gcols)
        rss2 = {}
        if cols:
            sb2, s2 = _sums(M, N)
            rss2 = dict(rowsumsq=s2, rowsumsq_cols=cols)
        want = _run(ops, lc.concatenation(c, s, g), d, "none", False, M, N, **rss2)
        _same(got[:, sl], want[:, sl], f"{lc.case_id(c)} group {g}")
        if g == 0 and cols:                       # the sums lie in group 0's columns: the q rows of the packed q/k/v projection
            assert cols <= gcols and torch.equal(sb1, sb2), "the sums differ from the concatenated call's"
        # the truth of group g's columns
        cat = lc.concatenation(c, s, g)
        dg = dict(d, a=mc.dequantize(cat[0], cat[1]), w=mc.dequantize(cat[2], cat[3]))
        p, m = mc.product(dg)
        truth, mag = mc.epilogue_op(dg, "none", p, mc.eff_mag(m, mc.trunc_mag(dg)))
        gc.compare(got[:, sl], truth[:, sl], mag[:, sl], what=f"{lc.case_id(c)} group {g}", slack=mc.SLACK)


def test_a_refused_call_raises_and_writes_nothing():
    """K2 = 64 and a group width of 128 are refused by the entry check, a group width that does not divide N by ops.gemm_mx8
    itself: each raises and the output keeps its pattern.  (tests/test_mxl_abi.py holds the refusals that need no device.)"""
    from ltxmi import _lib, ops
    c = dict(M=300, N=768, K1=256, K2=128, family="plain", groups=1)
    d = lc.make(c, "none", DEV)[0]
    s = lc.split(c, [d])
    half = lambda t: (t[0][:, :64], t[1][:, :2])
    six = (s["a2"][0].view(torch.uint8).repeat(1, 6).view(mc.E4M3), s["a2"][1].repeat(1, 6))      # N / 128 = 6 groups
    for pair, error, word in ((dict(a2=half(s["a2"]), w2=half(s["w2"])), _lib.LtxmiError, "K2=64"),
                              (dict(a2=six, w2=s["w2"], a2_group_cols=128), _lib.LtxmiError, "group_cols=128"),
                              (dict(a2=s["a2"], w2=s["w2"], a2_group_cols=512), ValueError, "a2_group_cols=512")):
        buf, out = mc.guarded(c["M"], c["N"], 8, "bf16", DEV)
        with pytest.raises(error, match=word):
            ops.gemm_mx8(*s["a"], *s["w"], out=out, **pair)
        torch.cuda.synchronize()
        assert mc.guard_figures(buf, out, "bf16") == (c["M"] * c["N"], 0), "a refused call wrote into the output"


@pytest.mark.parametrize("which", ["w2", "a2"])
@pytest.mark.parametrize("form", lc.FORMS, ids=lambda f: f"{f[0]}-{'mx' if f[1] else 'bf16'}")
def test_a_zero_pair_gives_the_one_pair_bits(form, which):
    from ltxmi import ops
    epi, mx = form
    c = dict(M=300, N=288, K1=256, K2=128, family="row_scales", groups=1)
    M, N = c["M"], c["N"]
    d = lc.make(c, epi, DEV)[0]
    s = lc.split(c, [d])
    pair = dict(a2=s["a2"], w2=s["w2"])
    pair[which] = tuple(torch.zeros_like(t) for t in pair[which])
    got = _run(ops, s["a"] + s["w"], d, epi, mx, M, N, pair)
    # the first pair alone, as contiguous operands of K = K1
    one = tuple(t.contiguous() for t in s["a"] + s["w"])
    _same(got, _run(ops, one, d, epi, mx, M, N), f"zero {which} {epi}")
