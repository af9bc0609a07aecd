"""The MX-FP8 quantiser and the block-scaled MFMA GEMM on a real MI355X (cases, restatement, truth and slack: tests/mx8_cases.py,
pinned on the CPU by tests/test_mx8_cases.py).

  quantiser     bit-identical to the restatement: rows {1, 37, 300} x K {32, 64, 2080}, padded strides on all three arrays,
                input families plain, row_scales and the exponent-rule / rounding witnesses;
  layout probe  the FIRST GEMM test: one-hot rows against asymmetric small integers with a different power-of-two scale in every
                block and row on both sides.  Every output is one exactly representable product and must match bit for bit: a
                swapped lane map, a scale from the wrong block or a permuted K fails on almost every element.  Both operands take
                the one-hot role in turn (each checks the other's map).  Shapes (mx8_cases.PROBE_SHAPES): 1, 2, 3, 4, 5 and 7
                K-tiles -- every path of the prologue and the K loop -- and the grids 1 x 1, 2 x 1, 2 x 10 and 3 x 12 of the band
                walk (a last band narrower than 8 tiles, a 32-column last tile, one valid row in a tile).  Variants: scale bytes
                over 1 .. 253, and operands as strided views at 4-byte aligned scale addresses;
  outputs       every GEMM test hands in its output inside a buffer of NaN patterns (mx8_cases.guarded): none may be left
                inside the view, nothing outside it may change;
  exact         the flat probe (integer outputs) under every epilogue that is exact on such data -- bias and no bias, residual
                out of and in place, the gate with 1, 7 and M + 3 rows per group, the e4m3 pack and its scale -- with zero
                tolerance; the fp32 scale rule exactly at, above and below its threshold 1.75 * 2^k;
  witness      exact data that shows how the scaled MFMA sums (a cut at 2^-13 of the largest product inside a group of 8 k): the
                reason for the TRUNC term below;
  random        plain / cancel / row_scales at (300, 288, 256) and (2048, 4096, 8192), M = 1, every epilogue: per element
                2^-7 |truth| + SLACK mag + TRUNC tmag, plus the per-row and per-256-column figures of gemm_cases.compare (on the
                cancel family with a residual: those figures on the error in excess of TRUNC tmag, see the test);
  MX output     the stored scale against the restatement applied to the truth, and the de-quantised value against the truth
                (mx8_cases.mx_out_figures).
The float64 truth is computed on the device (rocBLAS, independent of this library), once per (family, shape).

WHICH FIGURE BINDS.  TRUNC * tmag is the WORST case of the cut the witness shows (seven products of a group of 8 lost whole), about
5e-4 of mag on the random families, where the error measured is 1.4e-6 of mag: the per-element limit is there to catch a wrong
value (a wrong scale is a factor of two, a wrong element the size of mag / K), not to measure rounding.  What holds the rounding:
  plain, row_scales   the per-row and per-256-column relative L2 (3e-3) and max (1.6e-2) of gemm_cases.compare, unchanged; the
                      closest is the block L2 at 0.82 of its limit (row_scales, gate);
  cancel, none/gelu   the same figures (one row per column is a residue; the L2 of a row or block is held by the others);
  cancel + residual   every output is a residue, so the relative figures measure only how the accumulator was summed and the cut
                      alone is 2 - 4 x their limits.  They are taken on the error in excess of TRUNC * tmag; there the per-element
                      limit is what binds, and the raw figures are printed.  No tighter limit is set for them: one would have to
                      come from what this kernel gives, and the cut's typical size is the hardware's, not reasoned here;
  MX output           the scale byte (exact, or off by one within 2^-7 of a threshold) and 2^-4 |g| per element: half an e4m3 ulp."""
import pytest
import torch

import gemm_cases as gc
import mx8_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5a

_products = {}       # (family, M, N, K) -> (aq, acc, mag): the epilogues of a (family, shape) share the float64 product


@pytest.fixture(scope="module", autouse=True)
def _free():
    yield
    _products.clear()


def _epi(name):
    from ltxmi import ops
    return {"none": ops.EPI_NONE, "gelu": ops.EPI_GELU_TANH, "gate": ops.EPI_GATE_RESIDUAL, "residual": ops.EPI_GATE_RESIDUAL}[name]


def _strided(rows, cols, pad, dtype, fill):
    """A [rows, cols] view with row stride cols + pad inside a filled buffer with a guard row before and after."""
    ld = cols + pad
    buf = torch.full(((rows + 2) * ld,), fill, dtype=torch.uint8 if dtype != mc.BF else mc.BF, device=DEV)
    return buf, torch.as_strided(buf, (rows, cols), (ld, 1), ld)


def _untouched(buf, view, fill):
    b = buf.clone()
    torch.as_strided(b, view.shape, view.stride(), view.storage_offset()).fill_(fill)
    return bool((b == fill).all())


# ------------------------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("family", mc.QUANT_FAMILIES)
@pytest.mark.parametrize("K", mc.QUANT_K)
@pytest.mark.parametrize("rows", mc.QUANT_ROWS)
def test_quantizer_is_bit_identical_to_the_restatement(rows, K, family):
    from ltxmi import ops
    x = mc.quant_input(family, rows, K)
    want_q, want_s = mc.quantize(x)
    xbuf, xv = _strided(rows, K, 8, mc.BF, 7.0)
    xv.copy_(x)
    qbuf, qv = _strided(rows, K, 16, torch.uint8, SENTINEL)
    sbuf, sv = _strided(rows, K // 32, 3, torch.uint8, SENTINEL)
    ops.quantize_mx8(xv, out=(qv, sv))
    torch.cuda.synchronize()
    assert _untouched(qbuf, qv, SENTINEL) and _untouched(sbuf, sv, SENTINEL), "wrote outside the output views"
    assert torch.equal(sv.cpu(), want_s), "scale bytes"
    got, want = qv.cpu(), want_q.view(torch.uint8)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], float(x[tuple(bad[0])]))
    # the contiguous, allocating form
    q2, s2 = ops.quantize_mx8(x.to(DEV))
    assert q2.dtype == mc.E4M3 and torch.equal(q2.view(torch.uint8).cpu(), want) and torch.equal(s2.cpu(), want_s)


# ------------------------------------------------------------------------------------------------- layout probe
@pytest.mark.parametrize("one_hot", ["a", "w"])
@pytest.mark.parametrize("shape", mc.PROBE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_probe(shape, one_hot):
    from ltxmi import ops
    M, N, K = shape
    aq, a_s, wq, w_s, want = mc.probe(M, N, K, one_hot, device=DEV)
    _bf16_equals(lambda out: ops.gemm_mx8(aq, a_s, wq, w_s, out=out), want)


def _bf16_equals(call, want, prepare=None):
    """``call(out)`` on a guarded [M, N] bf16 view (``prepare(out)`` fills it first: an in-place residual): nothing outside the
    view changed, no guard pattern is left inside it -- a tile never written fails here by itself -- and the view holds
    ``want``'s bits.  -> the view."""
    M, N = want.shape
    buf, out = mc.guarded(M, N, 8, "bf16", DEV)
    if prepare is not None:
        prepare(out)
    call(out)
    torch.cuda.synchronize()
    left, outside = mc.guard_figures(buf, out, "bf16")
    assert outside == 0, f"{outside} elements outside the output view changed"
    assert left == 0, f"{left} outputs were never written"
    same = out.view(torch.int16) == want.to(DEV).view(torch.int16)
    assert bool(same.all()), (f"{int((~same).sum())} of {same.numel()} outputs differ; first at {(~same).nonzero()[0].tolist()}: "
                              f"{float(out[tuple((~same).nonzero()[0])])} for {float(want[tuple((~same).nonzero()[0])])}")
    return out


@pytest.mark.parametrize("one_hot", ["a", "w"])
@pytest.mark.parametrize("v", mc.PROBE_VARIANTS, ids=lambda v: "x".join(map(str, v["shape"])) + f"-{v['scales']}-{v['geometry']}")
def test_layout_probe_variants(v, one_hot):
    """Scale bytes over the whole E8M0 range, and operands handed over as views (lda > K, lda_s > K / 32 from a 4-byte aligned
    address, the weight a row range of a taller matrix): the expected bits, and for the views also the contiguous call's."""
    from ltxmi import ops
    M, N, K = v["shape"]
    aq, a_s, wq, w_s, want = mc.probe(M, N, K, one_hot, v["scales"], v["geometry"], device=DEV)
    out = _bf16_equals(lambda out: ops.gemm_mx8(aq, a_s, wq, w_s, out=out), want)
    if v["geometry"] == "strided":
        assert aq.stride(0) == K + 16 and a_s.stride(0) == K // 32 + 4 and a_s.data_ptr() % 16 == 4 and wq.data_ptr() % 16 == 0
        ref = ops.gemm_mx8(*(t.view(torch.uint8).contiguous() for t in (aq, a_s, wq, w_s)))
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), "the views and the contiguous operands give other bits"


# ------------------------------------------------------------------------------------------------- exact epilogues
def _exact_kw(c, d):
    from ltxmi import ops
    kw = dict(bias=d["bias"], epilogue=_epi(c["epi"]))
    if c["epi"] == "gate":
        kw.update(gate_table=d["gate_table"], gate_temb=d["gate_temb"], rows_per_group=d["rows_per_group"])
    return kw


@pytest.mark.parametrize("c", [c for c in mc.EXACT_CASES if c["out"] == "bf16"], ids=mc.exact_id)
def test_exact_epilogues_bf16_output(c):
    """Integer (and half-integer) data on which every fp32 operation of the epilogue is exact (mx8_cases.exact_ok): the bias and
    its absence, the residual out of place and in place, the gate with groups of 1, 7 and all rows.  Zero tolerance."""
    from ltxmi import ops
    M, N, K = c["shape"]
    d = mc.exact(c, device=DEV)
    kw, prepare = _exact_kw(c, d), None
    if c["epi"] in ("gate", "residual"):
        if c["in_place"]:
            prepare = lambda out: out.copy_(d["residual"])
        else:                                       # a residual with a stride of its own
            _, res = _strided(M, N, 16, mc.BF, 0.0)
            res.copy_(d["residual"])
            kw["residual"] = res

    def call(out):
        if c["in_place"]:
            kw["residual"] = out
        ops.gemm_mx8(d["aq"], d["a_scales"], d["wq"], d["w_scales"], out=out, **kw)
    _bf16_equals(call, d["truth"].to(mc.BF), prepare)


def _mx_equals(call, M, N, want_q, want_s):
    """``call((q, scales))`` on guarded views: nothing outside them changed, no NaN byte is left inside, and the bytes EQUAL
    the expected ones (no allowance near a threshold)."""
    qbuf, qv = mc.guarded(M, N, 16, "e4m3", DEV)
    sbuf, sv = mc.guarded(M, N // 32, 5, "scale", DEV)
    call((qv, sv))
    torch.cuda.synchronize()
    for buf, view, kind in ((qbuf, qv, "e4m3"), (sbuf, sv, "scale")):
        left, outside = mc.guard_figures(buf, view, kind)
        assert outside == 0, f"{kind}: {outside} bytes outside the output view changed"
        assert left == 0, f"{kind}: {left} bytes were never written"
    bad = (sv != want_s.to(DEV)).nonzero()
    assert bad.numel() == 0, ("scale bytes", bad[:4].tolist(), int(sv[tuple(bad[0])]), int(want_s[tuple(bad[0])]))
    want = want_q.view(torch.uint8).to(DEV)
    bad = (qv != want).nonzero()
    assert bad.numel() == 0, ("elements", bad[:4].tolist(), int(qv[tuple(bad[0])]), int(want[tuple(bad[0])]))


@pytest.mark.parametrize("c", [c for c in mc.EXACT_CASES if c["out"] == "mx"], ids=mc.exact_id)
def test_exact_mx_output(c):
    """Integers of magnitude <= 15: exact in e4m3 under the scale the rule picks, so the stored bytes are the restated quantiser's
    on the float64 truth."""
    from ltxmi import ops
    M, N, K = c["shape"]
    d = mc.exact(c, device=DEV)
    want_s = mc.scale_bytes_real(d["truth"])
    want_q = mc.quantize_elements(d["truth"], want_s)
    _mx_equals(lambda out: ops.gemm_mx8(d["aq"], d["a_scales"], d["wq"], d["w_scales"], mx_out=True, out=out, **_exact_kw(c, d)),
               M, N, want_q, want_s)


def test_mx_output_scale_rule_at_its_threshold():
    """fp32 accumulators exactly at, above and below 1.75 * 2^k (mx8_cases.witness_mx_out_threshold).  First the sums themselves:
    the bf16-output call with a residual that cancels the large term returns the exact remainder -- if that fails, the hardware's
    sum is what differs.  Then the MX-output bytes -- if those fail, the rule is."""
    from ltxmi import ops
    w = mc.witness_mx_out_threshold()
    ops_in = [w[k].to(DEV) for k in ("aq", "a_scales", "wq", "w_scales")]
    rows, N = w["residual"].shape
    _bf16_equals(lambda out: ops.gemm_mx8(*ops_in, out=out, epilogue=ops.EPI_GATE_RESIDUAL, residual=w["residual"].to(DEV)),
                 w["after"][:, None].expand(rows, N).to(mc.BF))
    _mx_equals(lambda out: ops.gemm_mx8(*ops_in, mx_out=True, out=out), rows, N, w["q"], w["scales"])


def test_scaled_mfma_truncation_witness():
    """Why the per-element limit carries TRUNC * tmag (tests/mx8_cases.py): the hardware's own sum of exact data."""
    from ltxmi import ops
    aq, a_s, wq, w_s, resid, hw, exact = mc.witness_truncation()
    out = ops.gemm_mx8(aq.to(DEV), a_s.to(DEV), wq.to(DEV), w_s.to(DEV), epilogue=ops.EPI_GATE_RESIDUAL, residual=resid.to(DEV))
    torch.cuda.synchronize()
    got = out.double().cpu()
    assert bool((got == got[:, :1]).all())
    print("in-group cut, rows as mx8_cases.witness_truncation lists them:", got[:, 0].tolist())
    assert got[:, 0].tolist() == hw.tolist()
    # and the limit the GPU cases use covers it: the loss is below TRUNC * tmag
    d = dict(a=mc.dequantize(aq, a_s), w=mc.dequantize(wq, w_s))
    assert bool(((exact - got[:, 0]).abs() <= mc.TRUNC * mc.trunc_mag(d)[:, 0]).all())


# ------------------------------------------------------------------------------------------------- random families
def _inputs(c):
    M, N, K = c["shape"]
    d = mc.make(c["family"], M, N, K, c["epi"], device=DEV)
    key = (c["family"], M, N, K)
    if key not in _products:
        if len(_products) > 1:
            _products.pop(next(iter(_products)))
        acc, mag = mc.product(d)
        _products[key] = (d["aq"].view(torch.uint8).clone(), acc, mag, mc.trunc_mag(d))
    aq, acc, mag, tmag = _products[key]
    assert torch.equal(aq, d["aq"].view(torch.uint8)), "the shared product belongs to other operands"
    t, m = mc.epilogue_op(d, c["epi"], acc, mc.eff_mag(mag, tmag))
    # TRUNC * tmag as the epilogue scales it (the gate), for the cases whose group figures need it
    tb = mc.TRUNC * (mc.epilogue_op(d, c["epi"], acc, tmag)[1] - mc.epilogue_op(d, c["epi"], acc, torch.zeros_like(tmag))[1])
    return d, t, m, tb


def _call(c, d, **kw):
    M, N, K = c["shape"]
    kw.update(bias=d["bias"], epilogue=_epi(c["epi"]))
    if c["epi"] == "gate":
        kw.update(gate_table=d["gate_table"], gate_temb=d["gate_temb"], rows_per_group=d["rows_per_group"])
    return kw


@pytest.mark.parametrize("c", mc.GEMM_CASES, ids=mc.case_id)
def test_gemm_bf16_output(c):
    from ltxmi import ops
    M, N, K = c["shape"]
    d, truth, mag, tb = _inputs(c)
    buf, out = mc.guarded(M, N, 8, "bf16", DEV)
    kw = _call(c, d, out=out)
    if c["epi"] == "gate":                      # in place, as the block's FF2 runs
        out.copy_(d["residual"])
        kw["residual"] = out
    elif c["epi"] == "residual":                # out of place, a residual with a stride of its own
        _, res = _strided(M, N, 16, mc.BF, 0.0)
        res.copy_(d["residual"])
        kw["residual"] = res
    ops.gemm_mx8(d["aq"], d["a_scales"], d["wq"], d["w_scales"], **kw)
    torch.cuda.synchronize()
    assert mc.guard_figures(buf, out, "bf16") == (0, 0), "(outputs never written, elements changed outside the output view)"
    if c["family"] == "cancel" and c["epi"] in ("gate", "residual"):
        # Every output is the rounding residue of its own accumulator here: the truth is 2^-9 of the accumulator, and the
        # whole-tensor, per-row and per-block figures -- relative to the TRUTH's norm, with no magnitude term -- measure nothing but
        # how the accumulator was summed.  The scaled MFMA's in-group cut (the witness above) is 2 to 4 times their limits on this
        # family (measured: row L2 2.3 - 3.3, block L2 3.0 - 3.6, whole tensor 2.1 of the limit).  So those figures are taken
        # on the error in EXCESS of TRUNC * tmag, element by element; the per-element limit is the one of every other case.
        assert bool(torch.isfinite(out.float()).all()), "non-finite output"
        err = out.to(mc.F64) - truth
        excess = torch.sign(err) * (err.abs() - tb).clamp_min(0)
        f = gc.figures(out, truth, mag, mc.SLACK)
        print(f"{mc.case_id(c)}: raw figures " + " ".join(f"{k} {v:.3f}" for k, v in sorted(f.items())))
        assert f["elem"] <= 1.0, f
        gc.compare(truth + excess, truth, mag, what=mc.case_id(c) + " (in excess of the cut)",
                   slack=mc.SLACK)
        return
    gc.compare(out, truth, mag, what=mc.case_id(c), slack=mc.SLACK)


@pytest.mark.parametrize("c", mc.MXOUT_CASES, ids=mc.case_id)
def test_gemm_mx_output(c):
    from ltxmi import ops
    M, N, K = c["shape"]
    d, truth, mag, _ = _inputs(c)
    qbuf, qv = mc.guarded(M, N, 16, "e4m3", DEV)
    sbuf, sv = mc.guarded(M, N // 32, 5, "scale", DEV)
    ops.gemm_mx8(d["aq"], d["a_scales"], d["wq"], d["w_scales"], mx_out=True, out=(qv, sv), **_call(c, d))
    torch.cuda.synchronize()
    assert mc.guard_figures(qbuf, qv, "e4m3") == (0, 0) and mc.guard_figures(sbuf, sv, "scale") == (0, 0), \
        "(bytes never written, bytes changed outside the output views)"
    assert bool((qv & 0x7f != 0x7f).all()), "a NaN element"
    f = mc.mx_out_figures(qv, sv, truth, mag)
    print(f"{mc.case_id(c)} mx-out: scale blocks outside the rule {f['scale_bad']}, worst value error {f['elem']:.3f} of its limit")
    assert f["scale_bad"] == 0 and f["elem"] <= 1.0, f


def test_mx_output_feeds_the_next_gemm():
    """FF1 -> FF2 as the block will run them: the (q, scales) pair ops.gemm_mx8 returns is what it takes."""
    from ltxmi import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 256, generator=g).to(mc.BF).to(DEV)
    w1 = (torch.randn(1024, 256, generator=g) / 16).to(mc.BF).to(DEV)
    w2 = (torch.randn(256, 1024, generator=g) / 32).to(mc.BF).to(DEV)
    xq, w1q, w2q = ops.quantize_mx8(x), ops.quantize_mx8(w1), ops.quantize_mx8(w2)
    h = ops.gemm_mx8(*xq, *w1q, epilogue=ops.EPI_GELU_TANH, mx_out=True)
    assert h[0].dtype == mc.E4M3 and h[0].shape == (300, 1024) and h[1].shape == (300, 32)
    y = ops.gemm_mx8(*h, *w2q)
    torch.cuda.synchronize()
    hd = mc.dequantize(h[0], h[1])
    want = hd @ mc.dequantize(*w2q).T
    dd = dict(a=hd, w=mc.dequantize(*w2q))
    mag = mc.eff_mag(hd.abs() @ dd["w"].abs().T, mc.trunc_mag(dd))
    gc.compare(y, want, mag, what="ff1 -> ff2", slack=mc.SLACK)
