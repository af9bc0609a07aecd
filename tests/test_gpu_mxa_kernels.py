"""The two kernels of include/ltxmi_mx_attn.h on a real MI355X (cases and restatements: tests/mxa_cases.py, pinned on the CPU by
tests/test_mxa_cases.py).

  row sums    ltxmi_gemm_mx8_rowsumsq: C bit-equal to ops.gemm_mx8 on the same operands; the sums within rtol 1e-5 / atol 1e-6 of
              the float64 sums of squares of the STORED bf16 output; the -7.0 sentinels in the guard rows before and after, in the
              blocks past ``cols`` and in the padding of a row stay intact; two runs give equal bits.  On the flat probe's integer
              outputs (mxa_cases.rss_exact) the sums EQUAL the float64 sums and C the truth, at the first block, a whole band
              of tiles and into the narrow last band, inside NaN-filled buffers;
  fused norm  ltxmi_norm_modulate_mx8: (q, scales) bit-identical to ops.quantize_mx8(ops.norm_modulate(...)) with row-strided
              inputs and outputs and sentinels around them, and on mx8_cases' witness rows under a zero modulation."""
import pytest
import torch

import mx8_cases as mc
import mxa_cases as xc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5a

_operands = {}       # (family, M, N, K) -> mx8_cases.make's dict on the device, and ops.gemm_mx8's outputs with / without the bias


@pytest.fixture(scope="module", autouse=True)
def _free():
    yield
    _operands.clear()


def _gemm_inputs(c):
    from ltxmi import ops
    key = (c["family"],) + c["shape"]
    if key not in _operands:
        d = mc.make(c["family"], *c["shape"], "none", device=DEV)
        kw = dict(a=d["aq"], a_scales=d["a_scales"], w=d["wq"], w_scales=d["w_scales"])
        _operands[key] = (d, kw, {b: ops.gemm_mx8(**kw, bias=d["bias"] if b else None) for b in (True, False)})
    return _operands[key]


@pytest.mark.parametrize("c", xc.RSS_CASES, ids=xc.rss_id)
def test_gemm_rowsumsq(c):
    from ltxmi import ops
    M, N, K = c["shape"]
    d, kw, plain = _gemm_inputs(c)
    cols, nblk = c["cols"], (N + 63) // 64
    ld = nblk + 3                                              # every block of N and a padding, all of it sentinels
    bias = d["bias"] if c["bias"] else None
    runs = []
    for _ in range(2):
        buf = torch.full((M + 2, ld), -7.0, dtype=torch.float32, device=DEV)
        out = ops.gemm_mx8(**kw, bias=bias, rowsumsq=buf[1:M + 1], rowsumsq_cols=cols)
        torch.cuda.synchronize()
        runs.append((out, buf))
    out, buf = runs[0]
    assert torch.equal(out.view(torch.int16), plain[c["bias"]].view(torch.int16)), "C differs from ops.gemm_mx8's"
    assert torch.equal(out.view(torch.int16), runs[1][0].view(torch.int16)) and torch.equal(buf, runs[1][1]), "two runs differ"
    assert bool((buf[0] == -7.0).all()) and bool((buf[M + 1] == -7.0).all()), "wrote a guard row"
    assert bool((buf[1:M + 1, cols // 64:] == -7.0).all()), "wrote a block past rowsumsq_cols"
    got, want = buf[1:M + 1, :cols // 64].double().cpu(), xc.rowsumsq(out.cpu(), cols)
    err = (got - want).abs() - (xc.RSS_ATOL + xc.RSS_RTOL * want.abs())
    print(f"row sums: worst |got - want| - (atol + rtol |want|) = {float(err.max()):.3e}; "
          f"worst relative error {float(((got - want).abs() / want.abs().clamp_min(1e-30)).max()):.3e}")
    assert bool((err <= 0).all()), (err.argmax().item(), float(err.max()))


@pytest.mark.parametrize("c", xc.RSS_EXACT_CASES, ids=xc.rss_exact_id)
def test_gemm_rowsumsq_exact(c):
    """The flat probe's integer outputs: C must equal the float64 truth and ops.gemm_mx8's C bit for bit, and the sums the
    float64 sums with no tolerance.  C and the sums lie in buffers of NaN patterns: every output and every block below ``cols``
    is written, the blocks at or past ``cols``, the row padding and the guard rows keep the pattern."""
    from ltxmi import ops
    M, N, K = c["shape"]
    d = xc.rss_exact(c, device=DEV)
    kw = dict(a=d["aq"], a_scales=d["a_scales"], w=d["wq"], w_scales=d["w_scales"], bias=d["bias"])
    cols, nblk = c["cols"], (N + 63) // 64
    cbuf, out = mc.guarded(M, N, 8, "bf16", DEV)
    sbuf, sums = mc.guarded(M, nblk, 3, "f32", DEV)            # every block of N and a padding
    ops.gemm_mx8(**kw, out=out, rowsumsq=sums, rowsumsq_cols=cols)
    torch.cuda.synchronize()
    assert mc.guard_figures(cbuf, out, "bf16") == (0, 0), "(outputs never written, elements changed outside the output view)"
    want = d["truth"].to(mc.BF).to(DEV)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)), "C differs from the truth"
    assert torch.equal(out.view(torch.int16), ops.gemm_mx8(**kw).view(torch.int16)), "C differs from ops.gemm_mx8's"
    written = sums[:, :cols // 64]
    left, outside = mc.guard_figures(sbuf, written, "f32")
    assert outside == 0, f"{outside} values at or past rowsumsq_cols, in the padding or in a guard row changed"
    assert left == 0, f"{left} sums were never written"
    got = written.double().cpu()
    bad = (got != d["sums"]).nonzero()
    assert bad.numel() == 0, (bad[:4].tolist(), float(got[tuple(bad[0])]), float(d["sums"][tuple(bad[0])]))


def _strided(rows, cols, pad, dtype, fill):
    """A [rows, cols] view with row stride cols + pad inside a filled buffer with a guard row before and after."""
    ld = cols + pad
    buf = torch.full(((rows + 2) * ld,), fill, dtype=dtype, device=DEV)
    return buf, torch.as_strided(buf, (rows, cols), (ld, 1), ld)


def _untouched(buf, view, fill):
    b = buf.clone()
    torch.as_strided(b, view.shape, view.stride(), view.storage_offset()).fill_(fill)
    return bool((b == fill).all())


def _fused_against_two_launches(x, kind, table, temb, rpg):
    from ltxmi import ops
    rows, D = x.shape
    kind_id = ops.NORM_LAYER if kind == "layer" else ops.NORM_RMS
    xbuf, xv = _strided(rows, D, 8, mc.BF, 7.0)
    xv.copy_(x)
    mod = xc.modulation_views(table.to(DEV), temb.to(DEV), D)
    y = torch.empty(rows, D, dtype=mc.BF, device=DEV)
    ops.norm_modulate(xv, y, xc.EPS, kind_id, *mod, rpg)
    want_q, want_s = ops.quantize_mx8(y)
    qbuf, qv = _strided(rows, D, 16, torch.uint8, SENTINEL)
    sbuf, sv = _strided(rows, D // 32, 3, torch.uint8, SENTINEL)
    ops.norm_modulate_mx8(xv, xc.EPS, kind_id, *mod, rpg, out=(qv, sv))
    torch.cuda.synchronize()
    assert _untouched(qbuf, qv, SENTINEL) and _untouched(sbuf, sv, SENTINEL), "wrote outside the output views"
    assert _untouched(xbuf, xv, 7.0), "wrote the input's buffer"
    bad = (sv != want_s).nonzero()
    assert bad.numel() == 0, ("scale bytes", bad[:4].tolist(), int(sv[tuple(bad[0])]), int(want_s[tuple(bad[0])]))
    bad = (qv != want_q.view(torch.uint8)).nonzero()
    assert bad.numel() == 0, ("elements", bad[:4].tolist(), int(qv[tuple(bad[0])]), int(want_q.view(torch.uint8)[tuple(bad[0])]),
                              float(y[tuple(bad[0])]))
    # the contiguous, allocating form
    q2, s2 = ops.norm_modulate_mx8(x.to(DEV), xc.EPS, kind_id, *mod, rpg)
    assert q2.dtype == mc.E4M3 and torch.equal(q2.view(torch.uint8), want_q.view(torch.uint8)) and torch.equal(s2, want_s)
    return y, want_q, want_s


@pytest.mark.parametrize("c", xc.NORM_CASES, ids=xc.norm_id)
def test_norm_modulate_mx8_is_the_two_launches(c):
    x, table, temb = xc.norm_inputs(c, "row_scales" if c["rpg"] == 13 else "plain")
    _fused_against_two_launches(x, c["kind"], table, temb, c["rpg"])


@pytest.mark.parametrize("D", xc.NORM_D)
def test_norm_modulate_mx8_on_the_scale_rule_witnesses(D):
    x, table, temb = xc.witness_inputs(D)
    y, q, s = _fused_against_two_launches(x, "rms", table, temb, 1)
    # and what both computed is the format's rule on those bf16 values (mx8_cases.quantize): the witnesses still sit at its edges
    want_q, want_s = mc.quantize(y.cpu())
    assert torch.equal(s.cpu(), want_s) and torch.equal(q.view(torch.uint8).cpu(), want_q.view(torch.uint8))
