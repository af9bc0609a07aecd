"""The kernels of include/ltxmi_mx_t5.h on a real MI355X.

  skinny GEMM   ltxmi_gemm_mx8_skinny's contract is ops.gemm_mx8's bits: every tile form, forced, against ops.gemm_mx8 on the same
                operands with torch.equal.  M {1, 33, 200, 512} x N {288 (ragged against the 64-column tile), 4096} x K-tile counts
                {1, stages - 1, stages, 2 stages + 1} of the ring depth the header states, the families of tests/mx8_cases.py, the
                epilogues none (with a bias, ldc > N) and residual (the residual IS the output, ldc > N); the guard rows and the
                row padding of the output stay as they were.  The reference is computed once per (family, shape, epilogue) and
                shared by the forms.  ``_form`` pins the form of every case first.  Every K-tile count used is one at which
                tests/mx8_cases.py holds ops.gemm_mx8 itself to an independent truth (asserted);
  witnesses     mx8_cases.probe (one exactly representable product per output: the operand, scale and C/D lane maps) and
                mx8_cases.witness_truncation (the hardware's own in-group cut) on every form, against the expected values
                themselves, not against another kernel;
  XXL shapes    (512, 4096, 10240) and (512, 20480, 4096) once each, the form chosen by shape;
  row passes    ltxmi_rmsnorm_weight_mx8 and ltxmi_gated_gelu_mx8 against the two launches they replace with torch.equal: rows
                {1, 37, 300} x D {128, 4096} (1000 is refused), mx8_cases' witness rows and row_scales rows, row-strided inputs
                and outputs with sentinels around them."""
import pytest
import torch

import mx8_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5a

_refs = {}           # (family, M, N, K, epi) -> the operands on the device and ops.gemm_mx8's output for them


@pytest.fixture(scope="module", autouse=True)
def _free():
    yield
    _refs.clear()


def _forms():
    from ltxmi import ops
    return ops.MXT_FORMS


def _ktiles():
    from ltxmi import ops
    s = ops.MXT_STAGES
    return sorted({1, s - 1, s, 2 * s + 1})


def _strided(rows, cols, pad, dtype, fill):
    """A [rows, cols] view with row stride cols + pad inside a filled buffer with a guard row before and after."""
    ld = cols + pad
    buf = torch.full(((rows + 2) * ld,), fill, dtype=dtype, device=DEV)
    return buf, torch.as_strided(buf, (rows, cols), (ld, 1), ld)


def _untouched(buf, view, fill):
    b = buf.clone()
    torch.as_strided(b, view.shape, view.stride(), view.storage_offset()).fill_(fill)
    return bool((b == fill).all())


def _reference(family, M, N, K, epi):
    """Operands of mx8_cases.make and what ops.gemm_mx8 gives for them: none = with the bias; residual = without one (the skinny
    entry takes no bias beside a residual), the residual being the output's own previous content."""
    from ltxmi import ops
    key = (family, M, N, K, epi)
    if key not in _refs:
        d = mc.make(family, M, N, K, epi, device=DEV)
        kw = dict(a=d["aq"], a_scales=d["a_scales"], w=d["wq"], w_scales=d["w_scales"])
        if epi == "none":
            extra = dict(bias=d["bias"])
            ref = ops.gemm_mx8(**kw, **extra)
        else:
            extra = dict(epilogue=ops.EPI_GATE_RESIDUAL)
            _, ref = _strided(M, N, 8, mc.BF, 7.0)
            ref.copy_(d["residual"])
            ops.gemm_mx8(**kw, **extra, residual=ref, out=ref)
        _refs[key] = (kw, extra, d.get("residual"), ref)
    return _refs[key]


def _check_case(form, family, M, N, K, epi):
    from ltxmi import ops
    kw, extra, residual, ref = _reference(family, M, N, K, epi)
    buf, out = _strided(M, N, 8, mc.BF, 7.0)
    if epi == "residual":
        out.copy_(residual)
        extra = dict(extra, residual=out)
    assert ops.gemm_mx8_skinny_form(**kw, **extra, out=out, form=form) == form
    ops.gemm_mx8_skinny(**kw, **extra, out=out, form=form)
    torch.cuda.synchronize()
    assert _untouched(buf, out, 7.0), "wrote outside the output view"
    same = out.view(torch.int16) == ref.view(torch.int16)
    assert bool(same.all()), (f"form {form} {family} {M}x{N}x{K} {epi}: {int((~same).sum())} of {same.numel()} outputs differ from "
                              f"ops.gemm_mx8; first at {(~same).nonzero()[0].tolist()}")


@pytest.mark.parametrize("N", [288, 4096])
@pytest.mark.parametrize("M", [1, 33, 200, 512])
@pytest.mark.parametrize("ktiles", [0, 1, 2, 3], ids=lambda i: f"ktiles{i}")
def test_skinny_gemm_is_bit_identical_to_gemm_mx8(ktiles, M, N):
    K = 128 * _ktiles()[ktiles]
    for family in mc.FAMILIES:
        for epi in ("none", "residual"):
            for form in _forms():
                _check_case(form, family, M, N, K, epi)
    _refs.clear()


def test_the_k_tile_counts_cover_the_ring():
    from ltxmi import ops
    s = ops.MXT_STAGES
    assert _ktiles() == [1, s - 1, s, 2 * s + 1] and len(_ktiles()) == 4


def test_every_k_tile_count_has_a_truth_behind_gemm_mx8():
    """The skinny kernel is held to ops.gemm_mx8's bits; ops.gemm_mx8 is held to an independent truth at the K-tile counts of
    mx8_cases.PROBE_SHAPES.  Every count used here must be among them, or the chain skinny -> gemm_mx8 -> truth is open."""
    assert set(_ktiles()) <= set(mc.TRUTH_KTILES), (_ktiles(), mc.TRUTH_KTILES)
    assert mc.TRUTH_KTILES == sorted({s[2] // 128 for s in mc.PROBE_SHAPES})


@pytest.mark.parametrize("one_hot", ["a", "w"])
@pytest.mark.parametrize("shape", [(300, 288, 256), (512, 544, 128 * 5)], ids=lambda s: "x".join(map(str, s)))
def test_layout_probe_on_every_form(shape, one_hot):
    from ltxmi import ops
    M, N, K = shape
    aq, a_s, wq, w_s, want = mc.probe(M, N, K, one_hot)
    args = (aq.to(DEV), a_s.to(DEV), wq.to(DEV), w_s.to(DEV))
    for form in _forms():
        assert ops.gemm_mx8_skinny_form(*args, form=form) == form
        got = ops.gemm_mx8_skinny(*args, form=form).cpu()
        same = got.view(torch.int16) == want.view(torch.int16)
        assert bool(same.all()), (f"form {form}: {int((~same).sum())} of {same.numel()} outputs differ; first at "
                                  f"{(~same).nonzero()[0].tolist()}")


def test_truncation_witness_on_every_form():
    from ltxmi import ops
    aq, a_s, wq, w_s, resid, hw, exact = mc.witness_truncation()
    for form in _forms():
        out = resid.to(DEV).clone()
        assert ops.gemm_mx8_skinny_form(aq.to(DEV), a_s.to(DEV), wq.to(DEV), w_s.to(DEV), epilogue=ops.EPI_GATE_RESIDUAL,
                                        residual=out, out=out, form=form) == form
        ops.gemm_mx8_skinny(aq.to(DEV), a_s.to(DEV), wq.to(DEV), w_s.to(DEV), epilogue=ops.EPI_GATE_RESIDUAL, residual=out, out=out,
                            form=form)
        got = out.double().cpu()
        assert bool((got == got[:, :1]).all())
        assert got[:, 0].tolist() == hw.tolist(), form


@pytest.mark.parametrize("shape", [(512, 4096, 10240), (512, 20480, 4096)], ids=lambda s: "x".join(map(str, s)))
def test_xxl_shapes(shape):
    from ltxmi import ops
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(7)
    a = torch.randn(M, K, generator=g, device=DEV).to(mc.BF)
    w = (torch.randn(N, K, generator=g, device=DEV) / 64).to(mc.BF)
    aq, wq = ops.quantize_mx8(a), ops.quantize_mx8(w)
    resid = torch.randn(M, N, generator=g, device=DEV).to(mc.BF)
    assert ops.gemm_mx8_skinny_form(*aq, *wq) == ops.MXT_FORMS[0]            # 128 x 64 tiles: 256 and 1280 workgroups
    assert torch.equal(ops.gemm_mx8_skinny(*aq, *wq).view(torch.int16), ops.gemm_mx8(*aq, *wq).view(torch.int16))
    out, ref = resid.clone(), resid.clone()
    ops.gemm_mx8_skinny(*aq, *wq, epilogue=ops.EPI_GATE_RESIDUAL, residual=out, out=out)
    ops.gemm_mx8(*aq, *wq, epilogue=ops.EPI_GATE_RESIDUAL, residual=ref, out=ref)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


def test_rows_above_the_limit_are_refused():
    from ltxmi import _lib, ops
    aq, a_s = torch.zeros(ops.MXT_MAX_ROWS + 1, 128, dtype=mc.E4M3, device=DEV), torch.zeros(ops.MXT_MAX_ROWS + 1, 4, dtype=torch.uint8, device=DEV)
    wq, w_s = torch.zeros(32, 128, dtype=mc.E4M3, device=DEV), torch.zeros(32, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.LtxmiError, match="row limit"):
        ops.gemm_mx8_skinny(aq, a_s, wq, w_s)


# ------------------------------------------------------------------------------------------------- the two row passes
ROWS, WIDTHS = (1, 37, 300), (128, 4096)
ROW_FAMILIES = ["witnesses", "row_scales"]


def _same_pair(got, want, y):
    (qv, sv), (want_q, want_s) = got, want
    bad = (sv != want_s).nonzero()
    assert bad.numel() == 0, ("scale bytes", bad[:4].tolist(), int(sv[tuple(bad[0])]), int(want_s[tuple(bad[0])]))
    bad = (qv.view(torch.uint8) != want_q.view(torch.uint8)).nonzero()
    assert bad.numel() == 0, ("elements", bad[:4].tolist(), int(qv.view(torch.uint8)[tuple(bad[0])]),
                              int(want_q.view(torch.uint8)[tuple(bad[0])]), float(y[tuple(bad[0])]))


@pytest.mark.parametrize("family", ROW_FAMILIES)
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_rmsnorm_weight_mx8_is_the_two_launches(rows, D, family):
    from ltxmi import ops
    x = mc.quant_input(family, rows, D)
    weight = (1.0 + 0.25 * torch.randn(D, generator=torch.Generator().manual_seed(D))).to(mc.BF).to(DEV)
    xbuf, xv = _strided(rows, D, 8, mc.BF, 7.0)                # a row-strided input
    xv.copy_(x)
    y = ops.rmsnorm_weight(xv, weight, 1e-6)
    want = ops.quantize_mx8(y)
    qbuf, qv = _strided(rows, D, 16, torch.uint8, SENTINEL)
    sbuf, sv = _strided(rows, D // 32, 3, torch.uint8, SENTINEL)
    ops.rmsnorm_weight_mx8(xv, weight, 1e-6, out=(qv, sv))
    torch.cuda.synchronize()
    assert _untouched(qbuf, qv, SENTINEL) and _untouched(sbuf, sv, SENTINEL), "wrote outside the output views"
    assert _untouched(xbuf, xv, 7.0), "wrote the input's buffer"
    _same_pair((qv, sv), want, y)
    got = ops.rmsnorm_weight_mx8(x.to(DEV), weight, 1e-6)      # the contiguous, allocating form
    assert got[0].dtype == mc.E4M3
    _same_pair(got, want, y)


@pytest.mark.parametrize("family", ROW_FAMILIES)
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_gated_gelu_mx8_is_the_two_launches(rows, F, family):
    from ltxmi import ops
    # the activation half spans the GELU's whole range (the witnesses reach 3e38 and the denormals), the gate half other rows
    h = torch.cat([mc.quant_input(family, rows, F), mc.quant_input("row_scales", rows, F, seed=1)], dim=1)
    hbuf, hv = _strided(rows, 2 * F, 8, mc.BF, 7.0)
    hv.copy_(h)
    y = ops.gated_gelu(hv)
    want = ops.quantize_mx8(y)
    qbuf, qv = _strided(rows, F, 16, torch.uint8, SENTINEL)
    sbuf, sv = _strided(rows, F // 32, 3, torch.uint8, SENTINEL)
    ops.gated_gelu_mx8(hv, out=(qv, sv))
    torch.cuda.synchronize()
    assert _untouched(qbuf, qv, SENTINEL) and _untouched(sbuf, sv, SENTINEL), "wrote outside the output views"
    assert _untouched(hbuf, hv, 7.0), "wrote the input's buffer"
    _same_pair((qv, sv), want, y)
    _same_pair(ops.gated_gelu_mx8(h.to(DEV)), want, y)


def test_a_width_that_is_no_multiple_of_32_is_refused():
    from ltxmi import ops
    x = torch.zeros(4, 1000, dtype=mc.BF, device=DEV)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.rmsnorm_weight_mx8(x, torch.ones(1000, dtype=mc.BF, device=DEV), 1e-6)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.gated_gelu_mx8(torch.zeros(4, 2000, dtype=mc.BF, device=DEV))
