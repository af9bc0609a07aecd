"""The normalisation kernels on a real MI355X at their dispatch edges and on hard inputs.

rowops.hip (``norm_modulate`` RMS / Layer, ``rmsnorm_rope`` and its ``_rstd`` form, ``rowsumsq_rstd``, ``pixelnorm_ada_silu``
wide and narrow, ``layernorm_affine``, ``qkv_norm_rope_pack``) and GroupNorm (``gn_stats`` / ``gn_finalize`` / ``gn_apply`` of
upsampler.hip) against the float64 truths of tests/norm_cases.py, under its three metrics: ``check`` on the whole tensor,
the same two figures per row (per sample and group for GroupNorm), and a per-element bound.  tests/test_norm_cases.py
pins on the CPU that an fp32 restatement of each operation meets all three on every case used here.

Every output is a view inside a larger buffer filled with a sentinel that must be intact afterwards (rows before and after,
the columns between D and the row stride).  Where the two kernels of one entry point add in the same order the test asks
for equal bits and says so: the narrow and the wide PixelNorm do not (8 values per lane + a short butterfly against
8 values per lane + the 64-lane butterfly give the same tree only at C = 512), so they are held to the three metrics;
the two paths of ``rowsumsq_rstd`` do not either ((v0 + v1) + (v2 + v3) per 16 bytes against a running sum per lane).

What these cases found on the library before the kernels changed (MI355X, 303 cases, 21 failed for a reason in the
library): the one-pass variance E[x^2] - mean^2 in fp32.
  norm_modulate Layer, D 2048: offset1024 rel L2 3.38e-2 (predicted 4.27e-2); offset256 passed ``check`` but had an element
  at 9.3 times its bound.  layernorm_affine, C 1024: offset1024 2.51e-2, offset256 an element at 26 times its bound.
  GroupNorm, 16 of 33 cases: offset1024 rel L2 1.5e-2 (S 105) to 2.4e+2 (S 70001, C 512: the variance clamps to 0 and
  rstd becomes eps^-1/2); offset256 3.1e-3 to 0.32; offset16 an element at 1.2 to 35 times its bound.
  GroupNorm was not run-to-run reproducible: three calls at S 70001, C 512 gave different bits, and so did the in-place
  call against the out-of-place one (float atomics, added in the order the blocks finish).
Everything else passed there: eps, every width and its refusal, strides, groups, tables, the pack layout, the narrow
PixelNorm kernel and its fallback, in-place row kernels.  The Layer kernels now take the variance about the mean from the
row in registers; GroupNorm sums shifted values into per-block partials that are added in block order."""
import pytest
import torch

import norm_cases as nc
from test_gpu_kernels import BF, DEV

pytestmark = pytest.mark.gpu

SENT = -12352.0                 # exactly representable in bf16
PAD = 2
UNSUPPORTED = -2
_FIG = {}


@pytest.fixture(scope="module", autouse=True)
def _report_closest_figures():
    yield
    print("\nclosest figures, as fractions of their limits: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_FIG.items())))


def _note(f):
    for k, v in f.items():
        if isinstance(v, float):
            _FIG[k] = max(_FIG.get(k, 0.0), v)


def guard(rows, D, ld=None, dtype=BF):
    """A [rows, D] view (row stride ld) inside a sentinel-filled buffer with PAD rows before and after."""
    ld = ld or D
    buf = torch.full((rows + 2 * PAD, ld), SENT, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + rows, :D]


def intact(buf, rows, D):
    b = buf.clone()
    b[PAD:PAD + rows, :D] = SENT
    return bool((b == SENT).all())


def _ops():
    from ltxmi import ops
    return ops


# ----------------------------------------------------------------------------------------------- one case of a row kernel
class RowCase:
    """Inputs on the host and the device, the float64 truth, and ``run(out)`` for one (operation, family, width)."""

    def __init__(self, op, family, D, rows, rpg=7, ldx=None, scale=True, silu=True, rope="shared", ld_tab=None):
        ops = _ops()
        self.op, self.D, self.rows = op, D, rows
        self.x = x = nc.make(family, rows, D)
        self.xbuf, self.xd = guard(rows, D, ldx)
        self.xd.copy_(x)
        if op in ("norm_modulate_rms", "norm_modulate_layer"):
            kind = op.rsplit("_", 1)[1]
            table, temb = nc.modulation((rows + rpg - 1) // rpg, D)
            td, ed = table.to(DEV), temb.to(DEV)                       # the tables are column slices of [groups, 6 D]
            self.truth, self.mag = nc.norm_modulate_op(x, kind, nc.EPS_DIT, table[1], nc.group_rows(temb[:, D:2 * D], rpg, rows),
                                                       table[0], nc.group_rows(temb[:, :D], rpg, rows))
            k = ops.NORM_LAYER if kind == "layer" else ops.NORM_RMS
            self.run = lambda out: ops.norm_modulate(self.xd, out, nc.EPS_DIT, k, td[1], ed[:, D:2 * D], td[0], ed[:, :D], rpg)
        elif op == "rmsnorm_rope":
            w = nc.bf(D, seed=9400, scale=0.1, offset=1.0)
            wd = w.to(DEV)
            if rope == "none":
                cos = sin = cd = sd = None
                period, ce, se = 0, None, None
            else:
                period = rows if rope == "per_row" else max(1, (rows * 2) // 5 if rows > 4 else rows)
                cos, sin = nc.rope_tables(period, D, ld_tab)
                idx = torch.arange(rows) % period
                ce, se = cos[idx], sin[idx]
                cd_full = torch.full((period, ld_tab or D), 3.0, dtype=BF, device=DEV)
                sd_full = torch.full((period, ld_tab or D), 3.0, dtype=BF, device=DEV)
                cd, sd = cd_full[:, :D], sd_full[:, :D]
                cd.copy_(cos)
                sd.copy_(sin)
            self.period, self.tables = period, (wd, cd, sd)
            self.truth, self.mag = nc.rmsnorm_rope_op(x, w, nc.EPS_QK, ce, se)

            def run(out):
                out.copy_(self.xd)
                return ops.rmsnorm_rope_(out, wd, nc.EPS_QK, cd, sd, period)
            self.run = run
        elif op == "pixelnorm":
            assert ldx is None
            g = torch.Generator().manual_seed(9500)
            sc, sh = torch.randn(1, D, generator=g) * 0.3, torch.randn(1, D, generator=g) * 0.3
            self.truth, self.mag = nc.pixelnorm_op(x, nc.EPS_PIXEL, sc.expand(rows, D) if scale else None,
                                                   sh.expand(rows, D) if scale else None, silu)
            scd, shd = (sc.to(DEV), sh.to(DEV)) if scale else (None, None)
            self.run = lambda out: ops.pixelnorm_ada_silu(self.xd.view(1, rows, D), scd, shd, silu, nc.EPS_PIXEL, out=out)
        elif op == "layernorm_affine":
            assert ldx is None
            gm, bt = nc.bf(D, seed=9600), nc.bf(D, seed=9601)
            self.truth, self.mag = nc.layernorm_affine_op(x, gm, bt, nc.EPS_DIT)
            gd, bd = gm.to(DEV), bt.to(DEV)
            self.run = lambda out: ops.layernorm_affine(self.xd, gd, bd, nc.EPS_DIT, out=out)
        else:
            raise KeyError(op)

    def verify(self, ldy=None, what=""):
        """Run into a guarded output, check the sentinels, the input and the three metrics; returns the bf16 output (CPU)."""
        strided = self.op in ("norm_modulate_rms", "norm_modulate_layer", "rmsnorm_rope")
        obuf, y = guard(self.rows, self.D, ldy if strided else None)
        self.run(y)
        torch.cuda.synchronize()
        assert intact(obuf, self.rows, self.D), f"{what}: wrote outside its rows / columns"
        assert intact(self.xbuf, self.rows, self.D) and torch.equal(self.xd.cpu(), self.x), f"{what}: the input changed"
        out = y.cpu()
        _note(nc.compare(out, self.truth, self.mag, what=what))
        return out


ROW_KERNELS = list(nc.ROW_OPS)
MODEL_WIDTHS = {"norm_modulate_rms": (2048,), "norm_modulate_layer": (2048,), "rmsnorm_rope": (2048,),
                "pixelnorm": (128, 1024), "layernorm_affine": (128, 1024)}
_FAMILY_CASES = [(op, fam, D) for op in ROW_KERNELS for D in MODEL_WIDTHS[op] for fam in nc.families_for(op, D)]
_WIDTH_CASES = [(op, fam, D) for op in ROW_KERNELS for D in nc.ROW_OPS[op] if D not in MODEL_WIDTHS[op]
                for fam in nc.families_for(op, D)]


@pytest.mark.parametrize("op,family,D", _FAMILY_CASES, ids=[f"{o}-{f}-{d}" for o, f, d in _FAMILY_CASES])
def test_every_row_kernel_on_every_family(op, family, D):
    """Model widths, the eps the models use, every input family (less those tests/norm_cases.py DROPPED lists)."""
    RowCase(op, family, D, nc.rows_for(D)).verify(what=f"{op} {family} D={D}")


@pytest.mark.parametrize("op,family,D", _WIDTH_CASES, ids=[f"{o}-{f}-{d}" for o, f, d in _WIDTH_CASES])
def test_every_row_kernel_at_every_width(op, family, D):
    """Both sides of 512 and 2048 (1, 4 or 16 chunks per lane), chunk counts that leave part of a wave idle (72, 1000,
    3000), one chunk (8) and the documented maximum (8192); rows = 4k + 1."""
    RowCase(op, family, D, nc.rows_for(D)).verify(what=f"{op} {family} D={D}")


@pytest.mark.parametrize("D", nc.REFUSED_WIDTHS)
def test_unsupported_widths_are_refused_and_write_nothing(D):
    from ltxmi import _lib
    ops, lib, rows = _ops(), _lib.lib, 5
    x = torch.ones(rows, 8208, dtype=BF, device=DEV)
    t = torch.ones(8, 3 * 8208, dtype=BF, device=DEV)
    f32 = torch.ones(8208, dtype=torch.float32, device=DEV)
    out = torch.full((rows * 3, 8208), SENT, dtype=BF, device=DEV)
    p, s = ops._ptr, ops._stream()
    ld = 8208
    codes = {
        "norm_modulate_rms": lib.ltxmi_norm_modulate_bf16(p(x), ld, p(out), ld, rows, D, 1e-6, 0, p(t), p(t), p(t), p(t), ld, 1, s),
        "norm_modulate_layer": lib.ltxmi_norm_modulate_bf16(p(x), ld, p(out), ld, rows, D, 1e-6, 1, p(t), p(t), p(t), p(t), ld, 1, s),
        "rmsnorm_rope": lib.ltxmi_rmsnorm_rope_bf16(p(out), ld, rows, D, p(t), 1e-5, p(t), p(t), ld, 1, s),
        "pixelnorm": lib.ltxmi_pixelnorm_ada_silu_bf16(p(x), p(out), rows, D, rows, p(f32), p(f32), 1, 1e-8, s),
        "layernorm_affine": lib.ltxmi_layernorm_affine_bf16(p(x), p(out), rows, D, p(t), p(t), 1e-6, s),
        "qkv_norm_rope_pack": lib.ltxmi_qkv_norm_rope_pack_bf16(p(t), 3 * ld, 1, rows, D, 1, p(t), p(t), 1e-5, None, None, 0, 0,
                                                                p(out), s),
    }
    torch.cuda.synchronize()
    assert codes == {k: UNSUPPORTED for k in codes}, codes
    assert bool((out == SENT).all())


# ------------------------------------------------------------------------------------------------- norm_modulate geometry
@pytest.mark.parametrize("kind", ["rms", "layer"])
@pytest.mark.parametrize("rows,rpg", [(1, 1), (2, 5), (3, 2), (222, 37), (222, 50), (222, 1), (222, 1000)])
def test_norm_modulate_rows_strides_and_groups(kind, rows, rpg):
    """Row counts 1, 2, 3 and 222; ldx != ldy != D; a last modulation group shorter than rows_per_group (222 = 4 x 50 + 22,
    3 = 2 + 1); rows_per_group 1 and larger than the row count; tables that are column slices of [groups, 6 D]."""
    D = 2048 if rows < 222 else 520
    c = RowCase(f"norm_modulate_{kind}", "row_scales", D, rows, rpg=rpg, ldx=D + 24)
    c.verify(ldy=D + 8, what=f"norm_modulate {kind} rows={rows} rpg={rpg}")


# --------------------------------------------------------------------------------------------------- rmsnorm_rope and rstd
@pytest.mark.parametrize("rope,ld_tab", [("none", None), ("shared", None), ("per_row", None), ("shared", 2048 + 64)])
def test_rmsnorm_rope_tables(rope, ld_tab):
    """No table, a shared table whose period does not divide the row count (101 rows, period 40), one table row per
    row, tables that are column slices (ld_tab > D)."""
    c = RowCase("rmsnorm_rope", "row_scales", 2048, 101, rope=rope, ld_tab=ld_tab)
    assert rope != "shared" or (c.period == 40 and 101 % c.period != 0)
    c.verify(ldy=2048 + 40, what=f"rmsnorm_rope {rope} ld_tab={ld_tab}")


def test_rmsnorm_rope_on_the_middle_third_of_a_packed_projection():
    ops, rows, D = _ops(), 45, 512
    buf = nc.make("plain", rows, 3 * D)
    w = nc.bf(D, seed=9400, scale=0.1, offset=1.0)
    cos, sin = nc.rope_tables(rows, D)
    d = buf.to(DEV).clone()
    ops.rmsnorm_rope_(d[:, D:2 * D], w.to(DEV), nc.EPS_QK, cos.to(DEV), sin.to(DEV), rows)
    truth, mag = nc.rmsnorm_rope_op(buf[:, D:2 * D], w, nc.EPS_QK, cos, sin)
    out = d.cpu()
    _note(nc.compare(out[:, D:2 * D], truth, mag, what="rmsnorm_rope middle third"))
    assert torch.equal(out[:, :D], buf[:, :D]) and torch.equal(out[:, 2 * D:], buf[:, 2 * D:])


def _sums(rows, blocks, ld, offset=0):
    """fp32 partial sums [rows, blocks] with row stride ld, optionally starting ``offset`` floats into their storage."""
    g = torch.Generator().manual_seed(9800 + blocks)
    ss = torch.rand(rows, blocks, generator=g) * 200 + 1
    store = torch.full((offset + rows * ld,), 1e30, dtype=torch.float32, device=DEV)
    view = store[offset:].view(rows, ld)[:, :blocks]
    view.copy_(ss)
    return ss, view


@pytest.mark.parametrize("blocks", [1, 3, 32, 33, 128])
def test_rmsnorm_rope_rstd_form(blocks):
    """The bf16 result is bit-equal to the plain form; the factor matches float64 to 1e-6 relative, ld > blocks."""
    ops = _ops()
    c = RowCase("rmsnorm_rope", "plain", 2048, 101)
    plain = c.verify(what="rmsnorm_rope plain form")
    ss, ssd = _sums(101, blocks, blocks + 5)
    fbuf, fac = guard(1, 101, dtype=torch.float32)
    obuf, y = guard(101, 2048)
    y.copy_(c.xd)
    wd, cd, sd = c.tables
    ops.rmsnorm_rope_(y, wd, nc.EPS_QK, cd, sd, c.period, rstd_of=(ssd, 64 * blocks, nc.EPS_QK, fac[0]))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), plain) and intact(obuf, 101, 2048) and intact(fbuf, 1, 101)
    want = nc.rstd_op(ss, 64 * blocks, nc.EPS_QK)
    assert float(((fac[0].cpu().double() - want) / want).abs().max()) <= 1e-6


def test_rowsumsq_rstd_both_paths():
    """The 16-byte path (blocks 32, ld 32) and the scalar path (blocks 30; ld 34; a base offset by one float) against float64
    to 1e-6.  The two paths do NOT add in the same order ((v0 + v1) + (v2 + v3) per 16 bytes against a running sum over
    j = part, part + 8, ...), so they are not asked for equal bits: both are held to the float64 factor."""
    ops = _ops()
    for blocks, ld, offset in [(32, 32, 0), (30, 32, 0), (32, 34, 0), (32, 32, 1), (128, 128, 0), (128, 130, 1)]:
        for rows in (1, 33, 257):
            ss, ssd = _sums(rows, blocks, ld, offset)
            assert (ssd.data_ptr() % 16 == 0) == (offset == 0)
            fbuf, fac = guard(1, rows, dtype=torch.float32)
            ops.rowsumsq_rstd(ssd, 64 * blocks, nc.EPS_QK, out=fac[0])
            torch.cuda.synchronize()
            want = nc.rstd_op(ss, 64 * blocks, nc.EPS_QK)
            assert intact(fbuf, 1, rows)
            assert float(((fac[0].cpu().double() - want) / want).abs().max()) <= 1e-6, (blocks, ld, offset, rows)


# ------------------------------------------------------------------------------------------------------ qkv_norm_rope_pack
@pytest.mark.parametrize("P", [1, 2, 8])
@pytest.mark.parametrize("D,rope", [(2048, True), (2048, False), (512, True), (512, False)])
def test_qkv_norm_rope_pack_layout_and_bits(P, D, rope):
    """q and k bit-equal to rmsnorm_rope_ on the same columns, v bit-equal to the input, every element of the send buffer
    written exactly once (the sentinel is gone everywhere inside and intact everywhere outside); B = 2, ld > 3 D."""
    ops, B, Nl = _ops(), 2, 21
    rows, ld = B * Nl, 3 * D + 16
    x = nc.make("row_scales", rows, 3 * D)
    xbuf, xd = guard(rows, 3 * D, ld)
    xd.copy_(x)
    wq, wk = nc.bf(D, seed=9401, scale=0.1, offset=1.0), nc.bf(D, seed=9402, scale=0.1, offset=1.0)
    cos, sin = nc.rope_tables(Nl, D, D + 8)
    cd, sd = (cos.to(DEV), sin.to(DEV)) if rope else (None, None)
    if rope:
        cfull = torch.zeros(Nl, D + 8, dtype=BF, device=DEV)
        sfull = torch.zeros(Nl, D + 8, dtype=BF, device=DEV)
        cfull[:, :D], sfull[:, :D] = cd, sd
        cd, sd = cfull[:, :D], sfull[:, :D]
    obuf, o = guard(1, rows * 3 * D)
    out = o[0].view(P, Nl, B, 3, D // P)
    ops.qkv_norm_rope_pack(xd, B, Nl, D, P, wq.to(DEV), wk.to(DEV), nc.EPS_QK, cd, sd, Nl if rope else 0, out=out)
    ref = xd.clone()
    ops.rmsnorm_rope_(ref[:, :D], wq.to(DEV), nc.EPS_QK, cd, sd, Nl)
    ops.rmsnorm_rope_(ref[:, D:2 * D], wk.to(DEV), nc.EPS_QK, cd, sd, Nl)
    torch.cuda.synchronize()
    assert intact(obuf, 1, rows * 3 * D) and intact(xbuf, rows, 3 * D) and torch.equal(xd.cpu(), x)
    r = ref.cpu()
    want = nc.pack_layout(r[:, :D], r[:, D:2 * D], x[:, 2 * D:], B, Nl, P)
    assert torch.equal(out.cpu(), want)
    idx = torch.arange(rows) % Nl
    for lo, w in ((0, wq), (D, wk)):                                        # and q, k against float64
        truth, mag = nc.rmsnorm_rope_op(x[:, lo:lo + D], w, nc.EPS_QK, cos[idx] if rope else None, sin[idx] if rope else None)
        _note(nc.compare(r[:, lo:lo + D], truth, mag, what=f"pack P={P} D={D} rope={rope} cols {lo}"))


# ------------------------------------------------------------------------------------------------------ pixelnorm_ada_silu
@pytest.mark.parametrize("scale", [True, False], ids=["ada", "noada"])
@pytest.mark.parametrize("silu", [True, False], ids=["silu", "nosilu"])
@pytest.mark.parametrize("C", nc.VAE_WIDTHS)
def test_pixelnorm_with_and_without_modulation_and_silu(C, scale, silu):
    RowCase("pixelnorm", "row_scales", C, 101, scale=scale, silu=silu).verify(what=f"pixelnorm C={C} ada={scale} silu={silu}")


def _pixelnorm_batched(C, B, rpb, family="plain", scale_offset=0, silu=True, inputs=None, per_row=True):
    """B samples of rpb rows through the wrapper; scale / shift optionally start ``scale_offset`` floats into their storage."""
    ops, rows = _ops(), B * rpb
    if inputs is None:
        g = torch.Generator().manual_seed(9500)
        inputs = nc.make(family, rows, C), torch.randn(B, C, generator=g) * 0.3, torch.randn(B, C, generator=g) * 0.3
    x, sc, sh = inputs
    truth, mag = nc.pixelnorm_op(x, nc.EPS_PIXEL, nc.group_rows(sc, rpb, rows), nc.group_rows(sh, rpb, rows), silu)
    scs = torch.zeros(scale_offset + B * C, dtype=torch.float32, device=DEV)
    shs = torch.zeros(scale_offset + B * C, dtype=torch.float32, device=DEV)
    scd, shd = scs[scale_offset:].view(B, C), shs[scale_offset:].view(B, C)
    scd.copy_(sc)
    shd.copy_(sh)
    assert (scd.data_ptr() % 16 == 0) == (scale_offset == 0)
    obuf, y = guard(rows, C)
    ops.pixelnorm_ada_silu(x.to(DEV).view(B, rpb, C), scd, shd, silu, nc.EPS_PIXEL, out=y)
    torch.cuda.synchronize()
    assert intact(obuf, rows, C)
    out = y.cpu()
    _note(nc.compare(out, truth, mag, what=f"pixelnorm C={C} B={B} rpb={rpb} offset={scale_offset}", per_row=per_row))
    return out


@pytest.mark.parametrize("C", [64, 128, 256])
def test_pixelnorm_narrow_kernel_second_trip_of_the_grid_stride_loop(C):
    """4096 workgroups x 4 waves x (512 / C) rows per wave, plus 5: the loop makes a second trip and ends ragged.  At C = 64
    the per-row figures are not asserted (nc.NARROW_TRIP: the fp32 restatement itself is at 1.06 of the per-row L2 limit
    over 131077 rows of 64 values); the whole-tensor and the per-element metrics are."""
    inputs = nc.narrow_trip_inputs(C)
    _pixelnorm_batched(C, 1, inputs[0].shape[0], inputs=inputs, per_row=nc.NARROW_TRIP[C])


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_pixelnorm_a_wave_spans_two_samples(C):
    """B = 3 with 13 rows per sample: not a multiple of the 8 / 4 / 2 rows a wave of the narrow kernel holds."""
    _pixelnorm_batched(C, 3, 13, family="row_scales")


@pytest.mark.parametrize("C", [64, 128, 256])
def test_pixelnorm_unaligned_scale_takes_the_wide_kernel(C):
    """scale / shift offset by one float are not 16-byte aligned: the entry point falls back to the row-per-wave kernel.
    The two kernels add the squares in different trees (the narrow one: 8 per lane, then 3 to 5 butterfly steps inside
    the row's lanes; the wide one: the 64-lane butterfly with idle lanes contributing zeros -- the same tree in exact
    arithmetic, but the compiler is free to contract either differently), so both are held to the three metrics
    and additionally may differ from each other by at most one bf16 step per element."""
    a = _pixelnorm_batched(C, 3, 13, family="row_scales", scale_offset=0)
    b = _pixelnorm_batched(C, 3, 13, family="row_scales", scale_offset=1)
    diff = (a.double() - b.double()).abs()
    assert bool((diff <= 2.0 ** -7 * a.double().abs() + 1e-30).all())


# --------------------------------------------------------------------------------------------------------------- GroupNorm
def _groupnorm(family, samples, S, C, groups, with_res, in_place=False):
    ops = _ops()
    x, gamma, beta, res = nc.gn_inputs(family, samples, S, C, with_res)
    truth, mag = nc.groupnorm_silu_op(x, groups, gamma, beta, nc.EPS_GN, res)
    xd = x.to(DEV)
    obuf, y = guard(samples * S, C)
    out = y.view(samples, S, C)
    ops.groupnorm_silu(xd, gamma.to(DEV), beta.to(DEV), groups, nc.EPS_GN, residual=None if res is None else res.to(DEV),
                       samples=samples, out=out)
    torch.cuda.synchronize()
    assert intact(obuf, samples * S, C) and torch.equal(xd.cpu(), x)
    o = out.cpu()
    _note(nc.compare(nc.group_view(o, groups), nc.group_view(truth, groups), nc.group_view(mag, groups),
                     what=f"groupnorm {family} samples={samples} S={S} C={C} groups={groups} res={with_res}"))
    return o


_GN = [(fam, case) for case in nc.GN_CASES for fam in nc.gn_families(case)]


@pytest.mark.parametrize("family,case", _GN, ids=[f"{f}-" + "x".join(map(str, c)) for f, c in _GN])
def test_groupnorm_geometry_and_families(family, case):
    """S below the rows per iteration, ragged last blocks, samples > 2048, more than 2048 x 256 chunks (70001 x 64 slots),
    C = 8 (one slot), one channel per group (the two halves of a packed pair in different groups), one group."""
    _groupnorm(family, *case)


# ---------------------------------------------------------------------------------------------------------------- in place
@pytest.mark.parametrize("op,D", [("pixelnorm", 128), ("pixelnorm", 1024), ("layernorm_affine", 128), ("layernorm_affine", 4096),
                                  ("norm_modulate_rms", 2048), ("norm_modulate_layer", 4096)])
def test_row_kernels_in_place_equal_out_of_place(op, D):
    """out = the input (autoencoder.py passes PixelNorm its own input): every 16-byte chunk is read and written by the same
    lane and the read is in registers before the write, so the result must be bit-equal to the out-of-place call."""
    c = RowCase(op, "row_scales", D, 1001)
    want = c.verify(what=f"{op} out of place")
    c.run(c.xd)
    torch.cuda.synchronize()
    assert torch.equal(c.xd.cpu(), want) and intact(c.xbuf, c.rows, D)


@pytest.mark.parametrize("case", [(3, 105, 64, 32, True), (1, 4097, 512, 32, False)])
def test_groupnorm_in_place_equals_out_of_place(case):
    """latent_upsampler.py passes out = x: the statistics passes finish before the apply pass starts (stream order), and the
    apply pass reads and writes each chunk in the same thread."""
    ops = _ops()
    samples, S, C, groups, with_res = case
    want = _groupnorm("plain", *case)
    x, gamma, beta, res = nc.gn_inputs("plain", samples, S, C, with_res)
    xbuf, xd = guard(samples * S, C)
    xd.copy_(x.view(-1, C))
    xv = xd.view(samples, S, C)
    ops.groupnorm_silu(xv, gamma.to(DEV), beta.to(DEV), groups, nc.EPS_GN, residual=None if res is None else res.to(DEV),
                       samples=samples, out=xv)
    torch.cuda.synchronize()
    assert torch.equal(xv.cpu(), want) and intact(xbuf, samples * S, C)


# -------------------------------------------------------------------------------------------------------- same bits twice
@pytest.mark.parametrize("op,D", [(op, D) for op in ROW_KERNELS for D in (MODEL_WIDTHS[op][-1], 8192)])
def test_row_kernels_give_the_same_bits_three_times(op, D):
    c = RowCase(op, "plain", D, 1001)
    outs = []
    for _ in range(3):
        obuf, y = guard(c.rows, D)
        c.run(y)
        outs.append(y)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_groupnorm_gives_the_same_bits_three_times():
    """S = 70001, C = 512: 2048 blocks add into each channel.  (Passing does not prove the order is fixed; that the block
    partials are added in block order is decided in upsampler.hip, this only watches it.)"""
    ops = _ops()
    x, gamma, beta, _ = nc.gn_inputs("plain", 1, 70001, 512, False)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    outs = [ops.groupnorm_silu(xd, gd, bd, 32, nc.EPS_GN, samples=1) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_pack_and_rstd_give_the_same_bits_three_times():
    ops, B, Nl, D, P = _ops(), 2, 333, 2048, 8
    xd = nc.make("plain", B * Nl, 3 * D).to(DEV)
    w = nc.bf(D, seed=9401, scale=0.1, offset=1.0).to(DEV)
    cos, sin = (t.to(DEV) for t in nc.rope_tables(Nl, D))
    outs = [ops.qkv_norm_rope_pack(xd, B, Nl, D, P, w, w, nc.EPS_QK, cos, sin, Nl) for _ in range(3)]
    ss, ssd = _sums(1001, 32, 32)
    facs = [ops.rowsumsq_rstd(ssd, 2048, nc.EPS_QK) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(facs[0], facs[1]) and torch.equal(facs[0], facs[2])
