"""The pointwise, layout and step-math kernels on a real MI355X at their edges.

csrc/pointwise.hip (``silu``, ``add``, ``stg_blend_``, ``ncdhw_to_ndhwc``, ``ndhwc_to_ncdhw``, ``unpatchify_to_ncdhw`` with
both of its kernels, ``patchify_to_ndhwc``, ``space_to_depth_skip``, ``guidance_step_`` plain and masked,
``image_cond_noise_``) and the tail of csrc/upsampler.hip (``pixel_shuffle2d``, ``tile_blend_``, ``adain_filter``) against the
float64 truths of tests/pointwise_cases.py: pure copies with ``torch.equal``, arithmetic under ``check`` on the whole
tensor and a per-element bound whose slack the CPU measures (tests/test_pointwise_cases.py pins that an fp32 restatement
meets both on every case used here).  Every geometry list there holds one case whose work items exceed the grid cap of
its launch, so the second trip of every grid-stride loop runs, with a ragged end; the others are the smallest shapes that
reach each branch.

The guidance scalars alpha and factor are not outputs of the kernel: ``_scalars`` recovers them from a call with fp32
latents = 0 and dt = -1, which returns factor (alpha a + c) per element, by least squares over all elements
(``pointwise_cases.recover_scalars``), and holds each to its float64 value within 2^-9.

Which test fails without which fix of this change:
  ops.silu / ops.add / ops.unpatchify_to_ncdhw refusing views     test_wrappers_refuse_views_they_would_misread
  ltxmi_silu_bf16 / ltxmi_add_bf16 / ltxmi_stg_blend_bf16 refusing pointers that are not 16-byte aligned
                                                                   test_misaligned_pointers_are_refused_and_write_nothing
  the rescale's deviations taken about the data                   test_guidance_step[257-1], [65539-0], [638976-1] and 7 more
  tile_blend's two weights each rounded once                      test_tile_blend_weights_are_each_rounded_once

What these cases found on the library before it changed (MI355X, 183 cases, 10 failed):
  * guidance_step_ took the two standard deviations of the rescale from one-pass sums, (sum x^2 - (sum x)^2 / n) / (n - 1) in
    fp32.  On the offset family (mean 4, deviation 0.5) the factor stayed within 0.004 of its 2^-9 allowance, but the
    fp32 latents missed the per-element bound in every setting that rescales: an element at 1.06 of the bound at n = 257,
    2.25 at n = 65539, 5.45 at n = 4992 x 128 (the factor off by 3e-6).  The bf16 latents passed.  The kernel now sums
    (text - mean)^2 about pass 1's mean and the guided prediction about the guidance formula applied to that mean; no
    atomics, the partials are still added in block order.  After the change the worst fp32 element is at 0.37 of the bound,
    and the latents of tests/test_gpu_kernels.py::test_guidance_step and ::test_guidance_step_with_conditioning_mask
    are bit for bit what the former kernel gave, fp32 and bf16 (compared with the former library on the same machine).
  * tile_blend formed the weight of ``a`` as 1.0f - fp32(z / extent), carrying the rounding of z / extent into a weight that
    is small at the end of the band (1e-6 of it at extent 33), where the reference rounds 1 - z / extent once.  Found by
    the CPU measurement of the slack; the kernel now divides (extent - z) by extent.  Bits change only where z / extent
    is inexact (not at the power-of-two extents of the product's tilings), by one rounding of the output.
  * ops.silu, ops.add and ops.unpatchify_to_ncdhw computed on the wrong memory for transposed or sliced inputs and a strided
    ``out=``, and the three 16-byte kernels took any pointer (both by reading; never launched that way).  They now refuse.
  * Everything else passed: every second trip of a grid-stride loop with its ragged end, the generic unpatchify kernel, both
    threshold decisions, alpha and factor (at most 0.001 and 0.002 of 2^-9), n = 2 ... 4992 x 128, used workspaces,
    in-place calls, guards, three-fold repeatability.
Worst per-element figure seen per kernel, as a fraction of its bound (printed at the end of a ``-s`` run): 0.498 for every
bf16 output (silu, add, stg_blend, both normalising passes, s2d_skip, tile_blend, guidance, masked guidance, cond_noise;
adain 0.497), which is the rounding itself; fp32 outputs: guidance 0.365, masked guidance 0.329, adain 0.456, cond_noise
0.105, tile_blend 0.137."""
import ctypes

import pytest
import torch

import pointwise_cases as pc
from test_gpu_kernels import BF, DEV

pytestmark = pytest.mark.gpu

SENT = -12352.0                 # exactly representable in bf16
PAD = 16                        # guard elements (a multiple of 8: the view stays 16-byte aligned)
UNSUPPORTED = -2
F32 = torch.float32
_FIG = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_figures():
    yield
    print("\nworst per-element figures, as fractions of the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_FIG.items())))


def _ops():
    from ltxmi import ops
    return ops


def _compare(kernel, out, truth, mag, what):
    fig = pc.compare(out.detach().cpu(), truth, mag, what=what)
    _FIG[kernel] = max(_FIG.get(kernel, 0.0), fig)
    return fig


def guarded(shape, dtype=BF):
    """A contiguous view of ``shape`` inside a sentinel-filled 1-D buffer with PAD guard elements before and after."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def guards_intact(buf):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all())


def same_bits_three_times(run):
    """run() -> a fresh result tensor; three calls give the same bits."""
    first = run().clone()
    return all(torch.equal(first, run()) for _ in range(2))


def _cases(*ops_):
    return [c for c in pc.ARITH_CASES if c[0] in ops_]


def _ids(cases):
    return [f"{c[0]}-{c[1]}-{c[2]}".replace(" ", "") for c in cases]


# ------------------------------------------------------------------------------------------------ silu, add
@pytest.mark.parametrize("op,family,n", _cases("silu", "add"), ids=_ids(_cases("silu", "add")))
def test_silu_and_add(op, family, n):
    """n = 8 and n = 8 (2048 x 256 + 5): the second trip of the grid-stride loop holds 5 chunks.  ``out=`` is a view inside a
    sentinel buffer whose guards stay intact; in place gives the bits of out of place; the large family's values below
    -90 give -0, not NaN (``compare`` asserts finiteness and the dead elements)."""
    ops = _ops()
    fn, args, _, _ = pc.arith_truth(op, family, n)
    truth, mag = fn(*args)
    d = [a.to(DEV) for a in args]
    call = ops.silu if op == "silu" else ops.add
    buf, view = guarded((1, n))
    out = call(*d, out=view)
    assert out.data_ptr() == view.data_ptr()
    _compare(op, out, truth, mag, f"{op} {family} n={n}")
    assert guards_intact(buf)
    assert torch.equal(call(*d), out)
    for k in range(len(d)):                                    # in place in each operand
        e = [a.clone() for a in d]
        assert torch.equal(call(*e, out=e[k]), out), f"{op} in place in operand {k}"
    if family == "large" and op == "silu":
        x = args[0].float()
        assert bool((out.cpu().float()[x < -90] == 0).all())
    if n == pc.SILU_SIZES[-1] and family == "plain":
        assert same_bits_three_times(lambda: call(*d))


# ------------------------------------------------------------------------------------------------ stg_blend
@pytest.mark.parametrize("family,geom", [c[1:] for c in _cases("stg_blend")], ids=_ids(_cases("stg_blend")))
def test_stg_blend(family, geom):
    """m in {1, 0, 0.25} (the sample with m = 1 is bit-identical); lda != ldv != D with the pad columns of both buffers
    intact; D = 8 and D = 2048; B L D / 8 past 524288; v as the middle column block of a packed [rows, 3 D] buffer.  The
    wrapper takes rows that are contiguous over (B, L) only, so the cases with lda != D go through the C entry point."""
    from ltxmi import _lib
    ops = _ops()
    B, L, D, lda, ldv = geom
    abuf, vbuf, off, m = pc.stg_inputs(family, geom)
    truth, mag = pc.stg_blend_op(abuf[..., :D], vbuf[..., off:off + D], m)
    vd, md = vbuf.to(DEV), m.to(DEV)

    def run():
        ad = abuf.to(DEV)
        if lda == D:
            ops.stg_blend_(ad, vd[..., off:off + D], md)
        else:
            _lib.check(_lib.lib.ltxmi_stg_blend_bf16(ops._ptr(ad), lda, ops._ptr(vd[..., off:off + D]), ldv, ops._ptr(md), B, L, D,
                                                    ops._stream()), "ltxmi_stg_blend_bf16")
        return ad
    ad = run()
    _compare("stg_blend", ad[..., :D], truth, mag, f"stg_blend {family} {geom}")
    assert torch.equal(ad[0].cpu(), abuf[0]), "the sample with m = 1 must be bit-identical"
    assert torch.equal(ad[..., D:].cpu(), abuf[..., D:]) and torch.equal(vd.cpu(), vbuf)
    if geom == pc.STG_GEOMS[-1]:
        assert same_bits_three_times(run)


# ------------------------------------------------------------------------------------------------ layout passes
@pytest.mark.parametrize("shape", pc.LAYOUT_SHAPES, ids=str)
def test_layout_copies_are_bit_exact(shape):
    """ncdhw_to_ndhwc and ndhwc_to_ncdhw without std / mean: C in {1, 16, 128}, a total past 524288 with odd T H W, and for
    the second ldx > c0 + C with c0 > 0."""
    ops = _ops()
    z, x, _, _ = pc.layout_inputs("plain", shape)
    assert torch.equal(ops.ncdhw_to_ndhwc(z.to(DEV)).cpu(), pc.to_ndhwc(z))
    c0, C = pc.NORMALISE_PAD[0], shape[1]
    assert x.shape[-1] > c0 + C and c0 > 0
    assert torch.equal(ops.ndhwc_to_ncdhw(x.to(DEV), c0, C).cpu(), pc.to_ncdhw(x[..., c0:c0 + C]))


_LAYOUT = _cases("unnormalise", "normalise")


@pytest.mark.parametrize("op,family,shape", _LAYOUT, ids=_ids(_LAYOUT))
def test_layout_passes_with_statistics(op, family, shape):
    ops = _ops()
    z, x, std, mean = pc.layout_inputs(family, shape)
    if op == "unnormalise":
        truth, mag = pc.unnormalise_op(z, std, mean)
        run = lambda: ops.ncdhw_to_ndhwc(z.to(DEV), std.to(DEV), mean.to(DEV))
    else:
        truth, mag = pc.normalise_op(x, pc.NORMALISE_PAD[0], shape[1], std, mean)
        run = lambda: ops.ndhwc_to_ncdhw(x.to(DEV), pc.NORMALISE_PAD[0], shape[1], std.to(DEV), mean.to(DEV))
    _compare(op, run(), truth, mag, f"{op} {family} {shape}")
    if shape == pc.LAYOUT_SHAPES[-1]:
        assert same_bits_three_times(run)


@pytest.mark.parametrize("geom", pc.UNPATCHIFY_GEOMS, ids=str)
def test_unpatchify_both_kernels(geom):
    """The patch-4 kernel past 524288 positions; the generic kernel at patch 2, at C_out 4 with patch 4 and at patch 1 past
    524288 outputs, and on the patch-4 kernel's shape through an input 8 bytes off a 16-byte boundary (legal for the
    scalar kernel, which the entry point then selects): the same bits as the patch-4 kernel."""
    ops = _ops()
    B, T, H, W, Co, p, off = geom
    shape = (B, T, H, W, Co * p * p)
    x = pc.make_like("plain", shape, seed=101)
    want = pc.unpatchify_ref(x, p)
    n = x.numel()
    buf = torch.empty(n + 8, dtype=BF, device=DEV)
    xd = buf[off:off + n].view(shape)
    xd.copy_(x)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == (2 * off) % 16
    out = ops.unpatchify_to_ncdhw(xd, Co, p)
    assert torch.equal(out.cpu(), want)
    if off:
        assert torch.equal(out, ops.unpatchify_to_ncdhw(x.to(DEV), Co, p))


@pytest.mark.parametrize("geom", pc.PATCHIFY_GEOMS, ids=str)
def test_patchify(geom):
    """patch 4 with C_pad 64 and patch 1 with C_pad = C, totals past 524288; the padded channels are exactly zero."""
    ops = _ops()
    B, C, T, H, W, p, cpad = geom
    x = pc.to_ncdhw(pc.make_like("plain", (B, T, H, W, C), seed=102))
    out = ops.patchify_to_ndhwc(x.to(DEV), p, cpad).cpu()
    want = pc.patchify_ref(x, p, cpad)
    assert torch.equal(out, want)
    assert not out[..., C * p * p:].any()


_S2D = _cases("s2d_skip")


@pytest.mark.parametrize("family,geom", [c[1:] for c in _S2D], ids=_ids(_S2D))
def test_space_to_depth_skip(family, geom):
    """The three strides, group in {1, 2, 4}, T odd where the time stride is 2 (the duplicated first frame), T = 1, and a
    total past 524288."""
    ops = _ops()
    conv, x = pc.s2d_inputs(family, geom)
    truth, mag = pc.s2d_skip_op(conv, x, (geom[0], geom[1]), geom[2])
    cd, xd = conv.to(DEV), x.to(DEV)
    run = lambda: ops.space_to_depth_skip(cd, xd, (geom[0], geom[1], geom[1]))
    _compare("s2d_skip", run(), truth, mag, f"space_to_depth_skip {family} {geom}")
    if geom == pc.S2D_GEOMS[-1]:
        assert same_bits_three_times(run)


@pytest.mark.parametrize("C", [8, 64])
def test_pixel_shuffle2d_past_the_cap(C):
    """C = 8 with 4 frames H W chunks past the 2048-block cap; a second width for the chunk index."""
    ops = _ops()
    B, T, H, W, _ = pc.PIXEL_SHUFFLE_SHAPE
    shape = (B, T, H, W, 4 * C) if C == 8 else (2, 1, 7, 5, 4 * C)
    x = pc.make_like("plain", shape, seed=103)
    assert torch.equal(ops.pixel_shuffle2d(x.to(DEV)).cpu(), pc.pixel_shuffle2d_ref(x))


# ------------------------------------------------------------------------------------------------ guidance step
def _guidance_call(ops, npred_d, lat_d, dt, setting, ws, **kw):
    gs, stg, rs, do_cfg, do_stg, do_res = setting
    return ops.guidance_step_(npred_d, lat_d, dt, gs, stg, rs, do_cfg, do_stg, do_res, ws, **kw)


def _scalars(ops, npred, setting, ws):
    """(alpha or None, factor) of the kernel, from a probe call with fp32 latents 0 and dt -1 (module docstring)."""
    gs, stg, _, do_cfg, do_stg, _ = setting
    o = torch.zeros(1, npred.shape[1], npred.shape[2], dtype=F32, device=DEV)
    _guidance_call(ops, npred.to(DEV), o, -1.0, setting, ws)
    return pc.recover_scalars(o, npred, gs, stg, do_cfg, do_stg)


@pytest.mark.parametrize("k", range(len(pc.GUIDANCE_SETTINGS)))
@pytest.mark.parametrize("n", pc.GUIDANCE_N)
def test_guidance_step(n, k):
    """n in {2, 255, 256, 257, one past the 256-block cap + 2, 4992 x 128} x the four settings of test_guidance_step plus
    guidance scale exactly 1.0 and 0.0 with do_cfg set x fp32 and bf16 latents x the plain and offset families: the two
    metrics, alpha and factor within 2^-9 of float64, and a workspace that held the partials of a call of another n gives
    the bits of a fresh one (filled with NaN: nothing stale, and nothing unwritten, is read)."""
    ops = _ops()
    setting = pc.GUIDANCE_SETTINGS[k]
    gs, stg, rs, do_cfg, do_stg, do_res = setting
    used = torch.empty(ops.GUIDANCE_WORKSPACE_FLOATS, device=DEV)
    other_n = 1000 if n != 1000 else 999
    for family in ("plain", "offset"):
        npred = pc.guidance_npred(family, n, do_cfg, do_stg)
        nd = npred.to(DEV)
        _, alpha, factor, _ = pc.guidance_parts(npred, *setting)
        a, f = _scalars(ops, npred, setting, used)
        assert abs(f / float(factor) - 1) <= pc.SCALAR_TOL, f"factor {f} against {float(factor)} ({family}, n={n})"
        if a is not None:
            assert abs(a / float(alpha) - 1) <= pc.SCALAR_TOL, f"alpha {a} against {float(alpha)} ({family}, n={n})"
        _FIG["guidance factor / 2^-9"] = max(_FIG.get("guidance factor / 2^-9", 0.0), abs(f / float(factor) - 1) / pc.SCALAR_TOL)
        if a is not None:
            _FIG["guidance alpha / 2^-9"] = max(_FIG.get("guidance alpha / 2^-9", 0.0), abs(a / float(alpha) - 1) / pc.SCALAR_TOL)
        for lt in (F32, BF):
            _, lat = pc.guidance_inputs(family, n, 3, lt)
            truth, mag = pc.guidance_step_op(npred, lat, pc.GUIDANCE_DT, *setting)
            # a call of another size first, into the same workspace
            _guidance_call(ops, pc.guidance_npred("plain", other_n, do_cfg, do_stg).to(DEV),
                           torch.zeros(1, other_n, 1, dtype=lt, device=DEV), 0.1, setting, used)
            d = lat.to(DEV).clone()
            _guidance_call(ops, nd, d, pc.GUIDANCE_DT, setting, used)
            _compare("guidance_" + ("f32" if lt == F32 else "bf16"), d.reshape(truth.shape), truth, mag,
                     f"guidance {family} n={n} setting {k} {lt}")
            fresh = torch.full((ops.GUIDANCE_WORKSPACE_FLOATS,), float("nan"), device=DEV)
            e = lat.to(DEV).clone()
            _guidance_call(ops, nd, e, pc.GUIDANCE_DT, setting, fresh)
            assert torch.equal(d, e), "a used workspace and a fresh one give different bits"
            if do_cfg and gs in (0.0, 1.0):                    # the branch that returns text: the bits of the call without cfg
                e = lat.to(DEV).clone()
                ops.guidance_step_(nd[1:].contiguous(), e, pc.GUIDANCE_DT, 0.0, stg, rs, False, do_stg, do_res, fresh)
                assert torch.equal(d, e)
            if n == pc.GUIDANCE_N[-1] and family == "plain":
                def run():
                    r = lat.to(DEV).clone()
                    _guidance_call(ops, nd, r, pc.GUIDANCE_DT, setting, used)
                    return r
                assert same_bits_three_times(run)


@pytest.mark.parametrize("lat_dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("tokens,channels", pc.MASKED_GEOMS)
def test_masked_guidance_step_at_the_threshold(tokens, channels, lat_dtype):
    """Masks for which 1 - mask is fp32(t - 1e-6), its two neighbours and t (pointwise_cases: THRESHOLDS), at a timestep on
    which the float64 oracle decides otherwise than the float32 one: the tokens the float32 oracle freezes are
    bit-identical to their input, the others meet the per-element bound.  channels in {1, 128}, tokens x channels past
    524288."""
    ops = _ops()
    tsch, i, masks4 = pc.guidance_threshold_case()
    t = tsch[i]
    dt = float(t - tsch[i + 1])
    mask = pc.threshold_mask(masks4, tokens)
    moves = pc.oracle_moves(tsch, t, mask)[0]
    assert moves[:4].tolist() == [False, False, True, True] and 0 < int(moves.sum()) < tokens
    setting = pc.GUIDANCE_SETTINGS[0]
    n = tokens * channels
    npred, lat = pc.guidance_inputs("plain", n, 3, lat_dtype)
    npred, lat = npred.reshape(3, tokens, channels), lat.reshape(1, tokens, channels)
    truth, mag = pc.guidance_step_op(npred, lat, dt, *setting)
    truth, mag = truth.reshape(tokens, channels), mag.reshape(tokens, channels)
    ws = torch.empty(ops.GUIDANCE_WORKSPACE_FLOATS, device=DEV)
    nd, md = npred.to(DEV), mask.to(DEV)

    def run():
        d = lat.to(DEV).clone()
        _guidance_call(ops, nd, d, dt, setting, ws, cond_mask=md, t=float(t))
        return d
    out = run().cpu()[0]
    assert torch.equal(out[~moves], lat[0][~moves]), "a token the float32 reference freezes has moved"
    _compare("guidance_masked_" + ("f32" if lat_dtype == F32 else "bf16"), out[moves], truth[moves], mag[moves],
             f"masked guidance {tokens}x{channels} {lat_dtype}")
    if tokens == pc.MASKED_GEOMS[-1][0]:
        assert same_bits_three_times(run)


_COND = _cases("cond_noise_f32", "cond_noise_bf16")


@pytest.mark.parametrize("op,family,geom", _COND, ids=_ids(_COND))
def test_image_cond_noise_at_the_threshold(op, family, geom):
    """Masks 1 - 1e-6 as fp32 evaluates it, its two neighbours and exactly 1.0: the tokens the float32 oracle does not reset
    are bit-identical to their input (the mask equal to the threshold among them), the others meet the bound."""
    ops = _ops()
    fn, args, kw, lt = pc.arith_truth(op, family, geom)
    lat, init, noise, mask, scale, t = args
    need = kw["need"][0]
    assert need[:4].tolist() == [False, False, True, True]
    truth, mag = fn(*args, **kw)
    idev, ndev, mdev = init.to(DEV), noise.to(DEV), mask.to(DEV)

    def run():
        d = lat.to(DEV).clone()
        ops.image_cond_noise_(d, idev, ndev, mdev, scale, t)
        return d
    out = run().cpu()
    assert torch.equal(out[0][~need], lat[0][~need]), "a token the float32 reference leaves alone was reset"
    _compare(op, out[0][need], truth[0][need], mag[0][need], f"{op} {family} {geom}")
    assert torch.equal(idev.cpu(), init) and torch.equal(ndev.cpu(), noise)
    if geom == pc.MASKED_GEOMS[-1]:
        assert same_bits_three_times(run)


# ------------------------------------------------------------------------------------------------ tile_blend, adain
@pytest.mark.parametrize("geom", pc.TILE_GEOMS, ids=str)
def test_tile_blend(geom):
    """extent = 1, an extent inside both lengths, and extent = the whole length with the band past 65535 blocks (bf16):
    the band under the two metrics, every element of b outside it and all of a bit-identical."""
    ops = _ops()
    sa, lb, dim, extent = geom
    a, b = pc.tile_inputs(geom)
    truth, mag = pc.tile_blend_op(a, b, extent, dim)
    ad = a.to(DEV)

    def run():
        bd = b.to(DEV)
        out = ops.tile_blend_(ad, bd, extent, dim)
        assert out.data_ptr() == bd.data_ptr()
        return out
    out = run().cpu()
    _compare("tile_blend", out, truth, mag, f"tile_blend {geom}")
    assert torch.equal(out.narrow(dim, extent, lb - extent), b.narrow(dim, extent, lb - extent))
    assert torch.equal(ad.cpu(), a)
    if geom == pc.TILE_GEOMS[-1]:
        assert same_bits_three_times(run)


def test_tile_blend_weights_are_each_rounded_once():
    """fp32, b = 0, extent 33: the output is a (1 - z / 33) alone, held to SLACK mag.  The weight formed as 1 - fp32(z / 33)
    misses it (tests/test_pointwise_cases.py shows by how much)."""
    ops = _ops()
    a, b = pc.tile_weight_inputs()
    truth, mag = pc.tile_blend_op(a, b, 33, 2)
    out = ops.tile_blend_(a.to(DEV), b.to(DEV), 33, 2)
    _compare("tile_blend_f32", out, truth, mag, "tile_blend fp32 weights")


_ADAIN = _cases("adain_f32", "adain_bf16")


@pytest.mark.parametrize("op,family,geom", _ADAIN, ids=_ids(_ADAIN))
def test_adain_filter(op, family, geom):
    """Every family (offset: planes around 100 with a spread of half a bf16 step, which two-pass statistics must pass),
    n != n_ref, n = 2, factor in {0, 1, 0.25}; factor 0 returns the input's bits for fp32."""
    ops = _ops()
    fn, (x, r, factor), _, lt = pc.arith_truth(op, family, geom)
    truth, mag = fn(x, r, factor)
    xd, rd = x.to(DEV), r.to(DEV)
    run = lambda: ops.adain_filter(xd, rd, factor)
    out = run()
    assert out.dtype == lt
    _compare(op, out, truth, mag, f"{op} {family} {geom}")
    if factor == 0.0 and lt == F32:
        assert torch.equal(out.cpu(), x)
    if geom[0] is pc.ADAIN_GEOMS[0] and family == "plain":
        assert same_bits_three_times(run)


# ------------------------------------------------------------------------------------------------ refusals
def test_wrappers_refuse_views_they_would_misread():
    """ops.silu, ops.add (inputs and out) and ops.unpatchify_to_ncdhw hand data_ptr() and numel() to kernels that assume a
    dense buffer: a transposed input, a sliced input and a strided ``out=`` raise ValueError, as their neighbours do."""
    ops = _ops()
    x = torch.ones(16, 32, dtype=BF, device=DEV)
    y = torch.ones(16, 32, dtype=BF, device=DEV)
    wide = torch.ones(16, 64, dtype=BF, device=DEV)
    tall = torch.ones(32, 16, dtype=BF, device=DEV)
    for bad in (tall.t(), wide[:, :32], wide[:, ::2]):
        assert bad.shape == x.shape and not bad.is_contiguous()
        with pytest.raises(ValueError):
            ops.silu(bad)
        with pytest.raises(ValueError):
            ops.silu(x, out=bad)
        with pytest.raises(ValueError):
            ops.add(bad, y)
        with pytest.raises(ValueError):
            ops.add(x, bad)
        with pytest.raises(ValueError):
            ops.add(x, y, out=bad)
    with pytest.raises(ValueError):
        ops.add(x, y[:8])
    with pytest.raises(ValueError):
        ops.silu(x, out=torch.ones(8, 32, dtype=BF, device=DEV))
    assert bool((wide == 1).all()) and bool((tall == 1).all())
    p = torch.ones(1, 2, 3, 5, 96, dtype=BF, device=DEV)
    with pytest.raises(ValueError):
        ops.unpatchify_to_ncdhw(p[..., :48], 3, 4)
    with pytest.raises(ValueError):
        ops.unpatchify_to_ncdhw(p.transpose(2, 3)[..., :48], 3, 4)
    with pytest.raises(ValueError):
        ops.unpatchify_to_ncdhw(p, 3, 4)                       # 96 channels are not 3 x 4 x 4
    torch.cuda.synchronize()


@pytest.mark.parametrize("shift", [2, 8])
def test_misaligned_pointers_are_refused_and_write_nothing(shift):
    """ltxmi_silu_bf16, ltxmi_add_bf16 and ltxmi_stg_blend_bf16 move 16-byte words: a pointer ``shift`` bytes off a 16-byte
    boundary, in any position, is LTXMI_ERR_UNSUPPORTED and nothing is written (the check sits in the entry point, in front
    of the launch)."""
    from ltxmi import _lib
    ops, lib = _ops(), _lib.lib
    n = 64
    x = torch.ones(n + 16, dtype=BF, device=DEV)
    m = torch.zeros(1, dtype=F32, device=DEV)
    out = torch.full((n + 16,), SENT, dtype=BF, device=DEV)
    s = ops._stream()
    ok = lambda t: ctypes.c_void_p(t.data_ptr())
    off = lambda t: ctypes.c_void_p(t.data_ptr() + shift)
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    codes = {
        "silu x": lib.ltxmi_silu_bf16(off(x), ok(out), n, s),
        "silu y": lib.ltxmi_silu_bf16(ok(x), off(out), n, s),
        "add a": lib.ltxmi_add_bf16(off(x), ok(x), ok(out), n, s),
        "add b": lib.ltxmi_add_bf16(ok(x), off(x), ok(out), n, s),
        "add y": lib.ltxmi_add_bf16(ok(x), ok(x), off(out), n, s),
        "stg a": lib.ltxmi_stg_blend_bf16(off(out), 8, ok(x), 8, ok(m), 1, 8, 8, s),
        "stg v": lib.ltxmi_stg_blend_bf16(ok(out), 8, off(x), 8, ok(m), 1, 8, 8, s),
    }
    torch.cuda.synchronize()
    assert codes == {k: UNSUPPORTED for k in codes}, codes
    assert bool((out == SENT).all())
    assert lib.ltxmi_silu_bf16(ok(x), ok(out), n, s) == 0      # the aligned call is taken
    torch.cuda.synchronize()
    assert bool((out[n:] == SENT).all()) and not bool((out[:n] == SENT).any())
