"""mixed_precision on a real MI355X: the two row kernels of the fp32 residual stream (csrc/stream32.hip) against the
bounds of tests/mixed_kernel_cases.py, and ``Transformer3DModel.forward(mixed=True)`` / ``LTXVideoPipeline(mixed_precision=
True)`` against the reference's own mixed rendering (tests/mixed_oracle.py run with bf16 linears; pinned to the reference's
output by tests/test_mixed_cpu.py) under ``assert_parity`` of tests/test_gpu_model.py:

        err(ours, mixed) <= err(reference, mixed) + 2e-3          (relative L2 against the fp32 truth)

Figures measured on the MI355X are in DESIGN.md (section 5, "mixed precision")."""
import pytest
import torch

import mixed_kernel_cases as mk
import mixed_oracle
import norm_cases as nc
from test_gpu_model import BF, DEV, _Holder, _oracle_loop, assert_parity, build_model, dit_case, rel

pytestmark = pytest.mark.gpu

SENT = -12352.0                 # exactly representable in bf16 (and fp32)
PAD = 2


def guard(rows, D, ld, dtype):
    """A [rows, D] view (row stride ld) inside a sentinel-filled buffer with PAD rows before and after."""
    buf = torch.full((rows + 2 * PAD, ld), SENT, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + rows, :D]


def intact(buf, rows, D):
    b = buf.clone()
    b[PAD:PAD + rows, :D] = SENT
    return bool((b == SENT).all())


# ------------------------------------------------------------------------------------------------ norm_modulate_f32in
@pytest.mark.parametrize("rpg", mk.GROUPS)
@pytest.mark.parametrize("D", mk.WIDTHS)
@pytest.mark.parametrize("kind", mk.KINDS)
def test_norm_modulate_f32in(kind, D, rpg):
    from ltxmi import ops
    x, table, temb, truth, mag = mk.norm_case(kind, D, rpg)
    xbuf, xd = guard(mk.ROWS, D, D + mk.PAD_COLS, torch.float32)
    xd.copy_(x)
    obuf, y = guard(mk.ROWS, D, D + mk.PAD_COLS, BF)
    td, ed = table.to(DEV), temb.to(DEV)                       # the tables are column slices of [groups, 6 D]
    ops.norm_modulate_f32in(xd, y, nc.EPS_DIT, ops.NORM_LAYER if kind == "layer" else ops.NORM_RMS, td[1], ed[:, D:2 * D],
                            td[0], ed[:, :D], rpg)
    torch.cuda.synchronize()
    what = f"norm_modulate_f32in {kind} D={D} rpg={rpg}"
    assert intact(obuf, mk.ROWS, D), f"{what}: wrote outside its rows / columns"
    assert intact(xbuf, mk.ROWS, D) and torch.equal(xd.cpu(), x), f"{what}: the input changed"
    f = nc.compare(y.cpu(), truth, mag, what=what)
    print(what, {k: round(v, 3) for k, v in f.items() if isinstance(v, float)})


def test_norm_modulate_f32in_is_the_bf16_kernel_on_bf16_valued_rows():
    """On rows whose values are bf16's the fp32-input kernel reads the numbers the bf16 kernel reads, and the two share the
    arithmetic (1 + (table + temb) against (1 + table) + temb: one rounding apart in fp32).  An fp32 ulp moves a value
    across a bf16 rounding boundary with a probability of about 2^-16 x 2^8 per element, so the outputs agree to a bf16 ulp
    everywhere and differ at all in far fewer than 1 % of the elements."""
    from ltxmi import ops
    D, rows, rpg = 2048, mk.ROWS, 7
    xb = nc.make("plain", rows, D).to(DEV)
    table, temb = (t.to(DEV) for t in nc.modulation((rows + rpg - 1) // rpg, D))
    a, b = torch.empty_like(xb), torch.empty_like(xb)
    for kind in (ops.NORM_RMS, ops.NORM_LAYER):
        ops.norm_modulate(xb, a, nc.EPS_DIT, kind, table[1], temb[:, D:2 * D], table[0], temb[:, :D], rpg)
        ops.norm_modulate_f32in(xb.float(), b, nc.EPS_DIT, kind, table[1], temb[:, D:2 * D], table[0], temb[:, :D], rpg)
        diff = (a.float() - b.float()).abs()
        assert bool((diff <= 2.0 ** -7 * a.float().abs() + 1e-6).all())
        assert float((diff > 0).float().mean()) < 0.01


# -------------------------------------------------------------------------------------------------- gate_residual_f32
def _run_gate(D, rpg, gated, round_product, with_copy):
    from ltxmi import ops
    h, y, g_tab, g_temb_cols = mk.gate_case(D, rpg)
    hbuf, hd = guard(mk.ROWS, D, D + mk.PAD_COLS, torch.float32)
    hd.copy_(h)
    ybuf, yd = guard(mk.ROWS, D, D + mk.PAD_COLS, BF)
    yd.copy_(y)
    bbuf, bd = guard(mk.ROWS, D, D + 2 * mk.PAD_COLS, BF)
    temb_full = torch.zeros((g_temb_cols.shape[0], 6 * D), dtype=BF, device=DEV)
    temb_full[:, 2 * D:3 * D] = g_temb_cols.to(DEV)
    kw = dict(gate_table=g_tab.to(DEV), gate_temb=temb_full[:, 2 * D:3 * D], rows_per_group=rpg) if gated else {}
    ops.gate_residual_f32_(hd, yd, round_product=round_product, h_bf16=bd if with_copy else None, **kw)
    torch.cuda.synchronize()
    what = f"gate_residual_f32 D={D} rpg={rpg} gated={gated} round={round_product}"
    assert intact(hbuf, mk.ROWS, D), f"{what}: wrote outside the [rows, D] window of h"
    assert intact(ybuf, mk.ROWS, D) and torch.equal(yd.cpu(), y), f"{what}: y changed"
    if with_copy:
        assert intact(bbuf, mk.ROWS, D), f"{what}: wrote outside the [rows, D] window of h_bf16"
        assert torch.equal(bd, hd.to(BF)), f"{what}: h_bf16 is not bf16(h) of the kernel's own h"
    else:
        assert bool((bbuf == SENT).all())
    g32 = mk.gate32(g_tab, g_temb_cols, rpg) if gated else None
    return hd.cpu(), h, y, g32, what


@pytest.mark.parametrize("rpg", mk.GROUPS)
@pytest.mark.parametrize("D", mk.WIDTHS)
def test_gate_residual_rounded_product_is_bit_equal(D, rpg):
    out, h, y, g32, what = _run_gate(D, rpg, True, 1, True)
    want = mk.gate_rounded_expected(h, y, g32)
    assert torch.equal(out, want), f"{what}: {int((out != want).sum())} elements differ from h + bf16(g * y)"
    assert not torch.equal(out, h + g32 * y.float())                # the rounding is really there


@pytest.mark.parametrize("rpg", mk.GROUPS)
@pytest.mark.parametrize("D", mk.WIDTHS)
def test_gate_residual_unrounded_product(D, rpg):
    out, h, y, g32, what = _run_gate(D, rpg, True, 0, False)
    print(what, "worst ulp", round(mk.gate_unrounded_check(out, h, y, g32, what), 3))
    assert not torch.equal(out, mk.gate_rounded_expected(h, y, g32))


@pytest.mark.parametrize("D", mk.WIDTHS)
def test_gate_residual_without_gate(D):
    out, h, y, _, what = _run_gate(D, 1, False, 0, True)
    print(what, "worst ulp", round(mk.gate_unrounded_check(out, h, y, None, what), 3))
    assert torch.equal(out, h + y.float())                          # one addition: nothing but its own rounding


def test_row_kernels_past_two_to_the_31_elements():
    """Element offsets past 2^31 (and byte offsets past 2^32) in both kernels, without moving that much data: 9 rows of 4096
    channels lie 2^28 + 8 elements apart in ONE untouched 9.7 GB allocation of fp32 (the stream; nothing but the 9 rows of it is
    read or written, the bf16 operands are 9 compact rows), so row 8 starts at element 2^31 + 64 and row 4 at byte 2^32 + 128.
    A 32-bit row offset anywhere in the address arithmetic lands these rows elsewhere."""
    from ltxmi import ops
    D, rows, ld, rpg = 4096, 9, (1 << 28) + 8, 4
    assert (rows - 1) * ld > 1 << 31
    g = torch.Generator(device=DEV).manual_seed(3)
    big = torch.empty(rows, ld, dtype=torch.float32, device=DEV)
    h = big[:, :D]
    h0 = torch.randn(rows, D, generator=g, device=DEV)
    h.copy_(h0)
    y = torch.randn(rows, D, generator=g, device=DEV).to(BF)
    table, temb = (t.to(DEV) for t in nc.modulation((rows + rpg - 1) // rpg, D))
    rows_of = torch.arange(rows, device=DEV) // rpg
    hb = torch.empty(rows, D, dtype=BF, device=DEV)
    ops.gate_residual_f32_(h, y, table[2], temb[:, 2 * D:3 * D], rpg, round_product=1, h_bf16=hb)
    want = h0 + ((table[2].float()[None] + temb[:, 2 * D:3 * D].float()[rows_of]) * y.float()).to(BF).float()
    assert torch.equal(h, want) and torch.equal(hb, want.to(BF))
    out, small = torch.empty(rows, D, dtype=BF, device=DEV), torch.empty(rows, D, dtype=BF, device=DEV)
    ops.norm_modulate_f32in(h, out, nc.EPS_DIT, ops.NORM_RMS, table[1], temb[:, D:2 * D], table[0], temb[:, :D], rpg)
    ops.norm_modulate_f32in(want, small, nc.EPS_DIT, ops.NORM_RMS, table[1], temb[:, D:2 * D], table[0], temb[:, :D], rpg)
    assert torch.equal(out, small)                                   # a row's result does not depend on where the row lies


# ------------------------------------------------------------------------------------------------------ model parity
def _mixed_forward(m, x, enc, mask, ts, frac, grid, **kw):
    with torch.no_grad():
        return m(x.float().to(DEV), freqs_cis=m.precompute_freqs_cis(frac.to(DEV)), encoder_hidden_states=enc.to(DEV),
                 encoder_attention_mask=mask.to(DEV), timestep=ts.to(DEV), latent_shape=grid, ltxv_model=_Holder(),
                 mixed=True, return_dict=False, **kw)[0]


@pytest.mark.parametrize("per_token", [False, True])
def test_transformer_mixed_small(per_token):
    """The shapes of test_transformer_small: 2 layers, D = 128 (2 heads x 64), grid (3, 5, 7), B 3, T 40."""
    grid, B, T = (3, 5, 7), 3, 40
    cfg, sd32, x, enc, mask, ts, frac = dit_case(2, 64, 2, grid, B, T, per_token=per_token)
    truth, eager = mixed_oracle.oracles(sd32, cfg, x, enc, mask, ts, frac, grid)
    out = _mixed_forward(build_model(cfg, sd32), x, enc, mask, ts, frac, grid)
    assert out.dtype == BF
    assert_parity(out, truth, eager, f"mixed small per_token={per_token}")


@pytest.mark.parametrize("alias", [0, 1])
@pytest.mark.parametrize("strategy", ["AttentionValues", "AttentionSkip", "Residual", "TransformerBlock"])
def test_transformer_mixed_stg_strategies(strategy, alias):
    """Every skip-layer strategy on the fp32 stream, block 1 of 2 skipped for the third row; with ``stg_alias_blocks`` the first
    block runs on two rows and the third is a copy (bit-identical, as on the bf16 stream)."""
    import ltxmi
    from oracle import dit
    grid, B, T = (3, 5, 7), 3, 40
    cfg, sd32, x, enc, mask, ts, frac = dit_case(2, 64, 2, grid, B, T, seed=3)
    x[2], enc[2], mask[2], ts[2] = x[1], enc[1], mask[1], ts[1]
    skip = dit.create_skip_layer_mask(2, 1, 3, 2, [1], torch.float32)
    code = {"AttentionValues": dit.ATTENTION_VALUES, "AttentionSkip": dit.ATTENTION_SKIP, "Residual": dit.RESIDUAL,
            "TransformerBlock": dit.TRANSFORMER_BLOCK}[strategy]
    m = build_model(cfg, sd32)
    kw = dict(skip_layer_mask=m.create_skip_layer_mask(1, 3, 2, [1]), skip_layer_strategy=getattr(ltxmi.SkipLayerStrategy, strategy))
    out = _mixed_forward(m, x, enc, mask, ts, frac, grid, **kw)
    if alias:
        assert torch.equal(_mixed_forward(m, x, enc, mask, ts, frac, grid, stg_alias_blocks=alias, **kw), out)
        return
    truth, eager = mixed_oracle.oracles(sd32, cfg, x, enc, mask, ts, frac, grid, skip_layer_mask=skip, skip_layer_strategy=code)
    assert_parity(out, truth, eager, f"mixed stg {strategy}")
    if strategy != "Residual":                                       # (a no-op without residual_connection, attention.py:1161-1168)
        assert rel(out[2], out[1]) > 1e-3


def test_transformer_mixed_2b_width_one_block():
    """One block at the 2B widths (D 2048 = 32 x 64, FF 8192, caption 4096), N = 624, B_eff 3 with the STG row."""
    import ltxmi
    from oracle import dit
    grid, B, T = (2, 13, 24), 3, 256
    cfg, sd32, x, enc, mask, ts, frac = dit_case(32, 64, 1, grid, B, T, caption=4096, seed=16)
    skip = dit.create_skip_layer_mask(1, 1, 3, 2, [0], torch.float32)
    truth, eager = mixed_oracle.oracles(sd32, cfg, x, enc, mask, ts, frac, grid, skip_layer_mask=skip,
                                        skip_layer_strategy=dit.ATTENTION_VALUES)
    m = build_model(cfg, sd32)
    out = _mixed_forward(m, x, enc, mask, ts, frac, grid, skip_layer_mask=m.create_skip_layer_mask(1, 3, 2, [0]),
                         skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues)
    assert out.shape == (3, 624, 128)
    assert_parity(out, truth, eager, "mixed 2B width, 1 block, N 624")


def test_transformer_mixed_13b_width_one_block():
    """One block at the 13B widths (D 4096 = 32 x 128): N = 1040 x B 2 puts self-attention on the head_dim-128 pipelined kernel,
    and the row kernels on 16 chunks per lane."""
    from ltxmi import ops
    grid, B, T = (5, 13, 16), 2, 128
    cfg, sd32, x, enc, mask, ts, frac = dit_case(32, 128, 1, grid, B, T, caption=4096, seed=26)
    assert ops.attention_kernel_id(B, 32, 1040, 1040, 128) == 6
    truth, eager = mixed_oracle.oracles(sd32, cfg, x, enc, mask, ts, frac, grid)
    out = _mixed_forward(build_model(cfg, sd32), x, enc, mask, ts, frac, grid)
    assert out.shape == (2, 1040, 128)
    assert_parity(out, truth, eager, "mixed 13B width, 1 block, N 1040")


def test_transformer_mixed_2b_full_depth():
    """All 28 layers at the 2B widths, N = 624 (the shape of test_transformer_2b_full_depth), the STG row perturbed from block
    19.  The oracles run on the GPU (torch's eager kernels: the reference's own path on this hardware; nothing of libltxmi).
    Parity with the reference's mixed rendering, and the reason the mode exists: the mixed output is closer to the fp32 truth
    than the product's own bf16 output on the same inputs (on the reference the ratio is about 0.5 at 4 and 8 layers; the
    figures measured here are in DESIGN.md section 5)."""
    import ltxmi
    from oracle import dit
    grid, B, T = (2, 13, 24), 3, 256
    cfg, sd32, x, enc, mask, ts, frac = dit_case(32, 64, 28, grid, B, T, caption=4096, seed=26)
    skip = dit.create_skip_layer_mask(28, 1, 3, 2, [19], torch.float32)
    truth, eager = mixed_oracle.oracles(sd32, cfg, x, enc, mask, ts, frac, grid, device=DEV, skip_layer_mask=skip,
                                        skip_layer_strategy=dit.ATTENTION_VALUES)
    m = build_model(cfg, sd32)
    del sd32
    kw = dict(skip_layer_mask=m.create_skip_layer_mask(1, 3, 2, [19]), skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues)
    out = _mixed_forward(m, x, enc, mask, ts, frac, grid, **kw)
    assert out.shape == (3, 624, 128) and out.dtype == BF
    e_mixed, e_ref = assert_parity(out, truth, eager, "mixed 2B, 28 layers, N 624, B_eff 3")
    with torch.no_grad():
        plain = m(x.to(DEV), freqs_cis=m.precompute_freqs_cis(frac.to(DEV)), encoder_hidden_states=enc.to(DEV),
                  encoder_attention_mask=mask.to(DEV), timestep=ts.to(DEV), latent_shape=grid, ltxv_model=_Holder(),
                  return_dict=False, **kw)[0]
    e_plain = rel(plain, truth)
    print(f"28 layers, rel L2 vs fp32 truth: mixed {e_mixed:.3e}, the product's bf16 path {e_plain:.3e} "
          f"(ratio {e_mixed / e_plain:.2f}); the reference's mixed rendering {e_ref:.3e}")
    assert e_mixed < e_plain, (e_mixed, e_plain)


def test_bf16_forward_is_untouched_by_a_mixed_forward():
    """Cached packs, text K/V and buffers survive a mixed forward: the bf16 forward gives the same bits before and after."""
    import ltxmi
    grid, B, T = (2, 4, 8), 3, 24
    cfg, sd32, x, enc, mask, ts, frac = dit_case(2, 64, 3, grid, B, T, seed=3)
    m = build_model(cfg, sd32)
    kw = dict(freqs_cis=m.precompute_freqs_cis(frac.to(DEV)), encoder_hidden_states=enc.to(DEV),
              encoder_attention_mask=mask.to(DEV), timestep=ts.to(DEV), skip_layer_mask=m.create_skip_layer_mask(1, 3, 2, [1]),
              skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues, latent_shape=grid, ltxv_model=_Holder(),
              return_dict=False)
    with torch.no_grad():
        before = m(x.to(DEV), **kw)[0].clone()
        mixed = m(x.float().to(DEV), mixed=True, **kw)[0].clone()
        after = m(x.to(DEV), **kw)[0]
        again = m(x.float().to(DEV), mixed=True, **kw)[0]
    assert torch.equal(before, after) and torch.equal(mixed, again)
    assert not torch.equal(mixed, before)


# -------------------------------------------------------------------------------------------------------------- loop
def _mixed_oracle_loop(sd32, cfg, noise_tokens, emb, msk, tsch, grid, gs, stg, rs, skips, ld):
    """``_oracle_loop`` of tests/test_gpu_model.py with the transformer in its mixed form (pipeline_ltx_video.py:1061,
    1152-1177): fp32 latents go in as they are, ``noise_pred`` comes back in ``ld``, guidance and the step run on fp32."""
    from oracle import dit, sched
    f, h, w = grid
    sd = {k: v.to(ld) for k, v in sd32.items()}
    pix = sched.latent_to_pixel_coords(sched.get_latent_coords(f, h, w, 1),
                                       causal_fix=cfg.get("causal_temporal_positioning", False)).to(torch.float32)
    pix[:, 0] = pix[:, 0] * (1.0 / 25.0)
    fc = dit.precompute_freqs_cis(pix, cfg, ld)
    lat = noise_tokens.clone().float()
    n = 3
    for i, t in enumerate(tsch):
        skip = dit.create_skip_layer_mask(cfg["num_layers"], 1, n, n - 1, skips[i], ld)
        npred = mixed_oracle.transformer3d_forward_mixed(sd, cfg, torch.cat([lat] * n), fc, emb.to(ld), t.expand(n).unsqueeze(-1), ld,
                                                         encoder_attention_mask=msk, latent_shape=(f, h, w), skip_layer_mask=skip,
                                                         skip_layer_strategy=dit.ATTENTION_VALUES)
        v = sched.guidance(npred.float(), n, gs[i], stg[i], rs[i], True, True, True)
        lat = sched.denoising_step(tsch, lat, v, t.expand(1).unsqueeze(-1), None, t)
    return sched.unpatchify(lat, f, h, w)


def test_pipeline_mixed_precision_two_steps():
    """test_pipeline_config1_two_steps with ``mixed_precision=True``: 2 denoise steps, CFG + STG, bf16 prompt embeddings (the
    latents are fp32 all the same, :1061), against the oracle's fp32 loop on identical noise; the yardstick is the reference's
    mixed loop."""
    import ltxmi
    from oracle import dit, sched
    heads, dh, layers, caption, T = 2, 64, 2, 128, 32
    cfg = dict(dit.default_2b_config(), num_attention_heads=heads, attention_head_dim=dh, num_layers=layers,
               cross_attention_dim=heads * dh, caption_channels=caption)
    sd32 = {k: v.to(BF).float() for k, v in dit.init_state_dict(cfg, seed=7).items()}
    g = torch.Generator().manual_seed(8)
    f, h, w = 2, 8, 8
    lat0 = torch.randn(1, f * h * w, 128, generator=g)
    pos, neg = torch.randn(1, T, caption, generator=g).to(BF), torch.randn(1, T, caption, generator=g).to(BF)
    pmask, nmask = torch.ones(1, T), torch.ones(1, T)
    pmask[:, 20:] = 0
    nmask[:, 5:] = 0
    gs, stg, rs, skip_blocks, steps = 3.0, 1.0, 0.7, [1], 2
    tsch = sched.set_timesteps(steps, (1, 128, f, h, w))
    emb = torch.cat([neg, pos, pos]).float()
    msk = torch.cat([nmask, pmask, pmask])
    per_step = ([gs] * steps, [stg] * steps, [rs] * steps, [skip_blocks] * steps)
    truth = _oracle_loop(sd32, cfg, lat0, emb, msk, tsch, (f, h, w), *per_step, torch.float32)
    same = _mixed_oracle_loop(sd32, cfg, lat0, emb, msk, tsch, (f, h, w), *per_step, torch.float32)
    torch.testing.assert_close(same, truth, rtol=1e-5, atol=2e-6)    # in fp32 the mixed loop is the plain loop
    eager = _mixed_oracle_loop(sd32, cfg, lat0, emb, msk, tsch, (f, h, w), *per_step, BF)

    m = build_model(cfg, sd32)
    pipe = ltxmi.LTXVideoPipeline(transformer=m, scheduler=ltxmi.RectifiedFlowScheduler(shifting="SD3", target_shift_terminal=0.1))
    out = pipe(height=256, width=256, num_frames=9, frame_rate=25.0, prompt_embeds=pos.to(DEV), prompt_attention_mask=pmask.to(DEV),
               negative_prompt_embeds=neg.to(DEV), negative_prompt_attention_mask=nmask.to(DEV), num_inference_steps=steps,
               guidance_scale=gs, stg_scale=stg, rescaling_scale=rs, skip_block_list=skip_blocks, latents=lat0.to(DEV),
               output_type="latent", skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues, is_video=True, joint_pass=True,
               mixed_precision=True)
    assert out.dtype == torch.float32 and out.shape == truth.shape == (1, 128, f, h, w)
    assert_parity(out, truth, eager, "pipeline mixed_precision, 2 steps")
