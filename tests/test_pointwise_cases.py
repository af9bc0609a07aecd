"""CPU tests of tests/pointwise_cases.py: the truths are the oracle's operations, the fp32 restatement of each operation
meets every metric on every case of tests/test_gpu_pointwise_kernels.py (the condition that makes that module fair), the
slack is what the CPU measures, DROPPED is exactly what fails, the threshold cases split as the module says, and every
geometry meant to pass a grid cap has more work items than the cap quoted from the source."""
import os

import pytest
import torch

import pointwise_cases as pc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ltx-video-gpupoor_amd", "csrc")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ------------------------------------------------------------------- the truths are the oracle's operations
def test_truths_agree_with_the_oracle_operations():
    from oracle import conditioning as oc, sched, upsampler as up, vae as ov
    g = pc.ADAIN_GEOMS[0]
    x, r = pc.adain_inputs("plain", g, pc.F32)
    for f in pc.ADAIN_FACTORS:
        assert _rel(pc.adain_op(x, r, f)[0], up.adain_filter_latent(x.double(), r.double(), f)) < 1e-12
    geom = pc.TILE_GEOMS[1]
    a, b = pc.tile_inputs(geom, pc.F32)
    want = ov._blend(a.double(), b.double().clone(), geom[3], geom[2])
    assert _rel(pc.tile_blend_op(a, b, geom[3], geom[2])[0], want) < 1e-12
    lat, init, noise = pc.masked_inputs("plain", 37, 4, pc.F32)
    mask = pc.threshold_mask(pc.cond_noise_threshold_masks(), 37)
    for dt in (pc.F32, pc.F64):
        want = oc.add_noise_to_image_conditioning_latents(0.63, init.to(dt), lat.to(dt), 0.15, mask.to(dt), noise.to(dt))
        assert torch.equal(pc.cond_noise_op(lat, init, noise, mask, 0.15, 0.63, dt=dt)[0], want)
    for k, (gs, stg, rs, do_cfg, do_stg, do_res) in enumerate(pc.GUIDANCE_SETTINGS):
        npred = pc.guidance_npred("offset", 257, do_cfg, do_stg)
        v, alpha, factor, _ = pc.guidance_parts(npred, gs, stg, rs, do_cfg, do_stg, do_res)
        x = list(npred.double())
        text = x[1] if do_cfg else x[0]
        use = do_cfg and gs not in (0.0, 1.0)
        out = (alpha * x[0] + gs * (text - alpha * x[0]) if use else text) + (stg * (text - x[-1]) if do_stg else 0)
        assert _rel(out * factor, v) < 1e-12, k                       # alpha and factor are the oracle's
        if do_cfg and not use:
            assert _rel(v / factor, text + stg * (text - x[-1])) < 1e-12
    tsch = sched.set_timesteps(8, (1, 128, 3, 20, 20))
    lat = pc.make("plain", 1, 257).double().reshape(1, 257, 1)
    want = sched.denoising_step(tsch.double(), lat, v.reshape(1, 257, 1), None, None, tsch[3].double())
    got, _ = pc.guidance_step_op(npred, lat, float(tsch[3].double() - tsch[4].double()), *pc.GUIDANCE_SETTINGS[-1])
    assert _rel(got.reshape(1, 257, 1), want) < 1e-12


def test_layout_references_are_the_oracle_permutations():
    from oracle import vae as ov
    x = pc.make_like("plain", (2, 3, 2, 3, 48))
    y = pc.unpatchify_ref(x, 4)
    assert y.shape == (2, 3, 3, 8, 12)
    b, t, h, w, c, r, q = 1, 2, 1, 2, 1, 3, 2                       # channel n = (c p + r) p + q holds pixel (h p + q, w p + r)
    assert y[b, c, t, h * 4 + q, w * 4 + r] == x[b, t, h, w, (c * 4 + r) * 4 + q]
    back = pc.patchify_ref(y, 4, 64)
    assert torch.equal(back[..., :48], x) and not back[..., 48:].any()
    assert torch.equal(pc.unpatchify_ref(x, 1), pc.to_ncdhw(x)) and torch.equal(ov.patchify(y, 1, 1), y)
    p = pc.make_like("plain", (1, 2, 3, 5, 32))
    s = pc.pixel_shuffle2d_ref(p)
    assert s.shape == (1, 2, 6, 10, 8)
    assert s[0, 1, 2 * 2 + 1, 2 * 4 + 0, 5] == p[0, 1, 2, 4, (1 * 2 + 0) * 8 + 5]


# -------------------------------------------------------- the fairness condition of the GPU module, case by case
_WORST = {}


def _id(c):
    return f"{c[0]}-{c[1]}-{c[2]}".replace(" ", "")


@pytest.mark.parametrize("op,family,geom", pc.ARITH_CASES, ids=[_id(c) for c in pc.ARITH_CASES])
def test_fp32_restatement_meets_every_metric(op, family, geom):
    out, truth, mag = pc.cpu_case(op, family, geom)
    pc.compare(out, truth, mag, what=f"{op} {family} {geom}")
    g = pc.op_group(op)
    _WORST[g] = max(_WORST.get(g, 0.0), pc.excess(out, truth, mag))


def test_recorded_slack_is_what_the_cpu_measures():
    groups = {pc.op_group(c[0]) for c in pc.ARITH_CASES}
    worst = _WORST if set(_WORST) == groups else pc.measure_excess()
    for op, v in sorted(worst.items()):
        print(f"{op}: excess {v:.3e} = {v / 2.0 ** -24:.2f} x 2^-24")
    top = max(worst.values())
    assert 0.9 * pc.MEASURED_EXCESS <= top <= pc.MEASURED_EXCESS, (top, pc.MEASURED_EXCESS)
    assert pc.SLACK == 4.0 * pc.MEASURED_EXCESS


def test_dropped_is_exactly_what_fails():
    """Every listed case passes (the test above); every dropped pair fails somewhere; at most 3 pairs and never plain."""
    assert len(pc.DROPPED) <= 3 and all(f != "plain" for _, f in pc.DROPPED)
    saved, pc.DROPPED = pc.DROPPED, {}
    try:
        every = pc.arith_cases()
    finally:
        pc.DROPPED = saved
    for pair in pc.DROPPED:
        failed = 0
        for op, fam, geom in every:
            if (op, fam) == pair:
                try:
                    pc.compare(*pc.cpu_case(op, fam, geom))
                except AssertionError:
                    failed += 1
        assert failed, pair
    assert [c for c in every if (c[0], c[1]) not in pc.DROPPED] == pc.ARITH_CASES


def test_the_settings_and_sizes_the_gpu_module_needs_are_in_the_table():
    assert pc.GUIDANCE_N == [2, 255, 256, 257, 65536 + 3, 4992 * 128]
    assert pc.GUIDANCE_SETTINGS[4][0] == 1.0 and pc.GUIDANCE_SETTINGS[5][0] == 0.0 and pc.GUIDANCE_SETTINGS[4][3] and pc.GUIDANCE_SETTINGS[5][3]
    assert pc.SILU_SIZES == [8, 8 * (2048 * 256 + 5)] and pc.STG_M == [1.0, 0.0, 0.25]
    assert {(g[0], g[1]) for g in pc.S2D_GEOMS} == {(2, 1), (1, 2), (2, 2)} and {g[2] for g in pc.S2D_GEOMS} == {1, 2, 4}
    assert any(g[0] == 2 and g[4] == 1 for g in pc.S2D_GEOMS) and any(g[0] == 2 and g[4] % 2 == 1 and g[4] > 1 for g in pc.S2D_GEOMS)
    assert {s[1] for s in pc.LAYOUT_SHAPES} == {1, 16, 128} and {c for _, c in pc.MASKED_GEOMS} == {1, 128}
    fams = {op: {c[1] for c in pc.ARITH_CASES if c[0] == op} for op in {c[0] for c in pc.ARITH_CASES}}
    for op, f in fams.items():
        want = {"plain", "offset"} if op.startswith("guidance") else ({"plain"} if op == "tile_blend" else set(pc.FAMILIES))
        assert f == want - {fam for o, fam in pc.DROPPED if o == op}, (op, f)
    x = pc.make("large", 1, pc.SILU_SIZES[1], seed=11).float()
    assert float(x.min()) < -90 and bool(torch.isfinite(x).all())
    x, _ = pc.adain_inputs("offset", pc.ADAIN_GEOMS[0], pc.F32)
    assert float(x.mean()) > 100 and float(x.std()) < 1
    assert any(g[2] != g[3] for g in pc.ADAIN_GEOMS) and any(g[2] == (1, 1, 2) for g in pc.ADAIN_GEOMS)


# ------------------------------------------------------------------------------------------------ grid caps
def _prod(*v):
    n = 1
    for x in v:
        n *= x
    return n


def test_every_large_geometry_passes_the_cap_quoted_from_the_source():
    for name, (blocks, threads, fname, text) in pc.CAPS.items():
        src = open(os.path.join(CSRC, fname)).read()
        assert text in src, (name, text)
    assert "constexpr int PW_THREADS = 256;" in open(os.path.join(CSRC, "pointwise.hip")).read()
    assert "constexpr int UP_THREADS = 256;" in open(os.path.join(CSRC, "upsampler.hip")).read()
    pw = pc.cap_items("pw_grid")
    assert pw == 524288 and pc.cap_items("guidance") == 65536
    assert pc.SILU_SIZES[1] // 8 > pw and pc.SILU_SIZES[1] // 8 % 256 != 0
    B, L, D, _, _ = pc.STG_GEOMS[-1]
    assert B * L * D // 8 > pw
    assert _prod(*pc.LAYOUT_SHAPES[-1]) > pw and _prod(*pc.LAYOUT_SHAPES[-1][2:]) % 2 == 1
    st, s, group, B, T, H, W, Cin = pc.S2D_GEOMS[-1]
    assert B * ((T + 1) // st) * (H // s) * (W // s) * (Cin // group) * st * s * s > pw
    B, T, H, W, Co, p, off = pc.UNPATCHIFY_GEOMS[0]
    assert (Co, p, off) == (3, 4, 0) and B * T * H * W > pw                         # positions of the patch-4 kernel
    assert pc.UNPATCHIFY_GEOMS[-1] == (B, T, H, W, Co, p, 4)                          # the same through 8 bytes of offset
    generic = [g for g in pc.UNPATCHIFY_GEOMS if (g[4], g[5]) != (3, 4)]
    assert {(g[4], g[5]) for g in generic} == {(3, 2), (4, 4), (3, 1)}
    assert all(_prod(g[0], g[1], g[2], g[3], g[4], g[5], g[5]) > pw for g in generic)
    for B, C, T, H, W, p, cpad in pc.PATCHIFY_GEOMS[:2]:
        assert B * T * (H // p) * (W // p) * cpad > pw
    assert {(g[5], g[6] == g[1]) for g in pc.PATCHIFY_GEOMS[:2]} == {(4, False), (1, True)}
    assert pc.GUIDANCE_N[-2] == pc.cap_items("guidance") + 3 and pc.GUIDANCE_N[-1] > pc.cap_items("guidance")
    assert all(t * c > pw for t, c in pc.MASKED_GEOMS[-1:])
    B, T, H, W, C4 = pc.PIXEL_SHUFFLE_SHAPE
    assert C4 == 32 and B * T * 4 * H * W * (C4 // 4 // 8) > pc.cap_items("pixel_shuffle2d")
    sa, lb, dim, extent = pc.TILE_GEOMS[-1]
    assert _prod(*sa) // sa[dim] * extent > pc.cap_items("tile_blend") and extent == sa[dim] == lb
    assert pc.TILE_GEOMS[0][3] == 1


# ------------------------------------------------------------------------------------------------ thresholds
def test_cond_noise_threshold_masks_split():
    m = pc.cond_noise_threshold_masks()
    assert m.dtype == torch.float32 and float(m[3]) == 1.0 and m[0] < m[1] < m[2] < m[3]
    assert float(m[1]) == 16777199 * 2.0 ** -24 and float(m[2]) == 16777200 * 2.0 ** -24
    r32, r64 = pc.oracle_resets(m.view(1, 4), pc.F32), pc.oracle_resets(m.view(1, 4), pc.F64)
    assert r32.tolist() == [[False, False, True, True]]
    # no fp32 value lies between fp32(1 - 1e-6) and the unrounded 1 - 1e-6 (module docstring): the two runs cannot differ
    assert float(m[1]) < 1.0 - 1e-6 < float(m[2]) and torch.equal(r32, r64)
    assert (m >= m[1]).tolist() != r32[0].tolist()                          # ``>=`` would reset the token at the threshold
    mask = pc.threshold_mask(m, 37)
    assert set(mask[0].tolist()) >= set(m.tolist()) and 0 < int(pc.oracle_resets(mask).sum()) < 37


def test_guidance_threshold_case_splits_and_float64_disagrees():
    tsch, i, masks = pc.guidance_threshold_case()
    t = tsch[i]
    assert masks.dtype == torch.float32 and 0 < i < tsch.numel() - 1
    A = t - torch.tensor(1e-6)
    step = 2.0 ** -24
    assert (1.0 - masks)[:3].double().tolist() == [float(A) - step, float(A), float(A) + step]      # exact in fp32
    assert masks[0] == torch.nextafter(masks[1], torch.tensor(1.0)) and masks[2] == torch.nextafter(masks[1], torch.tensor(0.0))
    assert abs(float(1.0 - masks[3]) - float(t)) <= step / 2
    m32, m64 = pc.oracle_moves(tsch, t, masks.view(1, 4), pc.F32), pc.oracle_moves(tsch, t, masks.view(1, 4), pc.F64)
    assert m32.tolist() == [[False, False, True, True]]
    assert not torch.equal(m32, m64), "the float64 run agrees on every token: the case proves nothing"
    assert (A <= 1.0 - masks).tolist() != m32[0].tolist()                      # ``<=`` would move the token at A
    for tt in tsch[(tsch >= 0.25) & (tsch < 1)]:                               # fp32 rounds A down there (module docstring)
        assert float((tt - torch.tensor(1e-6)).double()) < float(tt.double()) - 1e-6
    assert (tsch.numel(), i, float(t)) == (19, 17, 0.24470679461956024)
    from oracle import sched
    for steps in (8, 19, 40):                                                  # the default schedule lies on the grid 2^-24
        d = sched.set_timesteps(steps, (1, 128, 3, 20, 20)).double() * 2.0 ** 24
        assert torch.equal(d, d.round())


# -------------------------------------------------------------------------------------------- guidance scalars
@pytest.mark.parametrize("n", [2, 257, 65539])
@pytest.mark.parametrize("k", range(len(pc.GUIDANCE_SETTINGS)))
def test_scalars_are_recovered_from_a_probe_call(n, k):
    """What the GPU module does with the kernel, done with the fp32 restatement: latents 0 and dt -1 give back factor
    (alpha a + c), and the least-squares solve returns alpha and factor to 1e-5; a one-pass variance in fp32 on the offset
    family is seen by it."""
    gs, stg, rs, do_cfg, do_stg, do_res = pc.GUIDANCE_SETTINGS[k]
    for fam in ("plain", "offset"):
        npred = pc.guidance_npred(fam, n, do_cfg, do_stg)
        zero = torch.zeros(1, n, 1)
        o = pc.restate(pc.guidance_step_op, npred, zero, -1.0, gs, stg, rs, do_cfg, do_stg, do_res, out_dtype=pc.F32)
        _, alpha, factor, _ = pc.guidance_parts(npred, gs, stg, rs, do_cfg, do_stg, do_res)
        a, f = pc.recover_scalars(o, npred, gs, stg, do_cfg, do_stg)
        assert abs(f / float(factor) - 1) < 1e-5, (fam, f, float(factor))
        if a is not None:
            assert abs(a / float(alpha) - 1) < 1e-5, (fam, a, float(alpha))
        else:
            assert not (do_cfg and gs not in (0.0, 1.0))
        o_bad = o * 1.004                                                     # a factor wrong by 2^-8
        assert abs(pc.recover_scalars(o_bad, npred, gs, stg, do_cfg, do_stg)[1] / float(factor) - 1) > pc.SCALAR_TOL


def test_metrics_see_one_wrong_chunk():
    """One chunk of 8 in half a million that is 3 % off passes ``check`` and fails ``compare``."""
    from test_gpu_kernels import check
    x = pc.make("plain", 1, pc.SILU_SIZES[1], seed=11)
    truth, mag = pc.silu_op(x)
    bad = pc.restate(pc.silu_op, x).clone()
    bad[0, 800:808] = (bad[0, 800:808].float() * 1.03).to(pc.BF)
    check(bad, truth)
    with pytest.raises(AssertionError):
        pc.compare(bad, truth, mag)


def test_tile_blend_weight_case_has_teeth():
    """With b = 0 in fp32 the reference's weights (each rounded once) meet the bound and 1 - fp32(z / extent) does not."""
    a, b = pc.tile_weight_inputs()
    truth, mag = pc.tile_blend_op(a, b, 33, 2)
    good = pc.restate(pc.tile_blend_op, a, b, 33, 2, out_dtype=pc.F32)
    pc.compare(good, truth, mag)
    assert pc.excess(good, truth, mag) <= pc.MEASURED_EXCESS
    fig, _ = pc.element_figure(pc.tile_blend_one_minus_w(a, b, 33, 2), truth, mag)
    print(f"1 - w form: {fig:.2f} of the bound")
    assert fig > 1
