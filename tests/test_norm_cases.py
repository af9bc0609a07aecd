"""CPU tests of tests/norm_cases.py: the float64 truths are the reference's operations, the fp32 restatement of each
operation meets every metric on every case of the GPU module (the condition that makes tests/test_gpu_norm_kernels.py
fair), the slack figure is what the CPU measures, and the offset families have teeth."""
import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------- the truths are the reference's operations
@pytest.mark.parametrize("D", [64, 1000, 2048])
def test_truths_agree_with_the_reference_operations(D):
    from oracle import dit, leaves, vae as ov
    rows = 45
    x = nc.make("plain", rows, D)
    xf = x.float()
    zero, zrow = torch.zeros(D), torch.zeros(rows, D)
    # LayerNorm / RMSNorm without affine (+ a modulation of zero), and with a real modulation
    t, _ = nc.norm_modulate_op(x, "layer", 1e-6, zero, zrow, zero, zrow)
    assert _rel(t, F.layer_norm(xf, (D,), None, None, 1e-6)) < 1e-5
    t, _ = nc.norm_modulate_op(x, "rms", 1e-6, zero, zrow, zero, zrow)
    assert _rel(t, leaves.rms_norm(xf, 1e-6)) < 1e-5
    table, temb = nc.modulation(7, D)
    sc, sh = nc.group_rows(temb[:, D:2 * D], 7, rows), nc.group_rows(temb[:, :D], 7, rows)
    t, _ = nc.norm_modulate_op(x, "rms", 1e-6, table[1], sc, table[0], sh)
    ref = leaves.rms_norm(xf, 1e-6) * (1 + table[1].float() + sc.float()) + table[0].float() + sh.float()
    assert _rel(t, ref) < 1e-5
    # q / k norm with weight, then RoPE
    w = nc.bf(D, seed=1, scale=0.1, offset=1.0)
    cos, sin = nc.rope_tables(rows, D)
    t, _ = nc.rmsnorm_rope_op(x, w, 1e-5)
    assert _rel(t, leaves.rms_norm(xf, 1e-5, w.float())) < 1e-5
    t, _ = nc.rmsnorm_rope_op(x, w, 1e-5, cos, sin)
    assert _rel(t, dit.apply_rotary_emb(leaves.rms_norm(xf, 1e-5, w.float()), (cos.float(), sin.float()))) < 1e-5
    # PixelNorm (channel axis = dim 1 in the reference), LayerNorm with affine
    t, _ = nc.pixelnorm_op(x, 1e-8, silu=False)
    assert _rel(t, ov.pixel_norm(xf.t()[None], 1e-8)[0].t()) < 1e-5
    g, b = nc.bf(D, seed=2), nc.bf(D, seed=3)
    t, _ = nc.layernorm_affine_op(x, g, b, 1e-6)
    assert _rel(t, F.layer_norm(xf, (D,), g.float(), b.float(), 1e-6)) < 1e-5


@pytest.mark.parametrize("samples,S,C,groups,with_res", [(2, 105, 64, 32, True), (3, 7, 512, 1, False), (1, 33, 8, 8, False)])
def test_groupnorm_truth_agrees_with_torch_group_norm(samples, S, C, groups, with_res):
    x, gamma, beta, res = nc.gn_inputs("plain", samples, S, C, with_res)
    t, _ = nc.groupnorm_silu_op(x, groups, gamma, beta, 1e-5, res)
    ref = F.group_norm(x.float().permute(0, 2, 1), groups, gamma.float(), beta.float(), 1e-5).permute(0, 2, 1)
    ref = F.silu(ref + (res.float() if with_res else 0))
    assert _rel(t, ref) < 1e-5


def test_pack_layout_and_rstd_truth():
    B, Nl, D, P = 2, 5, 64, 4
    q, k, v = (nc.bf(B * Nl, D, seed=s) for s in (1, 2, 3))
    out = nc.pack_layout(q, k, v, B, Nl, P)
    assert out.shape == (P, Nl, B, 3, D // P)
    for p, n, b, c in [(0, 0, 0, 0), (3, 4, 1, 15), (2, 1, 1, 7)]:
        row, col = b * Nl + n, p * (D // P) + c
        assert out[p, n, b, 0, c] == q[row, col] and out[p, n, b, 1, c] == k[row, col] and out[p, n, b, 2, c] == v[row, col]
    ss = torch.rand(4, 6, dtype=torch.float32) * 100
    assert torch.allclose(nc.rstd_op(ss, 384, 1e-5), 1 / torch.sqrt(ss.double().sum(-1) / 384 + 1e-5))


# -------------------------------------------------------- the fairness condition of the GPU module, case by case
_ROW_CASES = [(op, fam, D) for op, widths in nc.ROW_OPS.items() for D in widths for fam in nc.families_for(op, D)]
_WORST = {}


@pytest.mark.parametrize("op,family,D", _ROW_CASES, ids=[f"{o}-{f}-{d}" for o, f, d in _ROW_CASES])
def test_fp32_restatement_meets_every_metric_row_kernels(op, family, D):
    out, truth, mag = nc.cpu_case(op, family, D)
    nc.compare(out, truth, mag, what=f"{op} {family} {D}")
    _WORST[op] = max(_WORST.get(op, 0.0), nc.excess(out, truth, mag))


_GN_CASES = [(fam, case) for case in nc.GN_CASES for fam in nc.gn_families(case)]


@pytest.mark.parametrize("family,case", _GN_CASES, ids=[f"{f}-" + "x".join(map(str, c)) for f, c in _GN_CASES])
def test_fp32_restatement_meets_every_metric_groupnorm(family, case):
    out, truth, mag = nc.gn_cpu_case(family, *case)
    nc.compare(out, truth, mag, what=f"groupnorm {family} {case}")
    _WORST["groupnorm"] = max(_WORST.get("groupnorm", 0.0), nc.excess(out, truth, mag))


@pytest.mark.parametrize("C", sorted(nc.NARROW_TRIP))
def test_fp32_restatement_meets_every_metric_narrow_pixelnorm_second_trip(C):
    """The 4096 x 4 x (512 / C) + 5 row cases; at C = 64 the per-row L2 of the restatement is over the limit (so it is not
    asserted on the GPU either), which this test pins so that the exemption cannot outlive its reason."""
    from test_gpu_kernels import REL_L2
    x, sc, sh = nc.narrow_trip_inputs(C)
    args = (x, nc.EPS_PIXEL, sc.expand_as(x), sh.expand_as(x), True)
    truth, mag = nc.pixelnorm_op(*args)
    out = nc.restate(nc.pixelnorm_op, *args)
    nc.compare(out, truth, mag, what=f"pixelnorm second trip C={C}", per_row=nc.NARROW_TRIP[C])
    assert nc.excess(out, truth, mag) <= nc.MEASURED_EXCESS
    if not nc.NARROW_TRIP[C]:
        assert nc.figures(out, truth, mag)["row_l2"] > 1


def test_recorded_slack_is_what_the_cpu_measures():
    """MEASURED_EXCESS is the largest excess of the fp32 restatement over all cases (those of the two tests above when they
    ran in this process, else measured here), and SLACK is 4 times it: the figure is pinned from both sides."""
    worst = _WORST if len(_WORST) == len(nc.ROW_OPS) + 1 else nc.measure_excess()
    for op, v in sorted(worst.items()):
        print(f"{op}: excess {v:.3e} = {v / 2.0 ** -24:.2f} x 2^-24")
    top = max(worst.values())
    assert 0.9 * nc.MEASURED_EXCESS <= top <= nc.MEASURED_EXCESS, (top, nc.MEASURED_EXCESS)
    assert nc.SLACK == 4.0 * nc.MEASURED_EXCESS


# ------------------------------------------------------------------------------------- the families have teeth
@pytest.mark.parametrize("D", [128, 2048, 8192])
def test_one_pass_variance_fails_offset1024_and_passes_offset256(D):
    """E[x^2] - mean^2 in fp32, summed as a one-wave-per-row kernel sums: within REL_L2 up to offset 256, out by a
    factor of 4 or more at offset 1024, where the fp32 restatement (variance about the mean) is unaffected."""
    from test_gpu_kernels import REL_L2
    zero, zrow = torch.zeros(D), torch.zeros(64, D)
    rel = {}
    for fam in ("plain", "offset256", "offset1024"):
        x = nc.make(fam, 64, D)
        truth, mag = nc.norm_modulate_op(x, "layer", 1e-6, zero, zrow, zero, zrow)
        rel[fam] = _rel(nc.one_pass_layernorm(x, 1e-6), truth)
        good = nc.restate(nc.norm_modulate_op, x, "layer", 1e-6, zero, zrow, zero, zrow)
        assert _rel(good, truth) <= REL_L2
    print(D, rel)
    assert rel["plain"] <= REL_L2 and rel["offset256"] <= REL_L2
    assert rel["offset1024"] > 4 * REL_L2


def test_metrics_see_what_the_whole_tensor_figures_miss():
    """A wrong small channel next to outlier channels, a statistic taken from the neighbouring row, and a dropped eps: each
    passes ``check`` or nearly, and each fails ``compare``."""
    D, rows = 2048, 41
    zero, zrow = torch.zeros(D), torch.zeros(rows, D)
    x = nc.make("outliers", rows, D)
    truth, mag = nc.norm_modulate_op(x, "rms", 1e-6, zero, zrow, zero, zrow)
    bad = truth.clone()
    bad[:, 5] *= 1.5                                          # a small channel, 50 % wrong
    from test_gpu_kernels import check
    check(bad.to(nc.BF), truth)                               # the whole-tensor figures stay green
    assert nc.figures(bad.to(nc.BF), truth, mag)["element"] > 10
    x = nc.make("row_scales", rows, D)
    truth, mag = nc.norm_modulate_op(x, "rms", 1e-6, zero, zrow, zero, zrow)
    xf = x.double()
    rstd = torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-6)
    with pytest.raises(AssertionError):
        nc.compare((xf * rstd.roll(1, 0)).to(nc.BF), truth, mag)         # the neighbour's factor
    x = nc.make("tiny", rows, D)
    truth, mag = nc.norm_modulate_op(x, "rms", 1e-6, zero, zrow, zero, zrow)
    xf = x.double()
    no_eps = xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-30)
    with pytest.raises(AssertionError):
        nc.compare(no_eps.to(nc.BF), truth, mag)
