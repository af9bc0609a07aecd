"""CPU pins of tests/conv_cases.py: the slack is what the module says it measured, the fp32 restatement meets every metric on
every (family, epilogue, K) the GPU file uses, the exact family's truths are small integers, the truth's indexing equals an
element-by-element loop in every mode, every GPU case is headed for the route it names, and the product's own layer shapes
take the routes of one table (a change to conv3d_plan's model shows up there)."""
import pytest
import torch

import conv_cases as cc


def test_slack_is_the_measured_excess():
    worst = cc.measure_excess()
    assert set(worst) == set(cc.MEASURED_EXCESS_BY_EPI)
    for epi, m in worst.items():
        rec = cc.MEASURED_EXCESS_BY_EPI[epi]
        print(f"{epi}: measured {m:.3e} ({m / 2.0 ** -24:.2f} x 2^-24), recorded {rec:.3e}")
        assert m <= rec <= 1.25 * m, (epi, m, rec)
    assert cc.MEASURED_EXCESS == max(cc.MEASURED_EXCESS_BY_EPI.values())
    assert cc.SLACK == 4.0 * cc.MEASURED_EXCESS


def test_slack_cases_cover_the_gpu_cases():
    used = {cc.slack_key(c) for c in cc.GPU_CASES if c["family"] != "exact"}
    assert used <= set(cc.SLACK_CASES)
    assert {k for _, _, k in used} >= {9 * 64, 27 * 64, 27 * 128, 27 * 192, 27 * 512, 27 * 1024}
    assert len({cc.case_id(c) for c in cc.GPU_CASES}) == len(cc.GPU_CASES)
    # every route, every epilogue of the four-wave form, 2 / 3 / 4 channel ranges, every instantiation of the finalising pass,
    # rows along H with and without the split
    wants = [tuple(c["want"].values()) for c in cc.GPU_CASES]
    assert {w[0] for w in wants} == {0, 1, 2, 3}
    assert {w[1] for w in wants if w[0] == 3} == set(range(7)) and {w[1] for w in wants if w[0] != 3} == {0, 1, 2}
    assert {w[2] for w in wants} == {1, 2, 3, 4} and {w[4] for w in wants} == {0, 2, 4, 8, 12, 16}
    assert {(w[2] > 1, w[3]) for w in wants if w[0] == 3} == {(False, 0), (False, 1), (True, 0), (True, 1)}


@pytest.mark.parametrize("family,epi,K", cc.SLACK_CASES, ids=lambda v: str(v))
def test_fp32_restatement_meets_every_metric(family, epi, K):
    assert (family, epi) not in cc.DROPPED
    c = cc.slack_case(family, epi, K)
    for t in cc.make(c).values():
        if torch.is_tensor(t):
            assert bool(torch.isfinite(t.float()).all())
    for name, r, t, mag in cc.restated_outputs(c):
        cc.compare(r, t, mag, what=f"restate {family} {epi} K{K} {name}")


def test_dropped_list():
    assert cc.DROPPED == {}
    assert len({e for _, e in cc.DROPPED}) == len(cc.DROPPED)          # at most one family per epilogue
    assert not any(f == "exact" for f, _ in cc.DROPPED)


_EXACT = {cc._input_key(c): c for c in cc.GPU_CASES if c["family"] == "exact"}


@pytest.mark.parametrize("c", list(_EXACT.values()), ids=cc.case_id)
def test_exact_family_truth_is_small_integers(c):
    """The condition under which the GPU output must equal the truth bit for bit -- and every (tap, 32-channel chunk) of the
    weights is non-zero within every 128-row block, so that no chunk can be dropped unseen."""
    d = cc.make(c)
    t, _ = cc.truth(c)
    if c["norm"] == "only":                                   # (the raw result is not an output: the integers feed the norm)
        t = cc.conv_op(d, c, cc.F32)[0]
    assert cc.exact_ok(t), float(t.abs().max())
    assert torch.equal(t.to(cc.BF).to(t.dtype), t)
    if c["judge"] == "whole" and t.numel() * c["Cin"] <= 2 ** 28:
        assert torch.equal(cc.conv_op(d, c, cc.F64)[0], t.double())              # fp32 was exact
    w = d["w"].float().view(c["Cout"], 9 * c["kernel_t"], c["Cin"] // 32, 32).abs().sum(-1)
    for n0 in range(0, c["Cout"], 128):
        assert bool((w[n0:n0 + 128].sum(0) > 0).all()), (n0, "a (tap, chunk) without a weight")


def test_cancel_family_cancels():
    """Every element is below 2^-8 of its sum of magnitudes, and an epilogue that rounds to bf16 before it adds is caught by
    the per-element metric."""
    c = cc.slack_case("cancel", "add", 27 * 128)
    d = cc.make(c)
    t, mag = cc.truth(c)
    assert float((t.abs() / mag).max()) <= 2.0 ** -8
    early = cc.conv_op(dict(d, add=None), dict(c, epi="none"), cc.F32)[0].to(cc.BF).float()
    with pytest.raises(AssertionError):
        cc.compare((early + d["add"].float()).to(cc.BF), t, mag, what="rounded early")


# ------------------------------------------------------------------------------------------- the truth's own indexing
def _naive(d, c):
    """include/ltxmi.h by index arithmetic: one dot product over the input channels per (output position, tap)."""
    x, kt = d["x"].double(), c["kernel_t"]
    B, T, H, W, cin = x.shape
    w = d["w"].double().view(c["Cout"], kt, 3, 3, cin)
    st, sh, _ = c["stride"]
    front, _, oT, oH, oW = cc.geometry(c)
    y = torch.zeros(B, oT, oH, oW, c["Cout"], dtype=torch.float64)
    mag = torch.zeros_like(y)
    for b in range(B):
        for t in range(oT):
            for h in range(oH):
                for v in range(oW):
                    for a in range(kt):
                        ti = t * st + a - front
                        if c["tzero"] and not 0 <= ti < T:
                            continue
                        ti = min(max(ti, 0), T - 1)
                        for i in range(3):
                            for j in range(3):
                                hi, wi = h * sh + i - 1, v * sh + j - 1
                                if not c["replicate"] and not (0 <= hi < H and 0 <= wi < W):
                                    continue
                                row = x[b, ti, min(max(hi, 0), H - 1), min(max(wi, 0), W - 1)]
                                y[b, t, h, v] += w[:, a, i, j] @ row
                                mag[b, t, h, v] += w[:, a, i, j].abs() @ row.abs()
    if d["bias"] is not None:
        y, mag = y + d["bias"].double(), mag + d["bias"].double().abs()
    if c["epi"].startswith("d2s"):
        cp = c["Cout"] // 8
        out, omag = (torch.zeros(B, 2 * T - 1, 2 * H, 2 * W, cp, dtype=torch.float64) for _ in range(2))
        for t in range(T):
            for h in range(H):
                for v in range(W):
                    for p in range(8):
                        to = 2 * t + (p >> 2) - 1
                        if to < 0:
                            continue                                      # the first upsampled frame is dropped
                        val, m = y[:, t, h, v, p * cp:(p + 1) * cp].clone(), mag[:, t, h, v, p * cp:(p + 1) * cp].clone()
                        if c["epi"] == "d2s_res":
                            for k in range(cp):
                                r = x[:, t, h, v, (k % (cin // 8)) * 8 + p]
                                val[:, k] += r
                                m[:, k] += r.abs()
                        out[:, to, 2 * h + ((p >> 1) & 1), 2 * v + (p & 1)] = val
                        omag[:, to, 2 * h + ((p >> 1) & 1), 2 * v + (p & 1)] = m
        y, mag = out, omag
    if d["add"] is not None:
        y, mag = y + d["add"].double(), mag + d["add"].double().abs()
    return y, mag


_MODES = [dict(causal=ca, replicate=r) for ca in (True, False) for r in (True, False)] + [
    dict(causal=False, replicate=False, tzero=True), dict(causal=True, replicate=True, tzero=True),
    dict(stride=(2, 1, 1)), dict(stride=(1, 2, 2), replicate=False), dict(stride=(2, 2, 2), grid=(1, 4, 4, 6)),
    dict(tpad=3, out_T=4), dict(causal=False, tpad=2, out_T=4, replicate=False), dict(kernel_t=1, causal=False),
    dict(kernel_t=1, causal=False, stride=(1, 2, 2), replicate=False), dict(epi="add", causal=False),
    dict(epi="d2s", cout=32), dict(epi="d2s_res", cout=128, causal=False, replicate=False), dict(bias=False)]


@pytest.mark.parametrize("mode", _MODES, ids=lambda m: "-".join(f"{k}{v}" for k, v in m.items()))
def test_truth_indexing_equals_a_naive_loop(mode):
    mode = dict(mode)
    c = cc._case(mode.pop("grid", (2, 3, 3, 5)), 64, mode.pop("cout", 8), (0, 0, 1, 0, 0), family="plain", **mode)
    d = cc.make(c)
    got, mag = cc.conv_op(d, c)
    want, wmag = _naive(d, c)
    assert got.shape == want.shape == cc.out_shape(c)
    assert float(((got - want).abs() / wmag).max()) <= 1e-12 and float(((mag - wmag).abs() / wmag).max()) <= 1e-12


def test_crops_are_the_full_truth():
    """The corner crops of the big cases give the values of the full-tensor truth at the positions they name."""
    for c in (cc._case((1, 7, 14, 23), 64, 8, (0, 0, 1, 0, 0), family="plain", causal=False, epi="add"),
              cc._case((1, 7, 27, 45), 64, 8, (0, 0, 1, 0, 0), family="plain", stride=(1, 2, 2), replicate=False),
              cc._case((1, 13, 14, 23), 64, 8, (0, 0, 1, 0, 0), family="plain", stride=(2, 1, 1)),
              cc._case((1, 7, 14, 23), 64, 8, (0, 0, 1, 0, 0), family="plain", kernel_t=1, causal=False),
              cc._case((1, 7, 14, 23), 64, 64, (0, 0, 1, 0, 0), family="plain", epi="d2s_res")):
        d = cc.make(c)
        full, fmag = cc.conv_op(d, c)
        for sl in cc.crops(c):
            t, mag, sel = cc.crop_truth(c, d, sl)
            assert t.numel() > 0 and t.shape == full[sel].shape
            assert float(((t - full[sel]).abs() / fmag[sel]).max()) <= 1e-12 and float(((mag - fmag[sel]).abs() / mag).max()) <= 1e-12


# ----------------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("c", cc.GPU_CASES, ids=cc.case_id)
def test_every_gpu_case_names_its_route(c):
    from ltxmi import ops
    kw, _ = cc.call_args(c, cc.empty_inputs(c), launch=False)
    r = ops.conv3d_route(**kw)
    assert isinstance(r, dict), r
    assert not r.pop("second_launch") and r == c["want"]
    if c["want"]["ksplit"] > 1:                                # the workspace is exactly what the split asks for
        kw["workspace"] = kw["workspace"][:-16]
        assert ops.conv3d_route(**kw)["ksplit"] == 1
    if c["versus"] is not None:
        other = ops.conv3d_route(**cc.call_args(c, cc.empty_inputs(c), launch=False, algo=c["versus"])[0])
        assert other["route"] != r["route"], other


# The product's own layers: (what, (B, T, H, W), Cin, Cout, keywords of _case, (route, epilogue, ksplit, swap_hw,
# finalize_blocks[, a note where ops.conv3d runs the norm as a launch of its own])) with algo 0 and the workspace ops.conv3d
# gives.  Decoder: the 0.9.5 decoder on a 13 x 16 x 24 latent
# (profiles/r04_vae_layers.log); encoder: its strided and SpaceToDepthDownsample convolutions on 97 x 512 x 768 pixels
# patchified by 4; upsampler: LatentUpsampler's per-frame and zero-padded convolutions on the same latent.
PRODUCT_ROUTES = [
    ("dec conv_in", (1, 13, 16, 24), 128, 1024, {}, (2, 0, 1, 0, 0)),
    ("dec 1024 conv1 + norm", (1, 13, 16, 24), 1024, 1024, dict(norm="only"), (3, 6, 3, 1, 4)),
    ("dec 1024 conv2 + add", (1, 13, 16, 24), 1024, 1024, dict(epi="add"), (3, 6, 3, 1, 4)),
    ("dec 1024 conv2 + add + next norm", (1, 13, 16, 24), 1024, 1024, dict(epi="add", norm="second"), (3, 6, 3, 1, 4)),
    ("dec 1024 -> 4096 d2s + next norm", (1, 13, 16, 24), 1024, 4096, dict(epi="d2s_res", norm="second"), (3, 6, 3, 1, 16)),
    ("dec 512 conv1 + norm", (1, 25, 32, 48), 512, 512, dict(norm="only"), (3, 6, 2, 0, 2)),
    ("dec 512 conv2 + add", (1, 25, 32, 48), 512, 512, dict(epi="add"), (2, 1, 1, 0, 0)),
    ("dec 512 -> 2048 d2s + next norm", (1, 25, 32, 48), 512, 2048, dict(epi="d2s_res", norm="second"), (3, 2, 1, 0, 0, "norm as a second launch")),
    ("dec 256 conv1", (1, 49, 64, 96), 256, 256, {}, (3, 0, 1, 0, 0)),
    ("dec 256 conv2 + add", (1, 49, 64, 96), 256, 256, dict(epi="add"), (3, 1, 1, 0, 0)),
    ("dec 256 -> 1024 d2s + next norm", (1, 49, 64, 96), 256, 1024, dict(epi="d2s_res", norm="second"), (3, 5, 1, 0, 0)),
    ("dec 128 conv1 + norm", (1, 97, 128, 192), 128, 128, dict(norm="only"), (3, 3, 1, 0, 0)),
    ("dec 128 conv2 + add + next norm", (1, 97, 128, 192), 128, 128, dict(epi="add", norm="second"), (3, 4, 1, 0, 0)),
    ("dec conv_out", (1, 97, 128, 192), 128, 48, {}, (2, 0, 1, 0, 0)),
    ("enc compress_all 128 -> 256", (1, 97, 128, 192), 128, 256, dict(stride=(2, 2, 2)), (1, 0, 1, 0, 0)),
    ("enc compress_space 256 -> 512", (1, 49, 64, 96), 256, 512, dict(stride=(1, 2, 2)), (1, 0, 1, 0, 0)),
    ("enc compress_time 512 -> 512", (1, 49, 32, 48), 512, 512, dict(stride=(2, 1, 1)), (0, 0, 1, 0, 0)),
    ("enc space-to-depth conv 128 -> 32", (1, 97, 128, 192), 128, 32, dict(tpad=3, out_T=98), (0, 0, 1, 0, 0)),
    ("up per-frame 512 -> 512", (13, 1, 32, 48), 512, 512, dict(kernel_t=1, causal=False, replicate=False), (0, 0, 1, 0, 0)),
    ("up per-frame 512 -> 2048", (13, 1, 32, 48), 512, 2048, dict(kernel_t=1, causal=False, replicate=False), (1, 0, 1, 0, 0)),
    ("up 3d 512 -> 512", (1, 13, 32, 48), 512, 512, dict(tzero=True, causal=False, replicate=False), (2, 0, 1, 0, 0)),
    ("up 3d 128 -> 512", (1, 13, 16, 24), 128, 512, dict(tzero=True, causal=False, replicate=False), (0, 0, 1, 0, 0)),
]


@pytest.mark.parametrize("row", PRODUCT_ROUTES, ids=lambda r: r[0])
def test_product_shapes_take_the_routes_of_the_table(row):
    from ltxmi import ops
    what, grid, cin, cout, kw, want = row
    c = cc._case(grid, cin, cout, want[:5], **kw)
    args, _ = cc.call_args(c, cc.empty_inputs(c), launch=False)
    del args["workspace"]                                       # ops.conv3d's own: what ltxmi_conv3d_workspace_bytes asks for
    r = ops.conv3d_route(**args)
    assert isinstance(r, dict), (what, r)
    assert r.pop("second_launch") == (len(want) > 5) and r == c["want"], (what, r)
