"""CPU pins of tests/conv_reflect_cases.py and of the reflect mode's host side: the reflect truth's indexing equals an
element-by-element loop and torch's own nn.Conv3d(padding_mode="reflect"); it equals the replicate and the zeros truth in the
interior and differs from both on the border (or a case could not tell the modes apart); the exact family's truths stay small
integers; every case takes the route of its replicate twin; the two new refusals of the entry check; the modules accept the
mode."""
import ctypes

import pytest
import torch

import conv_cases as cc
import conv_reflect_cases as rc


def _mirror(i, n):
    return -i if i < 0 else (2 * n - 2 - i if i >= n else i)


def _naive(d, c):
    """include/ltxmi.h with pad_replicate = 2 by index arithmetic (plain store): -1 reads 1, L reads L - 2, each axis alone."""
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
                        ti = min(max(ti, 0), T - 1)                         # the time axis is never mirrored
                        for i in range(3):
                            for j in range(3):
                                row = x[b, ti, _mirror(h * sh + i - 1, H), _mirror(v * sh + j - 1, W)]
                                y[b, t, h, v] += w[:, a, i, j] @ row
                                mag[b, t, h, v] += w[:, a, i, j].abs() @ row.abs()
    if d["bias"] is not None:
        y, mag = y + d["bias"].double(), mag + d["bias"].double().abs()
    if d["add"] is not None:
        y, mag = y + d["add"].double(), mag + d["add"].double().abs()
    return y, mag


_MODES = [dict(causal=True), dict(causal=False), dict(causal=False, tzero=True), dict(causal=True, tzero=True),
          dict(grid=(2, 2, 2, 2)), dict(grid=(1, 2, 2, 5), causal=False), dict(stride=(2, 1, 1)), dict(stride=(1, 2, 2)),
          dict(stride=(2, 2, 2), grid=(1, 4, 4, 6)), dict(stride=(2, 2, 2), grid=(1, 5, 5, 7)), dict(tpad=3, out_T=4),
          dict(kernel_t=1, causal=False), dict(epi="add", causal=False), dict(bias=False)]


@pytest.mark.parametrize("mode", _MODES, ids=lambda m: "-".join(f"{k}{v}" for k, v in m.items()) or "default")
def test_reflect_truth_indexing_equals_a_naive_loop(mode):
    mode = dict(mode)
    c = cc._case(mode.pop("grid", (2, 3, 3, 5)), 64, 8, (0, 0, 1, 0, 0), family="plain", **mode)
    d = rc.make(c)
    got, mag = rc.conv_op(d, c)
    want, wmag = _naive(d, c)
    assert got.shape == want.shape == cc.out_shape(c)
    assert float(((got - want).abs() / wmag).max()) <= 1e-12 and float(((mag - wmag).abs() / wmag).max()) <= 1e-12


@pytest.mark.parametrize("causal", [True, False])
def test_reflect_truth_is_torchs_conv3d_padding_mode(causal):
    """What the reference runs: nn.Conv3d(padding=(0, 1, 1), padding_mode="reflect") on the time-padded input."""
    c = cc._case((2, 4, 5, 7), 64, 8, (0, 0, 1, 0, 0), family="plain", causal=causal)
    d = rc.make(c)
    conv = torch.nn.Conv3d(64, 8, 3, padding=(0, 1, 1), padding_mode="reflect").double()
    with torch.no_grad():
        conv.weight.copy_(d["w"].double().view(8, 3, 3, 3, 64).permute(0, 4, 1, 2, 3))
        conv.bias.copy_(d["bias"].double())
        x = d["x"].double().permute(0, 4, 1, 2, 3)
        x = torch.cat([x[:, :, :1]] * (2 if causal else 1) + [x] + ([] if causal else [x[:, :, -1:]]), dim=2)
        want = conv(x).permute(0, 2, 3, 4, 1)
    got, mag = rc.conv_op(d, c)
    assert float(((got - want).abs() / mag).max()) <= 1e-12


def test_the_old_modes_through_this_module_are_conv_cases_own():
    """``_conv`` with "replicate" / "zeros" is conv_cases._conv: the three modes stand side by side in one piece of code."""
    for kw in (dict(), dict(causal=False, tzero=True), dict(stride=(2, 2, 2)), dict(kernel_t=1, causal=False), dict(epi="d2s_res", cout=64)):
        kw = dict(kw)
        for repl in (True, False):
            c = cc._case((2, 3, 5, 7), 64, kw.pop("cout", 8), (0, 0, 1, 0, 0), family="plain", **dict(kw, replicate=repl))
            d = cc.make(c)
            for a, b in zip(rc.conv_op(d, c, pad="replicate" if repl else "zeros"), cc.conv_op(d, c)):
                assert torch.equal(a, b)


# one case per geometry: the modes' footprint does not depend on the family (the exact one where the geometry has it)
_GEOMETRY = {}
for _c in rc.GPU_CASES:
    _k = tuple((k, v) for k, v in cc._input_key(_c) if k != "family")
    if _k not in _GEOMETRY or _c["family"] == "exact":
        _GEOMETRY[_k] = _c


@pytest.mark.parametrize("c", list(_GEOMETRY.values()), ids=rc.case_id)
def test_reflect_differs_from_the_old_modes_on_the_border_only(c):
    d = dict(rc.make(c), add=None)                                   # (the raw convolution: `add` and a norm act per position)
    cr = dict(c, norm=None, epi="none" if c["epi"] == "add" else c["epi"])
    dt = cc.F32 if c["family"] == "exact" else cc.F64
    refl = rc.conv_op(d, cr, dt)[0]
    border = rc.border_mask(cr)
    assert border.shape == refl.shape[1:4]
    assert bool(border.any())
    for pad in ("replicate", "zeros"):
        other = rc.conv_op(d, cr, dt, pad=pad)[0]
        same = (refl == other).all(-1).all(0)                        # per output position, over samples and channels
        if c["H"] >= 3 and c["W"] >= 3:
            assert bool((~border).any()) and bool(same[~border].all()), f"{pad}: differs in the interior"
        assert not bool(same[border].any()), f"{pad}: a border position where the modes give the same values"


_EXACT = {cc._input_key(c): c for c in rc.GPU_CASES if c["family"] == "exact"}


@pytest.mark.parametrize("c", list(_EXACT.values()), ids=rc.case_id)
def test_exact_family_truth_is_small_integers_under_reflect(c):
    d = rc.make(c)
    t = rc.conv_op(d, c, cc.F32)[0]
    assert rc.exact_ok(t), float(t.abs().max())
    assert torch.equal(t.to(cc.BF).to(t.dtype), t)
    if t.numel() * c["Cin"] <= 2 ** 28:
        assert torch.equal(rc.conv_op(d, c, cc.F64)[0], t.double())              # fp32 was exact


def test_cases_cover_the_issue_and_the_slack():
    assert len({rc.case_id(c) for c in rc.GPU_CASES}) == len(rc.GPU_CASES)
    assert all(c["replicate"] for c in rc.GPU_CASES)
    used = {cc.slack_key(c) for c in rc.GPU_CASES if c["family"] != "exact"}
    assert used <= set(cc.SLACK_CASES), used - set(cc.SLACK_CASES)          # SLACK was measured on every (family, epilogue, K) used
    wants = [tuple(c["want"].values()) for c in rc.GPU_CASES]
    assert {w[0] for w in wants} == {0, 1, 2, 3}
    assert {w[1] for w in wants if w[0] == 3} == {0, 3, 4, 5, 6} and {w[1] for w in wants if w[0] in (0, 2)} == {0, 1, 2}
    assert {(w[2] > 1, w[3]) for w in wants if w[0] == 3} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    for route in range(4):                 # causal and not, and time_pad_zeros, on every kernel
        mine = [c for c in rc.GPU_CASES if c["want"]["route"] == route]
        assert {c["causal"] for c in mine} == {True, False} and any(c["tzero"] for c in mine), route
    assert any(c["tzero"] for c in rc.SPLIT_CASES) or {c["causal"] for c in rc.SPLIT_CASES} == {True, False}


def test_cancel_family_cancels_under_reflect():
    c = next(c for c in rc.GPU_CASES if c["family"] == "cancel")
    t, mag = rc.truth(c)
    assert float((t.abs() / mag).max()) <= 2.0 ** -8
    twin = cc.conv_op(cc.make(c), c)[0]                              # with the twin's `add` the reflect border would not cancel
    assert not torch.equal(rc.make(c)["add"], cc.make(c)["add"]) and twin.shape == t.shape


# ----------------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("c", rc.GPU_CASES, ids=rc.case_id)
def test_reflect_case_takes_the_route_of_its_replicate_twin(c):
    from ltxmi import ops
    kw, _ = rc.call_args(c, cc.empty_inputs(c), launch=False)
    assert kw["pad_replicate"] == ops.PAD_REFLECT == 2
    r = ops.conv3d_route(**kw)
    assert isinstance(r, dict), r
    twin = ops.conv3d_route(**dict(kw, pad_replicate=True))
    assert r == twin and ops.conv3d_route(**dict(kw, pad_replicate=ops.PAD_ZEROS)) == r
    assert not r.pop("second_launch") and r == c["want"]


def _abi_args(H, W, mode, cin=64, cout=8):
    from ltxmi import _lib
    a = _lib.Conv3dArgs()
    a.x, a.w, a.y, a.bias = 256, 512, 768, 1024                      # addresses only: nothing is dereferenced
    a.B, a.T, a.H, a.W, a.Cin, a.Cout, a.causal, a.pad_replicate = 1, 3, H, W, cin, cout, 1, mode
    return a


@pytest.mark.parametrize("H,W,mode,says", [(1, 5, 2, b"reflect"), (5, 1, 2, b"reflect"), (1, 1, 2, b"reflect"), (5, 7, 3, b"pad_replicate = 3"),
                                           (5, 7, -1, b"pad_replicate = -1"), (1, 1, 3, b"pad_replicate = 3")])
def test_entry_check_refuses_what_cannot_be_mirrored(H, W, mode, says):
    from ltxmi import _lib
    a, info = _abi_args(H, W, mode), _lib.Conv3dRouteInfo()
    assert _lib.lib.ltxmi_conv3d_route(ctypes.byref(a), ctypes.byref(info)) == -1            # LTXMI_ERR_INVALID_ARG, no device
    assert info.route == -1 and says in _lib.lib.ltxmi_last_error(), _lib.lib.ltxmi_last_error()
    assert _lib.lib.ltxmi_conv3d_ndhwc_bf16(ctypes.byref(a), None) == -1                     # the launch: the same check, first
    assert says in _lib.lib.ltxmi_last_error()


def test_entry_check_takes_the_three_modes_and_single_rows_in_the_old_ones():
    from ltxmi import _lib, ops
    for H, W, mode in ((5, 7, 0), (5, 7, 1), (5, 7, 2), (2, 2, 2), (1, 5, 1), (5, 1, 0), (1, 1, 1)):
        info = _lib.Conv3dRouteInfo()
        assert _lib.lib.ltxmi_conv3d_route(ctypes.byref(_abi_args(H, W, mode)), ctypes.byref(info)) == 0, (H, W, mode)
    # the mode chooses nothing: the queries answer alike for all three
    for grid, cin, cout, post in (((1, 13, 16, 24), 1024, 1024, 0), ((1, 25, 32, 48), 512, 512, 1), ((1, 97, 128, 192), 128, 128, 1)):
        seen = set()
        for mode in (0, 1, 2):
            a = _abi_args(grid[2], grid[3], mode, cin, cout)
            a.T, a.post_norm = grid[1], post
            seen.add((int(_lib.lib.ltxmi_conv3d_workspace_bytes(ctypes.byref(a))), int(_lib.lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)))))
        assert len(seen) == 1, (grid, seen)
    assert (ops.PAD_ZEROS, ops.PAD_REPLICATE, ops.PAD_REFLECT) == (0, 1, 2) and int(False) == ops.PAD_ZEROS and int(True) == ops.PAD_REPLICATE
    assert _lib.lib.ltxmi_version() == b"ltxmi 0.9.0"


# ----------------------------------------------------------------------------------------------------- modules
def test_causal_conv3d_takes_reflect_and_keeps_the_mode():
    import ltxmi
    from ltxmi import autoencoder, ops
    for name, mode, repl in (("zeros", ops.PAD_ZEROS, False), ("replicate", ops.PAD_REPLICATE, True), ("reflect", ops.PAD_REFLECT, False)):
        m = autoencoder.CausalConv3d(6, 10, 3, spatial_padding_mode=name)
        assert m.spatial_padding_mode == name and m.pad_mode == mode and m.pad_replicate is repl
    for bad in ("circular", "mirror", ""):
        with pytest.raises(NotImplementedError, match="zeros, replicate and reflect"):
            autoencoder.CausalConv3d(6, 10, 3, spatial_padding_mode=bad)
    assert autoencoder.make_conv_nd(3, 6, 10, 3, causal=True, spatial_padding_mode="reflect").pad_mode == ops.PAD_REFLECT
    assert ltxmi.CausalVideoAutoencoder is autoencoder.CausalVideoAutoencoder


def test_from_config_builds_with_reflect_in_every_convolution():
    import ltxmi
    from ltxmi import autoencoder, ops
    from oracle import vae as ov
    from oracle import vae_encoder as oe
    cfg = dict(ov.demo_config(128), spatial_padding_mode="reflect", decoder_base_channels=64, encoder_base_channels=64,
               build_encoder=True, encoder_blocks=oe.demo_encoder_blocks())
    vae = ltxmi.CausalVideoAutoencoder.from_config(cfg)
    convs = [m for m in vae.modules() if isinstance(m, autoencoder.CausalConv3d)]
    assert len(convs) > 10 and {m.pad_mode for m in convs} == {ops.PAD_REFLECT}
    assert any(m in set(vae.encoder.modules()) for m in convs) and any(m in set(vae.decoder.modules()) for m in convs)
    with pytest.raises(NotImplementedError):
        ltxmi.CausalVideoAutoencoder.from_config(dict(cfg, spatial_padding_mode="circular"))
