"""The temporal and spatial + temporal modes of ``ltxmi.LatentUpsampler`` (latent_upsampler.py:83-97, 136-142), host side:
construction, the reference's key names and shapes, config round trips, ``from_pretrained`` from the metadata of a
safetensors file, the row packing that turns PixelShuffleND(n) into a copy of whole channel runs, and the argument checks
of ``ltxmi_pixel_shuffle_nd_ndhwc_bf16``.  Nothing here needs a device; the kernels are in tests/test_gpu_upsampler_modes.py.
"""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

BF = torch.bfloat16
SMALL = dict(in_channels=8, mid_channels=32, num_blocks_per_stage=1, dims=3)
MODES = {"temporal": dict(SMALL, spatial_upsample=False, temporal_upsample=True),
         "spatial_temporal": dict(SMALL, spatial_upsample=True, temporal_upsample=True)}
UPSAMPLER_ROWS = {"temporal": 2, "spatial_temporal": 8}          # Conv3d(mid, 2 mid) / Conv3d(mid, 8 mid)


@pytest.fixture(params=sorted(MODES))
def mode(request):
    return request.param


def test_constructs_with_the_reference_keys_and_shapes(mode):
    import ltxmi
    from oracle import upsampler as ou
    cfg = MODES[mode]
    m = ltxmi.LatentUpsampler.from_config(cfg)
    want = ou.init_state_dict(cfg)
    got = m.state_dict()
    assert set(got) == set(want)
    for k, v in want.items():
        assert tuple(got[k].shape) == tuple(v.shape), k
    mid = cfg["mid_channels"]
    assert tuple(got["upsampler.0.weight"].shape) == (UPSAMPLER_ROWS[mode] * mid, mid, 3, 3, 3)
    res = m.load_state_dict(want, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in want.items():
        assert torch.equal(m.state_dict()[k], v), k


def test_config_round_trips(mode):
    import ltxmi
    cfg = MODES[mode]
    m = ltxmi.LatentUpsampler.from_config(cfg)
    c = m.config()
    assert c == dict(cfg, _class_name="LatentUpsampler")
    m2 = ltxmi.LatentUpsampler.from_config(c)
    assert m2.config() == c
    assert {k: tuple(v.shape) for k, v in m2.state_dict().items()} == {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_from_pretrained_reads_the_mode_from_the_metadata(mode, tmp_path):
    import ltxmi
    from oracle import upsampler as ou
    from safetensors.torch import save_file
    cfg = MODES[mode]
    sd = ou.init_state_dict(cfg, seed=11)
    path = os.path.join(tmp_path, "temporal-upscaler.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, path, metadata={"config": json.dumps(cfg)})
    m = ltxmi.LatentUpsampler.from_pretrained(path, device="cpu")
    assert m.temporal_upsample is True and m.spatial_upsample is cfg["spatial_upsample"] and m.dims == 3
    assert m.config() == dict(cfg, _class_name="LatentUpsampler")
    assert not m.training and m.dtype == BF
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v.to(BF)), k


def test_flag_combinations_the_reference_cannot_run():
    import ltxmi
    with pytest.raises(NotImplementedError, match="dims=3"):
        ltxmi.LatentUpsampler(in_channels=8, mid_channels=32, num_blocks_per_stage=1, dims=2, spatial_upsample=False,
                              temporal_upsample=True)
    with pytest.raises(NotImplementedError, match="dims=3"):
        ltxmi.LatentUpsampler.from_config(dict(SMALL, dims=2, spatial_upsample=True, temporal_upsample=True))
    with pytest.raises(ValueError, match="spatial_upsample or temporal_upsample"):
        ltxmi.LatentUpsampler(in_channels=8, mid_channels=32, num_blocks_per_stage=1, dims=3, spatial_upsample=False,
                              temporal_upsample=False)


# ------------------------------------------------------------------------ row packing
def _shuffle_p_outermost(y, arity):
    """PixelShuffleND(arity) of a conv output whose channels are (p1 .. pn c) -- the p indices outermost, c fastest."""
    if arity == 3:
        B, C, D, H, W = y.shape
        c = C // 8
        return y.view(B, 2, 2, 2, c, D, H, W).permute(0, 4, 5, 1, 6, 2, 7, 3).reshape(B, c, 2 * D, 2 * H, 2 * W)
    if arity == 2:
        B, C, H, W = y.shape
        c = C // 4
        return y.view(B, 2, 2, c, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, c, 2 * H, 2 * W)
    B, C, D, H, W = y.shape
    c = C // 2
    return y.view(B, 2, c, D, H, W).permute(0, 2, 3, 1, 4, 5).reshape(B, c, 2 * D, H, W)


@pytest.mark.parametrize("arity", [1, 2, 3])
def test_packed_rows_make_the_shuffle_a_copy(arity):
    """conv with the packed rows + a shuffle with p outermost == conv with the original rows + PixelShuffleND(arity).
    Both sides use the bf16 cast of the weights (what ``packed`` returns) and run the same fp32 convolution; a row of the
    packed weight is a row of the original one, so each output value is the same sum of the same products and the two
    sides agree to fp32 round-off of the summation order: ``torch.allclose`` at its fp32 defaults (rtol 1e-5, atol 1e-8)."""
    from ltxmi.latent_upsampler import _ConvParams
    from oracle import upsampler as ou
    torch.manual_seed(20 + arity)
    dims = 2 if arity == 2 else 3
    cin, c = 8, 24
    cout = c * 2 ** arity
    conv = _ConvParams(cin, cout, dims)
    w, b = conv.packed(arity)
    assert w.dtype == b.dtype == BF and tuple(w.shape) == (cout, cin * 3 ** dims) and tuple(b.shape) == (cout,)
    assert w.is_contiguous() and b.is_contiguous()
    assert conv.packed(arity)[0] is w                                   # cached
    taps = (3,) * dims
    # tap-major [cout, taps..., cin] -> nn.Conv's [cout, cin, taps...]
    w_nn = w.float().view(cout, *taps, cin).permute(0, dims + 1, *range(1, dims + 1)).contiguous()
    conv_f = F.conv2d if dims == 2 else F.conv3d
    x = torch.randn(2, cin, 5, 7) if dims == 2 else torch.randn(2, cin, 3, 5, 7)
    ours = _shuffle_p_outermost(conv_f(x, w_nn, b.float(), padding=1), arity)
    ref = ou.pixel_shuffle(conv_f(x, conv.weight.detach().to(BF).float(), conv.bias.detach().to(BF).float(), padding=1), arity)
    assert ours.shape == ref.shape
    print(f"arity {arity}: max |ours - ref| = {float((ours - ref).abs().max()):.3e}")
    assert torch.allclose(ours, ref)
    # another arity is another pack, not the cached one
    other = 1 if arity != 1 else 3
    if cout % 2 ** other == 0:
        assert conv.packed(other)[0] is not w
        assert conv.packed(arity)[0] is not w and torch.equal(conv.packed(arity)[0], w)


def test_arity2_pack_is_the_pack_the_spatial_mode_always_had():
    """Rows (c p1 p2) -> (p1 p2 c): new row p*c_out + c is old row c*4 + p of the tap-major weight, then the bf16 cast."""
    from ltxmi.latent_upsampler import _ConvParams
    torch.manual_seed(7)
    cin, c = 16, 40
    conv = _ConvParams(cin, 4 * c, 2)
    w, b = conv.packed(2)
    rows = [ci * 4 + p for p in range(4) for ci in range(c)]
    tap_major = conv.weight.detach().permute(0, 2, 3, 1).reshape(4 * c, 9 * cin)
    assert torch.equal(w, tap_major[rows].to(BF))
    assert torch.equal(b, conv.bias.detach()[rows].to(BF))
    # and no shuffle at all leaves the rows where they are
    w0, b0 = conv.packed()
    assert torch.equal(w0, tap_major.to(BF)) and torch.equal(b0, conv.bias.detach().to(BF))


# ------------------------------------------------------------------------ the C entry's argument checks
def test_pixel_shuffle_nd_rejects_bad_arguments_without_a_device():
    """Every refusal comes back as LTXMI_ERR_INVALID_ARG before anything is launched (the pointers are never followed)."""
    from ltxmi import _lib
    lib = _lib.lib
    INVALID = -1
    buf = ctypes.create_string_buffer(4096 + 64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    fn = lib.ltxmi_pixel_shuffle_nd_ndhwc_bf16
    good = dict(x=p, y=p, B=1, T=2, H=3, W=5, C=8, pt=2, ps=2, drop_first=1)

    def call(**over):
        a = dict(good, **over)
        return fn(a["x"], a["y"], a["B"], a["T"], a["H"], a["W"], a["C"], a["pt"], a["ps"], a["drop_first"], None)

    bad = [dict(x=None), dict(y=None),
           dict(B=0), dict(T=0), dict(H=0), dict(W=0), dict(C=0), dict(B=-1), dict(T=-2), dict(H=-3), dict(W=-5), dict(C=-8),
           dict(C=12), dict(C=4), dict(C=20),
           dict(pt=0), dict(pt=3), dict(pt=4), dict(pt=-1), dict(ps=0), dict(ps=3), dict(ps=4), dict(ps=-2),
           dict(pt=1, ps=1, drop_first=0),
           dict(drop_first=2), dict(drop_first=-1),
           dict(pt=1, ps=2, drop_first=1)]
    for over in bad:
        assert call(**over) == INVALID, over
        assert b"ltxmi_pixel_shuffle_nd_ndhwc_bf16" in lib.ltxmi_last_error(), over
    assert b"drop_first" in lib.ltxmi_last_error()


def test_pixel_shuffle_nd_wrapper_has_no_cpu_path():
    from ltxmi import ops
    with pytest.raises(TypeError):
        ops.pixel_shuffle_nd(torch.zeros(1, 2, 3, 5, 16, dtype=BF), 2, 1, drop_first=True)
    with pytest.raises(TypeError):
        ops.pixel_shuffle_nd(torch.zeros(1, 2, 3, 5, 16), 2, 1)
