"""G17 (tests/golden/g17_reflect.*, written by tools/make_golden_reflect.py from the reference's own modules with
spatial_padding_mode="reflect"): the CPU oracle, which hands the mode to F.pad unchanged, matches it at the tolerance of
tests/test_oracle_golden.py -- convolutions, blocks, one small Decoder and one small Encoder -- and the mode really acts."""
import json
import os

import pytest
import torch

from golden_cases import sub
from oracle import vae
from oracle import vae_encoder as ve
from test_oracle_golden import TOL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g17():
    from safetensors.torch import load_file
    with open(os.path.join(GOLDEN, "g17_reflect.json")) as f:
        meta = json.load(f)
    assert meta["mode"] == "reflect" and meta["vae_cfg"]["spatial_padding_mode"] == "reflect"
    return load_file(os.path.join(GOLDEN, "g17_reflect.safetensors")), meta


def test_g17_shares_the_inputs_of_g8_and_g11(g17, golden):
    t, meta = g17
    torch.testing.assert_close(t["x"], golden("g8_conv_blocks")[0]["x"], rtol=0, atol=0)
    torch.testing.assert_close(t["res.x"], golden("g8_conv_blocks")[0]["res.x"], rtol=0, atol=0)
    torch.testing.assert_close(t["enc_x"], golden("g11_encoder_blocks")[0]["x"], rtol=0, atol=0)
    assert all(list(t[k].shape) == s for k, s in meta["shapes"].items())
    assert os.path.getsize(os.path.join(GOLDEN, "g17_reflect.safetensors")) <= min(
        os.path.getsize(os.path.join(GOLDEN, "g10_decoder_b.safetensors")), 1 << 20)


def test_g17_convolutions(g17):
    t, _ = g17
    sd = sub(t, "conv.")
    for causal, name in ((True, "causal"), (False, "noncausal")):
        out = vae.causal_conv3d(t["x"], sd, "", causal, "reflect")
        torch.testing.assert_close(out, t[f"conv.{name}"], **TOL)
        for other in ("replicate", "zeros"):                    # the border, and only the border, knows the mode
            d = (vae.causal_conv3d(t["x"], sd, "", causal, other) - out).abs().amax((0, 1, 2))
            assert float(d[1:-1, 1:-1].max()) == 0.0 and float(d[0].min()) > 0 and float(d[-1].min()) > 0
            assert float(d[:, 0].min()) > 0 and float(d[:, -1].min()) > 0
    for name, stride in (("time", (2, 1, 1)), ("space", (1, 2, 2)), ("all", (2, 2, 2))):
        out = ve.strided_causal_conv3d(t["enc_x"], sub(t, f"sconv.{name}."), "", stride, "reflect")
        torch.testing.assert_close(out, t[f"sconv.{name}.out"], **TOL)
        blk = dict(stride=stride, group=8 * stride[0] * stride[1] * stride[2] // 16)
        out = ve.space_to_depth_downsample(t["enc_x"], sub(t, f"s2d.{name}.sd."), "", blk, "reflect")
        torch.testing.assert_close(out, t[f"s2d.{name}.out"], **TOL)


def test_g17_blocks(g17):
    t, _ = g17
    out = vae.resnet_block(t["res.x"], sub(t, "res.sd."), "", False, "reflect", t["res.temb"])
    torch.testing.assert_close(out, t["res.out"], **TOL)
    assert float((vae.resnet_block(t["res.x"], sub(t, "res.sd."), "", False, "replicate", t["res.temb"]) - out).abs().max()) > 1e-3
    blk = dict(stride=(2, 2, 2), residual=True, reduction=2)
    torch.testing.assert_close(vae.depth_to_space_upsample(t["res.x"], sub(t, "up.sd."), "", blk, False, "reflect"), t["up.out"], **TOL)
    blk = dict(stride=(2, 2, 2), residual=False, reduction=1)
    torch.testing.assert_close(vae.depth_to_space_upsample(t["res.x"], sub(t, "up2.sd."), "", blk, False, "reflect"), t["up2.out"], **TOL)


def test_g17_decoder_and_encoder(g17):
    t, meta = g17
    cfg = meta["vae_cfg"]
    out = vae.decoder_forward(sub(t, "dec.sd."), cfg, t["dec.z"], t["dec.timestep"])
    assert out.shape == t["dec.out"].shape == (1, 3, 3, 24, 32)
    torch.testing.assert_close(out, t["dec.out"], **TOL)
    other = vae.decoder_forward(sub(t, "dec.sd."), dict(cfg, spatial_padding_mode="replicate"), t["dec.z"], t["dec.timestep"])
    assert float((other - out).abs().max()) > 1e-3
    out = ve.encoder_forward(sub(t, "enc.sd."), cfg, t["enc.x"])
    assert out.shape == t["enc.out"].shape
    torch.testing.assert_close(out, t["enc.out"], **TOL)
    other = ve.encoder_forward(sub(t, "enc.sd."), dict(cfg, spatial_padding_mode="replicate"), t["enc.x"])
    assert float((other - out).abs().max()) > 1e-3
