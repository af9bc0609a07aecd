"""The VAE with spatial_padding_mode = "reflect" on a real MI355X against the CPU oracle (which hands the mode to F.pad):
decode at two widths with the convolutions chosen by shape and through the implicit GEMM, encode, hw-tiled decode, a checkpoint
whose config says "reflect" loaded from disk -- under the parity bounds of tests/test_gpu_model.py, whose helpers these are --
and the same weights decoded under "replicate", which the reflect oracle must tell apart."""
import functools
import json
import os

import pytest
import torch

from test_gpu_model import BF, DEV, RTOL, assert_parity, build_vae, rel, vae_case

pytestmark = pytest.mark.gpu
TS = torch.tensor([0.05])


def _bf(sd):
    return {k: (v.to(BF) if v.is_floating_point() and v.dim() > 0 else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _case(base, with_encoder=False):
    cfg, sd = vae_case("b", base=base, with_encoder=with_encoder)
    assert cfg["spatial_padding_mode"] == "replicate"           # the weights do not depend on the mode
    return dict(cfg, spatial_padding_mode="reflect"), sd


@functools.lru_cache(maxsize=None)
def _decode_oracles(base, shape, seed):
    """(z, fp32 truth, the oracle in bf16) of one decode -- computed once, shared by the tests that judge against it."""
    from oracle import vae as ov
    cfg, sd = _case(base)
    z = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(BF)
    return z, ov.vae_decode(sd, cfg, z.float(), TS), ov.vae_decode(_bf(sd), cfg, z, TS)


def _decode(v, z):
    import ltxmi
    return ltxmi.vae_decode(z.to(DEV), v, True, vae_per_channel_normalize=True, timestep=TS.to(DEV))


def _all_reflect(v):
    from ltxmi import autoencoder, ops
    convs = [m for m in v.modules() if isinstance(m, autoencoder.CausalConv3d)]
    return len(convs) > 0 and {m.pad_mode for m in convs} == {ops.PAD_REFLECT}


@pytest.mark.parametrize("algo", [0, 1], ids=["by-shape", "implicit-gemm"])
@pytest.mark.parametrize("base,shape,seed", [(64, (1, 128, 3, 4, 5), 9), (128, (1, 128, 3, 6, 8), 19)], ids=["base64", "base128"])
def test_vae_decode_reflect(base, shape, seed, algo, monkeypatch):
    from ltxmi import ops
    cfg, sd = _case(base)
    z, truth, eager = _decode_oracles(base, shape, seed)
    v = build_vae(cfg, sd)
    assert _all_reflect(v)
    monkeypatch.setattr(ops, "CONV_ALGO", algo)
    out = _decode(v, z)
    assert out.shape == truth.shape == (1, 3, 17, shape[3] * 32, shape[4] * 32)
    assert_parity(out, truth, eager, f"vae decode reflect, base {base}, algo {algo}")


def test_replicate_decode_is_told_apart_by_the_reflect_oracle():
    """The same weights under "replicate": the two decodes differ, most in the frame border, and the replicate one misses the
    parity bound against the reflect oracle that the reflect one meets -- a convolution that quietly replicated would fail
    every test of this file."""
    cfg, sd = _case(64)
    z, truth, eager = _decode_oracles(64, (1, 128, 3, 4, 5), 9)
    refl = _decode(build_vae(cfg, sd), z)
    repl = _decode(build_vae(dict(cfg, spatial_padding_mode="replicate"), sd), z)
    e_refl, e_repl, e_ref = rel(refl, truth), rel(repl, truth), rel(eager, truth)
    diff = (refl.float() - repl.float()).abs().cpu()[0].mean((0, 1))              # [H, W]
    band = torch.ones_like(diff, dtype=torch.bool)
    band[16:-16, 16:-16] = False
    print(f"reflect vs its oracle {e_refl:.3e} (bf16 oracle {e_ref:.3e}); replicate vs the reflect oracle {e_repl:.3e}; "
          f"mean |reflect - replicate| in the 16-pixel border {float(diff[band].mean()):.3e}, inside {float(diff[~band].mean()):.3e}")
    assert e_refl <= e_ref + RTOL < e_repl
    assert float(diff[band].mean()) > float(diff[~band].mean()) > 0.0


def test_vae_encode_reflect():
    from oracle import vae_encoder as oe
    import ltxmi
    cfg, sd = _case(64, with_encoder=True)
    x = (torch.rand(1, 3, 9, 64, 96, generator=torch.Generator().manual_seed(12)) * 2 - 1).to(BF)
    truth = oe.encode(sd, cfg, x.float())                                    # moments [1, 256, 2, 2, 3]
    eager = oe.encode(_bf(sd), cfg, x)
    v = build_vae(cfg, sd)
    assert _all_reflect(v.encoder)
    dist = v.encode(x.to(DEV)).latent_dist
    assert isinstance(dist, ltxmi.DiagonalGaussianDistribution)
    out = dist.parameters
    assert out.shape == truth.shape == (1, 256, 2, 2, 3) and bool(torch.isfinite(out).all())
    e_ours, e_ref = rel(out, truth), rel(eager, truth)
    e_repl = rel(oe.encode(sd, dict(cfg, spatial_padding_mode="replicate"), x.float()), truth)
    print(f"vae encode reflect: ours {e_ours:.3e}  reference-bf16-eager {e_ref:.3e}  (the replicate oracle: {e_repl:.3e})")
    assert e_ours <= e_ref + RTOL, (e_ours, e_ref)
    assert e_repl > e_ref + RTOL                                             # the bound tells the modes apart


def test_vae_hw_tiled_decode_reflect():
    """Tiles are padded on their own, as in the reference: every tile mirrors at its own edges.  128-pixel tiles (4 latent
    positions, a new tile every 3) on a 5 x 8 latent: tiles of 4 and 2 rows, 4, 4 and 2 columns -- none a single row or column,
    which reflect padding refuses here as in torch (with 64-pixel tiles the last tile of every grid is one)."""
    from oracle import vae as ov
    cfg, sd = _case(64)
    v = build_vae(cfg, sd)
    z = torch.randn(1, 128, 2, 5, 8, generator=torch.Generator().manual_seed(11)).to(BF)
    truth = ov.decode(sd, cfg, z.float(), TS, use_hw_tiling=True, tile_sample_min_size=128)
    eager = ov.decode(_bf(sd), cfg, z, TS, use_hw_tiling=True, tile_sample_min_size=128)
    v.set_tiling_params(sample_size=128, overlap_factor=0.25)
    v.enable_hw_tiling()
    out = v.decode(z.to(DEV), return_dict=False, target_shape=(1, 3, 9, 160, 256), timestep=TS.to(DEV))[0]
    v.disable_hw_tiling()
    assert out.shape == truth.shape
    assert_parity(out, truth, eager, "hw-tiled decode, reflect")


def test_checkpoint_whose_config_says_reflect(tmp_path):
    from safetensors.torch import save_file
    from oracle import vae as ov
    import ltxmi
    cfg, sd = _case(64)
    path = os.path.join(tmp_path, "vae_reflect.safetensors")
    save_file({"vae." + k: v.contiguous() for k, v in _bf(sd).items()}, path, metadata={"config": json.dumps({"vae": cfg})})
    v = ltxmi.CausalVideoAutoencoder.from_pretrained(path, device=DEV).eval()
    v.decoder.timestep_scale_multiplier.data = v.decoder.timestep_scale_multiplier.data.float()
    assert _all_reflect(v)
    z = torch.randn(1, 128, 2, 3, 4, generator=torch.Generator().manual_seed(32)).to(BF)
    truth = ov.vae_decode(sd, cfg, z.float(), TS)
    eager = ov.vae_decode(_bf(sd), cfg, z, TS)
    assert_parity(_decode(v, z), truth, eager, "VAE loaded from a checkpoint whose config says reflect")
