"""The temporal and spatial + temporal latent upsamplers on a real MI355X: ``ops.pixel_shuffle_nd`` (PixelShuffleND over
time and / or space with the first-frame trim in the store address) bit-exact against the oracle, and
``LatentUpsampler.forward`` / ``upsample_latents`` in both new modes against the oracle (latent_upsampler.py:83-97, 109-149;
pipeline_ltx_video.py:1760-1772).

Model tolerance: the project's parity rule (tests/test_gpu_model.py).  Our result and the reference's bf16 eager result are
two bf16 renderings of the same fp32 computation, so each is measured against the fp32 oracle ("truth") and

        err(ours) <= err(reference bf16 eager) + 2e-3          (relative L2 over the tensor)

where the reference's bf16 eager path is the oracle run with weights and input in bf16.
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
RTOL = 2e-3
SENTINEL = -12288.0                  # exact in bf16, far outside anything randn produces


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def assert_parity(out, truth, eager, what):
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite output"
    e_ours, e_ref = rel(out, truth), rel(eager, truth)
    print(f"{what}: rel L2 vs fp32 oracle: ours {e_ours:.3e} / reference-bf16-eager {e_ref:.3e}")
    assert e_ours <= e_ref + RTOL, (what, e_ours, e_ref)


# ------------------------------------------------------------------------ the shuffle kernel
SHUFFLES = [(2, 1, 1), (2, 2, 1), (2, 1, 0), (2, 2, 0), (1, 2, 0)]           # (pt, ps, drop_first)
SHAPES = [(2, 1, 3, 5, 8),          # one frame in: with drop_first one frame out, only the p1 = 1 half is ever stored
          (1, 3, 5, 7, 24),         # odd sizes, C not a power of two
          (2, 2, 4, 4, 64)]         # (B, T, H, W, C)


def _oracle_shuffle(x, pt, ps, drop):
    """x NCDHW [B, pt*ps*ps*C, T, H, W] in the reference's channel order (c p1 .. pn) -> [B, C, pt*T - drop, ps*H, ps*W]."""
    from oracle import upsampler as ou
    if pt == 2:
        return ou.pixel_shuffle(x, 3 if ps == 2 else 1)[:, :, drop:]
    B, C4, T, H, W = x.shape                                        # PixelShuffleND(2) works on folded frames
    y = ou.pixel_shuffle(x.permute(0, 2, 1, 3, 4).reshape(B * T, C4, H, W), 2)
    return y.view(B, T, C4 // 4, 2 * H, 2 * W).permute(0, 2, 1, 3, 4)[:, :, drop:]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pt,ps,drop", SHUFFLES)
def test_pixel_shuffle_nd_is_exact(pt, ps, drop, shape):
    from ltxmi import ops
    B, T, H, W, C = shape
    f = pt * ps * ps
    g = torch.Generator().manual_seed(1000 * pt + 100 * ps + 10 * drop + C)
    x = torch.randn(B, f * C, T, H, W, generator=g).to(BF)          # the reference's channel order (c p1 .. pn)
    truth = _oracle_shuffle(x, pt, ps, drop)
    To, Ho, Wo = pt * T - drop, ps * H, ps * W
    assert tuple(truth.shape) == (B, C, To, Ho, Wo)
    xp = x.view(B, C, f, T, H, W).transpose(1, 2).reshape(B, f * C, T, H, W)        # packed (p1 .. pn c)
    xd = xp.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    # the output sits in front of one guard frame; both start as the sentinel
    frame = Ho * Wo * C
    buf = torch.full(((B * To + 1) * frame,), SENTINEL, dtype=BF, device=DEV)
    out = buf[: B * To * frame].view(B, To, Ho, Wo, C)
    got = ops.pixel_shuffle_nd(xd, pt, ps, drop_first=bool(drop), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    host = buf.cpu()
    assert torch.equal(host[B * To * frame:], torch.full((frame,), SENTINEL, dtype=BF)), "guard frame was written"
    res = host[: B * To * frame].view(B, To, Ho, Wo, C).permute(0, 4, 1, 2, 3)
    assert torch.equal(res, truth)                                  # every value in place, so no sentinel is left either
    # the allocating form gives the same tensor
    assert torch.equal(ops.pixel_shuffle_nd(xd, pt, ps, drop_first=bool(drop)).cpu(), host[: B * To * frame].view(B, To, Ho, Wo, C))
    if (pt, ps, drop) == (1, 2, 0):
        assert torch.equal(ops.pixel_shuffle2d(xd).cpu().permute(0, 4, 1, 2, 3), truth)


def test_pixel_shuffle_nd_wrapper_checks():
    from ltxmi import ops
    x = torch.zeros(1, 2, 3, 5, 64, dtype=BF, device=DEV)
    for pt, ps, drop in [(1, 1, False), (3, 1, False), (2, 4, False), (1, 2, True)]:
        with pytest.raises(ValueError):
            ops.pixel_shuffle_nd(x, pt, ps, drop_first=drop)
    with pytest.raises(ValueError):
        ops.pixel_shuffle_nd(x[..., :24].contiguous(), 2, 2)        # 24 channels are not 8 * C with C % 8 == 0
    with pytest.raises(ValueError):
        ops.pixel_shuffle_nd(x[..., ::2], 2, 1)                     # not contiguous
    with pytest.raises(ValueError):
        ops.pixel_shuffle_nd(x, 2, 1, out=torch.empty(1, 4, 3, 5, 16, dtype=BF, device=DEV))       # shape of drop_first=False is [1,4,3,5,32]
    with pytest.raises(TypeError):
        ops.pixel_shuffle_nd(x.float(), 2, 1)


# ------------------------------------------------------------------------ the model, both new modes
WIDTHS = dict(in_channels=128, mid_channels=64, num_blocks_per_stage=2, dims=3)      # test_latent_upsampler_and_bridge's, dims 3
MODES = {"temporal": dict(WIDTHS, spatial_upsample=False, temporal_upsample=True),
         "spatial_temporal": dict(WIDTHS, spatial_upsample=True, temporal_upsample=True)}
LATENTS = [(1, 128, 3, 6, 10), (2, 128, 1, 4, 6)]


@functools.lru_cache(maxsize=None)
def _weights(mode):
    from oracle import upsampler as ou
    return {k: v.to(BF).float() for k, v in ou.init_state_dict(MODES[mode], seed=5).items()}         # bf16-representable


@functools.lru_cache(maxsize=None)
def _model(mode):
    import ltxmi
    m = ltxmi.LatentUpsampler.from_config(MODES[mode])
    m.load_state_dict(_weights(mode), strict=True)
    return m.to(device=DEV, dtype=BF).eval()


@functools.lru_cache(maxsize=None)
def _case(mode, shape):
    """(latent bf16, fp32 truth, the reference's bf16 eager rendering), computed once per (mode, shape)."""
    from oracle import upsampler as ou
    cfg, sd = MODES[mode], _weights(mode)
    g = torch.Generator().manual_seed(14 + shape[2])
    z = torch.randn(*shape, generator=g).to(BF)
    truth = ou.latent_upsampler_forward(sd, cfg, z.float())
    eager = ou.latent_upsampler_forward({k: v.to(BF) for k, v in sd.items()}, cfg, z)
    return z, truth, eager


@pytest.mark.parametrize("shape", LATENTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_latent_upsampler_temporal_modes(mode, shape):
    z, truth, eager = _case(mode, shape)
    b, c, f, h, w = shape
    want = (b, c, 2 * f - 1, 2 * h, 2 * w) if mode == "spatial_temporal" else (b, c, 2 * f - 1, h, w)
    m = _model(mode)
    with torch.no_grad():
        out = m(z.to(DEV))
    assert tuple(out.shape) == tuple(truth.shape) == want
    assert_parity(out, truth, eager, f"latent upsampler {mode} {list(shape)}")


def test_upsample_latents_with_a_temporal_upsampler():
    """_upsample_latents (:1760-1772): un_normalize -> upsampler -> normalize around the temporal mode, fp32 latents in and out."""
    import ltxmi
    from oracle import upsampler as ou
    mode, shape = "temporal", LATENTS[0]
    cfg, sd = MODES[mode], _weights(mode)
    z = _case(mode, shape)[0]
    g = torch.Generator().manual_seed(15)
    stats = {"per_channel_statistics.std-of-means": 0.5 + torch.rand(128, generator=g),
             "per_channel_statistics.mean-of-means": 0.2 * torch.randn(128, generator=g)}
    truth = ou.upsample_latents(sd, cfg, z.float(), stats)
    eager = ou.upsample_latents({k: v.to(BF) for k, v in sd.items()}, cfg, z, stats)
    vae = types.SimpleNamespace(std_of_means=stats["per_channel_statistics.std-of-means"].to(DEV),
                                mean_of_means=stats["per_channel_statistics.mean-of-means"].to(DEV))
    with torch.no_grad():
        got = ltxmi.upsample_latents(_model(mode), z.float().to(DEV), vae)
    b, c, f, h, w = shape
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(truth.shape) == (b, c, 2 * f - 1, h, w)
    assert_parity(got, truth, eager, "upsample_latents, temporal upsampler")


def test_in_place_weight_edit_rebuilds_the_packed_conv_weight():
    """``weight.mul_(0.5)`` on a ResBlock convolution between two runs: the second run is, bit for bit, that of a fresh model
    loaded from the edited state dict (the pack keys on the weight's version counter, ltxmi/derived.py), not the first run again."""
    import ltxmi
    from oracle import upsampler as ou
    cfg = dict(MODES["spatial_temporal"], num_blocks_per_stage=1)
    sd = {k: v.to(BF).float() for k, v in ou.init_state_dict(cfg, seed=6).items()}

    def load(state):
        m = ltxmi.LatentUpsampler.from_config(cfg)
        m.load_state_dict(state, strict=True)
        return m.to(device=DEV, dtype=BF).eval()
    z = torch.randn(1, 128, 3, 4, 4, generator=torch.Generator().manual_seed(16)).to(BF).to(DEV)
    m = load(sd)
    with torch.no_grad():
        first = m(z)
        m.res_blocks[0].conv1.weight.mul_(0.5)
        second = m(z)
        fresh = load({k: v.float().cpu() for k, v in m.state_dict().items()})(z)
    assert torch.equal(second, fresh)
    assert not torch.equal(second, first)
