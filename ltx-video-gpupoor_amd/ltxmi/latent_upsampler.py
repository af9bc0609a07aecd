"""``LatentUpsampler`` + ``adain_filter_latent`` + the multi-scale bridge on libltxmi kernels.

Drop-in for:
  ResBlock / LatentUpsampler (from_config, from_pretrained, forward)   ltx_video/models/autoencoders/latent_upsampler.py:15-203
  adain_filter_latent                                                  ltx_video/pipelines/pipeline_ltx_video.py:1709-1737
  LTXMultiScalePipeline._upsample_latents                              pipeline_ltx_video.py:1760-1772
Same config keys and parameter names (checkpoint-compatible with ltxv-spatial-upscaler-0.9.7).

Activations are channels-last bf16.  nn.Conv3d(padding=1) / nn.Conv2d(padding=1) are the implicit GEMM of
``ltxmi_conv3d_ndhwc_bf16`` with zero padding in time (``time_pad_zeros``) or a per-frame 3x3 kernel
(``kernel_t = 1``); GroupNorm(32) + SiLU (+ the ResBlock residual) is one statistics pass + one apply pass;
the pixel shuffle is a 16-byte-vector copy because the upsampling conv's rows are packed (p1 .. pn c);
un_normalize / normalize ride on the NCDHW<->NDHWC layout kernels.

All three modes of the reference (:83-97, 136-142) run: spatial (Conv2d + PixelShuffleND(2), per frame), temporal
(Conv3d + PixelShuffleND(1)) and spatial + temporal (Conv3d + PixelShuffleND(3)).  The two temporal modes drop
the first output frame (``x[:, :, 1:]``); here that trim is the store address of the shuffle kernel
(``ltxmi_pixel_shuffle_nd_ndhwc_bf16``), not a second pass.  They exist on the reference's dims == 3 branch only.
"""
import json
import math
from typing import Optional

import torch
from torch import nn

from . import ops
from .derived import DerivedOwner

BF16 = torch.bfloat16


class _ConvParams(DerivedOwner, nn.Module):
    """nn.Conv2d / nn.Conv3d(kernel 3, padding 1) parameters under the reference's names."""

    def __init__(self, cin, cout, dims):
        super().__init__()
        self.dims = dims
        bound = 1.0 / math.sqrt(cin * 3 ** dims)
        self.weight = nn.Parameter((torch.rand(cout, cin, *([3] * dims)) * 2 - 1) * bound)
        self.bias = nn.Parameter((torch.rand(cout) * 2 - 1) * bound)

    def packed(self, shuffle=0):
        """(weight [cout, taps * cin] tap-major, bias) in bf16.  shuffle = n in {1, 2, 3}: the rows feed PixelShuffleND(n),
        whose channel split is (c p1 .. pn); they are reordered to (p1 .. pn c) so that the shuffle moves whole runs of c.
        Rebuilt when the weight or the bias changes (ltxmi/derived.py)."""
        def build():
            with torch.no_grad():
                cout = self.weight.shape[0]
                perm = (0, 2, 3, 1) if self.dims == 2 else (0, 2, 3, 4, 1)
                w = self.weight.permute(*perm).reshape(cout, -1)             # tap-major, cin fastest
                b = self.bias
                if shuffle:                                                  # rows (c p1 .. pn) -> (p1 .. pn c)
                    f = 2 ** shuffle
                    c = cout // f
                    w = w.view(c, f, -1).transpose(0, 1).reshape(cout, -1)
                    b = b.view(c, f).transpose(0, 1).reshape(-1)
                return w.contiguous().to(BF16), b.contiguous().to(BF16)
        return self.derived("packed").get((self.weight, self.bias), (shuffle,), build)

    def forward(self, x, shuffle=0):
        """x NDHWC bf16."""
        w, b = self.packed(shuffle)
        return ops.conv3d(x, w, b, causal=False, pad_replicate=False, kernel_t=1 if self.dims == 2 else 3,
                          time_pad_zeros=self.dims == 3)


class _GroupNormParams(nn.Module):
    def __init__(self, groups, ch, eps=1e-5):
        super().__init__()
        self.num_groups, self.eps = groups, eps
        self.weight = nn.Parameter(torch.ones(ch))
        self.bias = nn.Parameter(torch.zeros(ch))


class ResBlock(nn.Module):                                                   # latent_upsampler.py:15-39
    def __init__(self, channels: int, mid_channels: Optional[int] = None, dims: int = 3):
        super().__init__()
        mid_channels = channels if mid_channels is None else mid_channels
        self.dims = dims
        self.conv1 = _ConvParams(channels, mid_channels, dims)
        self.norm1 = _GroupNormParams(32, mid_channels)
        self.conv2 = _ConvParams(mid_channels, channels, dims)
        self.norm2 = _GroupNormParams(32, channels)

    def forward(self, x):
        samples = x.shape[0] * (x.shape[1] if self.dims == 2 else 1)
        h = self.conv1(x)
        h = ops.groupnorm_silu(h, self.norm1.weight, self.norm1.bias, 32, self.norm1.eps, samples=samples, out=h)
        h = self.conv2(h)
        return ops.groupnorm_silu(h, self.norm2.weight, self.norm2.bias, 32, self.norm2.eps, residual=x,
                                  samples=samples, out=h)


class _Upsampler(nn.Module):
    """The reference's ``upsampler`` (:83-97) under its key ``upsampler.0``:
      spatial             nn.Sequential(Conv2d(mid, 4 mid, 3, padding=1), PixelShuffleND(2)), per frame
      temporal            nn.Sequential(Conv3d(mid, 2 mid, 3, padding=1), PixelShuffleND(1)), then x[:, :, 1:]
      spatial + temporal  nn.Sequential(Conv3d(mid, 8 mid, 3, padding=1), PixelShuffleND(3)), then x[:, :, 1:]
    (the trim is forward's, :136-138; it is folded into the shuffle here)."""

    def __init__(self, mid, spatial=True, temporal=False):
        super().__init__()
        self.spatial, self.temporal = spatial, temporal
        if temporal:
            setattr(self, "0", _ConvParams(mid, (8 if spatial else 2) * mid, 3))
        else:
            setattr(self, "0", _ConvParams(mid, 4 * mid, 2))

    def forward(self, x):
        conv = getattr(self, "0")
        if not self.temporal:
            return ops.pixel_shuffle2d(conv(x, shuffle=2))
        ps = 2 if self.spatial else 1
        return ops.pixel_shuffle_nd(conv(x, shuffle=3 if self.spatial else 1), pt=2, ps=ps, drop_first=True)


class LatentUpsampler(nn.Module):
    def __init__(self, in_channels: int = 128, mid_channels: int = 512, num_blocks_per_stage: int = 4, dims: int = 3,
                 spatial_upsample: bool = True, temporal_upsample: bool = False):
        super().__init__()
        if not (spatial_upsample or temporal_upsample):
            raise ValueError("Either spatial_upsample or temporal_upsample must be True")
        if dims not in (2, 3):
            raise NotImplementedError("ltxmi.LatentUpsampler: dims must be 2 or 3")
        if temporal_upsample and dims != 3:
            # the reference's dims == 2 branch (:128-147) hands folded 4-D frames to self.upsampler, which a Conv3d cannot take
            raise NotImplementedError("ltxmi.LatentUpsampler: temporal_upsample needs dims=3 (the reference's dims=2 forward "
                                      "feeds folded [b*f, c, h, w] frames to the upsampler, which its Conv3d cannot take)")
        self.in_channels, self.mid_channels = in_channels, mid_channels
        self.num_blocks_per_stage, self.dims = num_blocks_per_stage, dims
        self.spatial_upsample, self.temporal_upsample = spatial_upsample, temporal_upsample
        self.initial_conv = _ConvParams(in_channels, mid_channels, dims)
        self.initial_norm = _GroupNormParams(32, mid_channels)
        self.res_blocks = nn.ModuleList([ResBlock(mid_channels, dims=dims) for _ in range(num_blocks_per_stage)])
        self.upsampler = _Upsampler(mid_channels, spatial_upsample, temporal_upsample)
        self.post_upsample_res_blocks = nn.ModuleList(
            [ResBlock(mid_channels, dims=dims) for _ in range(num_blocks_per_stage)])
        self.final_conv = _ConvParams(mid_channels, in_channels, dims)

    @property
    def dtype(self):
        return self.initial_conv.weight.dtype

    @property
    def device(self):
        return self.initial_conv.weight.device

    def forward_ndhwc(self, x):
        samples = x.shape[0] * (x.shape[1] if self.dims == 2 else 1)
        x = self.initial_conv(x)
        x = ops.groupnorm_silu(x, self.initial_norm.weight, self.initial_norm.bias, 32, self.initial_norm.eps,
                               samples=samples, out=x)
        for blk in self.res_blocks:
            x = blk(x)
        x = self.upsampler(x)
        for blk in self.post_upsample_res_blocks:
            x = blk(x)
        return self.final_conv(x)

    def forward(self, latent, _stats=None):
        """latent [b, c, f, h, w] -> [b, c, f, 2h, 2w] (spatial), [b, c, 2f-1, h, w] (temporal) or [b, c, 2f-1, 2h, 2w]
        (both) (latent_upsampler.py:109-149).  ``_stats`` = (std, mean) fp32 [c]: un_normalize on the way in and
        normalize on the way out (``_upsample_latents``)."""
        std, mean = _stats if _stats is not None else (None, None)
        x = ops.ncdhw_to_ndhwc(latent.to(BF16), std, mean)
        y = self.forward_ndhwc(x)
        return ops.ndhwc_to_ncdhw(y, 0, self.in_channels, std, mean)

    @classmethod
    def from_config(cls, config):                                            # :151-160
        return cls(in_channels=config.get("in_channels", 4), mid_channels=config.get("mid_channels", 128),
                   num_blocks_per_stage=config.get("num_blocks_per_stage", 4), dims=config.get("dims", 2),
                   spatial_upsample=config.get("spatial_upsample", True),
                   temporal_upsample=config.get("temporal_upsample", False))

    def config(self):                                                        # :162-171
        return {"_class_name": "LatentUpsampler", "in_channels": self.in_channels, "mid_channels": self.mid_channels,
                "num_blocks_per_stage": self.num_blocks_per_stage, "dims": self.dims,
                "spatial_upsample": self.spatial_upsample, "temporal_upsample": self.temporal_upsample}

    @classmethod
    def from_pretrained(cls, pretrained_model_path, *args, device="cuda", dtype=BF16, **kwargs):   # :173-191
        from safetensors import safe_open
        path = str(pretrained_model_path)
        if not path.endswith(".safetensors"):
            raise ValueError(f"unrecognised checkpoint path: {path}")
        sd = {}
        with safe_open(path, framework="pt", device="cpu") as f:
            meta = f.metadata()
            for k in f.keys():
                sd[k] = f.get_tensor(k)
        m = cls.from_config(json.loads(meta["config"]))
        m.load_state_dict(sd, strict=True)
        return m.to(device=device, dtype=dtype).eval()


def adain_filter_latent(latents, reference_latents, factor=1.0):
    """pipeline_ltx_video.py:1709-1737, one kernel (a block per (b, c) plane)."""
    return ops.adain_filter(latents, reference_latents.to(latents.dtype), factor)


def upsample_latents(latent_upsampler: LatentUpsampler, latents, vae):
    """LTXMultiScalePipeline._upsample_latents (:1760-1772): un_normalize_latents -> upsampler ->
    normalize_latents with the VAE's per-channel statistics, both folded into the layout passes."""
    stats = (vae.std_of_means.float().contiguous(), vae.mean_of_means.float().contiguous())
    return latent_upsampler(latents, _stats=stats).to(latents.dtype)
