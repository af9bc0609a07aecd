"""Generate tests/golden/g17_reflect.safetensors (+ g17_reflect.json) by running the REFERENCE's own autoencoder modules with
``spatial_padding_mode="reflect"``.

BUILD-CONTAINER-ONLY, like oracle/gen/make_golden.py whose import shims and module handles it uses (``ref_cc3``, ``ref_cva``):
the reference is imported read-only, seeded tiny cases run on the CPU, and only data is written -- inputs, weights and outputs
as plain tensors, the configuration as JSON.  manifest.json is not touched.

    python tools/make_golden_reflect.py          # from the repo root

G17, with the seeds and shapes of G8 / G10c / G11 where those have the case:
  conv.*      CausalConv3d(6, 10) on [2, 6, 4, 5, 7], causal and not                          (G8: seeds 40 / 41)
  sconv.*     CausalConv3d(8, 12) with the three encoder strides on [2, 8, 5, 6, 8], causal   (G11: 60 / 61)
  s2d.*       SpaceToDepthDownsample(8 -> 16) for the three strides                           (G11: 62)
  res.*       ResnetBlock3D(8 -> 8, timestep-conditioned) on [2, 8, 3, 4, 5]                  (G8: 42)
  up.* up2.*  DepthToSpaceUpsample(8, (2, 2, 2)) with residual / reduction 2, and without     (G8: 44 / 45)
  dec.* enc.* one Decoder.forward and one Encoder.forward of a small VAE, base channels 8, patch size 2 (as G10c's), whose
              blocks take every convolution kind: compress_all with residual, compress_space and res_x going up;
              compress_space_res (space-to-depth), strided compress_all and compress_time going down."""
import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen import make_golden as mg  # noqa: E402  (installs the import shims, imports the reference)

MODE = "reflect"
VAE_CFG = {"_class_name": "CausalVideoAutoencoder", "dims": 3, "in_channels": 3, "out_channels": 3, "latent_channels": 8,
           "encoder_blocks": [["res_x", {"num_layers": 1}], ["compress_space_res", {"multiplier": 2}], ["res_x", {"num_layers": 1}],
                              ["compress_all", {}], ["compress_time", {}]],
           "decoder_blocks": [["res_x", {"num_layers": 1}], ["compress_space", {}], ["res_x", {"num_layers": 1}],
                              ["compress_all", {"residual": True, "multiplier": 2}], ["res_x", {"num_layers": 1}]],
           "scaling_factor": 1.0, "norm_layer": "pixel_norm", "patch_size": 2, "latent_log_var": "uniform",
           "use_quant_conv": False, "causal_decoder": False, "timestep_conditioning": True,
           "spatial_padding_mode": MODE, "encoder_base_channels": 8, "decoder_base_channels": 8}


@torch.no_grad()
def main():
    t = {}
    g = torch.Generator().manual_seed(40)
    x = torch.randn(2, 6, 4, 5, 7, generator=g)
    t["x"] = x
    torch.manual_seed(41)
    conv = mg.ref_cc3.CausalConv3d(6, 10, kernel_size=3, spatial_padding_mode=MODE)
    assert conv.conv.padding_mode == MODE
    t["conv.conv.weight"], t["conv.conv.bias"] = conv.conv.weight, conv.conv.bias
    t["conv.causal"], t["conv.noncausal"] = conv(x, causal=True), conv(x, causal=False)
    torch.randn(2, 3, 8, 64, 64, generator=g)                                  # G8's patchify input: the generator state G8 goes on from

    torch.manual_seed(42)
    res = mg.ref_cva.ResnetBlock3D(dims=3, in_channels=8, out_channels=8, eps=1e-6, norm_layer="pixel_norm",
                                   timestep_conditioning=True, spatial_padding_mode=MODE).eval()
    xr = torch.randn(2, 8, 3, 4, 5, generator=g)
    temb = torch.randn(2, 32, 1, 1, 1, generator=g) * 0.5
    t["res.x"], t["res.temb"] = xr, temb
    t["res.out"] = res(xr, causal=False, timestep=temb)
    t.update({"res.sd." + k: v for k, v in res.state_dict().items()})
    torch.manual_seed(44)
    up = mg.ref_cva.DepthToSpaceUpsample(dims=3, in_channels=8, stride=(2, 2, 2), residual=True, out_channels_reduction_factor=2,
                                         spatial_padding_mode=MODE).eval()
    t["up.out"] = up(xr, causal=False)
    t.update({"up.sd." + k: v for k, v in up.state_dict().items()})
    torch.manual_seed(45)
    up2 = mg.ref_cva.DepthToSpaceUpsample(dims=3, in_channels=8, stride=(2, 2, 2), residual=False, out_channels_reduction_factor=1,
                                          spatial_padding_mode=MODE).eval()
    t["up2.out"] = up2(xr, causal=False)
    t.update({"up2.sd." + k: v for k, v in up2.state_dict().items()})

    g = torch.Generator().manual_seed(60)
    xs = torch.randn(2, 8, 5, 6, 8, generator=g)
    t["enc_x"] = xs
    for name, stride in (("time", (2, 1, 1)), ("space", (1, 2, 2)), ("all", (2, 2, 2))):
        torch.manual_seed(61)
        conv = mg.ref_cc3.CausalConv3d(8, 12, kernel_size=3, stride=stride, spatial_padding_mode=MODE)
        t[f"sconv.{name}.conv.weight"], t[f"sconv.{name}.conv.bias"] = conv.conv.weight, conv.conv.bias
        t[f"sconv.{name}.out"] = conv(xs, causal=True)
        torch.manual_seed(62)
        s2d = mg.ref_cva.SpaceToDepthDownsample(dims=3, in_channels=8, out_channels=16, stride=stride, spatial_padding_mode=MODE).eval()
        t[f"s2d.{name}.out"] = s2d(xs)
        t.update({f"s2d.{name}.sd.{k}": v for k, v in s2d.state_dict().items()})

    torch.manual_seed(170)
    vae = mg.ref_cva.CausalVideoAutoencoder.from_config(mg.jsonable(VAE_CFG)).eval()
    modes = {m.padding_mode for m in vae.modules() if isinstance(m, torch.nn.Conv3d)}
    assert modes == {MODE}, modes
    g = torch.Generator().manual_seed(171)
    sd = vae.state_dict()
    t.update({"dec.sd." + k: v for k, v in sd.items() if k.startswith("decoder.")})
    t.update({"enc.sd." + k: v for k, v in sd.items() if k.startswith("encoder.")})
    z = torch.randn(1, 8, 2, 3, 4, generator=g)
    ts = torch.tensor([0.05])
    t["dec.z"], t["dec.timestep"] = z, ts
    # reversed decoder_blocks: res_x @ (2, 3, 4), compress_all -> (3, 6, 8), res_x, compress_space -> (3, 12, 16), res_x, unpatchify 2
    t["dec.out"] = vae.decoder(z, target_shape=(1, 3, 3, 24, 32), timestep=ts)
    xe = torch.rand(1, 3, 5, 32, 48, generator=g) * 2 - 1
    t["enc.x"] = xe
    t["enc.out"] = vae.encoder(xe)

    out = os.path.join(ROOT, "tests", "golden")
    tensors = {k: v.detach().clone().contiguous() for k, v in t.items()}
    save_file(tensors, os.path.join(out, "g17_reflect.safetensors"))
    meta = dict(mode=MODE, vae_cfg=VAE_CFG, shapes={k: list(v.shape) for k, v in tensors.items() if ".sd." not in k and "weight" not in k})
    with open(os.path.join(out, "g17_reflect.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    print(f"  g17_reflect: {len(tensors)} tensors, {sum(v.numel() * v.element_size() for v in tensors.values()) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
