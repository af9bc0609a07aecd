#!/usr/bin/env python3
"""What the spatial padding mode costs a VAE decode: the bench's decoder (bench.make_vae's configuration and seed, so the same
weights) built once per mode -- "replicate", "reflect", and "zeros" for reference -- and decoded alternately in one process.

  --config 2   z [1, 128, 13, 16, 24] -> 97 frames of 768 x 512, untiled          (bench.py --full: vae_decode)
  --config 5   z [1, 128, 33, 23, 40] -> 257 frames of 1280 x 720, z-tiled by 4   (bench.py --full: vae_decode_config5)

Per round every mode is decoded --iters times between two device events (after a warm-up decode of every mode); the modes
alternate inside a round, so drift of the card hits them alike.  Reported per mode: median / min / max of the rounds' ms per
decode.  Reported, not asserted: the mode only changes the per-tile row table of the direct convolutions and one add / subtract
with carry in the implicit GEMM's gather, so equality is what to expect.  One config per process: run each under its own
``timeout``.  Writes --out (JSON) if given and prints the result.

    python tools/vae_pad_mode_time.py --config 2 [--rounds 5] [--iters 5] [--out profiles/vae_reflect_config2.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

CONFIGS = {2: dict(grid=(13, 16, 24), z_tile=0), 5: dict(grid=(33, 23, 40), z_tile=4)}
MODES = ("replicate", "reflect", "zeros")


def build(mode, device, z_tile):
    """bench.make_vae's decoder with ``spatial_padding_mode`` = mode."""
    import ltxmi
    from oracle import vae as ov
    cfg = dict(ov.demo_config(128), spatial_padding_mode=mode)
    torch.manual_seed(5)
    with torch.device(device):
        vae = ltxmi.CausalVideoAutoencoder.from_config(cfg)
    vae = vae.to(dtype=torch.bfloat16).eval()
    vae.decoder.timestep_scale_multiplier.data = vae.decoder.timestep_scale_multiplier.data.float()
    if z_tile:
        vae.enable_z_tiling(z_tile)
    return vae


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=sorted(CONFIGS), default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "vae_pad_mode_time.py measures on the GPU"
    import ltxmi
    dev = "cuda:0"
    torch.cuda.set_device(0)
    c = CONFIGS[a.config]
    vaes = {m: build(m, dev, c["z_tile"]) for m in MODES}
    w = [next(iter(v.decoder.parameters())) for v in vaes.values()]
    assert all(torch.equal(w[0], x) for x in w[1:]), "the modes must decode the same weights"
    z = torch.randn(1, 128, *c["grid"], device=dev, generator=torch.Generator(device=dev).manual_seed(6)).to(torch.bfloat16)
    ts = torch.tensor([0.05], device=dev)

    @torch.no_grad()
    def decode(mode):
        return ltxmi.vae_decode(z, vaes[mode], True, vae_per_channel_normalize=True, timestep=ts)

    imgs = {m: decode(m) for m in MODES}                       # warm-up, and: the modes really differ
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(i.float()).all()) for i in imgs.values())
    differ = {m: round(float((imgs[m].float() - imgs["replicate"].float()).norm() / imgs["replicate"].float().norm()), 4) for m in MODES}
    del imgs
    times = {m: [] for m in MODES}
    for _ in range(a.rounds):
        for m in MODES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                decode(m)
            e1.record()
            e1.synchronize()
            times[m].append(e0.elapsed_time(e1) / a.iters)
    result = dict(config=a.config, latent=[1, 128, *c["grid"]], z_tile=c["z_tile"], rounds=a.rounds, iters_per_round=a.iters,
                  rel_l2_vs_replicate_decode=differ,
                  ms_per_decode={m: dict(median=round(statistics.median(t), 3), min=round(min(t), 3), max=round(max(t), 3),
                                         rounds=[round(x, 3) for x in t]) for m, t in times.items()})
    med = {m: result["ms_per_decode"][m]["median"] for m in MODES}
    result["reflect_over_replicate"] = round(med["reflect"] / med["replicate"], 4)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
