"""Generate tests/golden/g16_mixed.safetensors (+ g16_mixed.json) by running the REFERENCE's own
``Transformer3DModel.forward(mixed=True)`` under CPU autocast.

BUILD-CONTAINER-ONLY, like oracle/gen/make_golden.py whose helpers it uses (``ref_shims``, ``build_dit``, ``dit_inputs``,
``coords``): the reference is imported read-only, seeded tiny cases run on the CPU, and only data is written -- inputs,
weights and outputs as plain tensors, the metadata as JSON.

    python tools/make_golden_mixed.py          # from the repo root

G16: the tiny DiT of the other DiT goldens with bf16 weights, B 3, grid (2, 3, 4).  Each case stores the mixed forward
(``mixed=True`` under ``torch.autocast("cpu", dtype=torch.bfloat16)``, bf16 out), the plain bf16 forward and the fp32 forward
of the same (bf16-valued) weights:
  L2.sample / L2.token   2 layers, per-sample / per-token timestep
  L8.sample              8 layers
  L4.<strategy>          4 layers, blocks 1 and 2 skipped for the third batch row, once per skip-layer strategy
One four-block state dict serves every case: an L-layer model takes block i % 4 as its block i, which keeps the file the
size of the other DiT goldens."""
import json
import os
import sys
import types

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen import make_golden as mg  # noqa: E402  (installs the import shims, imports the reference)

BF = torch.bfloat16
STORED_BLOCKS = 4
CASES = [("L2.sample", 2, False, None), ("L2.token", 2, True, None), ("L8.sample", 8, False, None)] + \
        [(f"L4.{s}", 4, False, s) for s in ("AttentionValues", "AttentionSkip", "Residual", "TransformerBlock")]


def state_dict_for(sd, layers):
    """Block i of an L-layer model = stored block i % STORED_BLOCKS."""
    out = {k: v for k, v in sd.items() if not k.startswith("transformer_blocks.")}
    for i in range(layers):
        src = f"transformer_blocks.{i % STORED_BLOCKS}."
        out.update({f"transformer_blocks.{i}." + k[len(src):]: v for k, v in sd.items() if k.startswith(src)})
    return out


@torch.no_grad()
def main():
    cfg = dict(mg.TINY_DIT, num_layers=STORED_BLOCKS)
    f, h, w, B, T = 2, 3, 4, 3, 8
    sd = {k: v.to(BF) for k, v in mg.build_dit(cfg, 160).state_dict().items()}         # the weights ARE bf16 values
    _, pc = mg.coords(f, h, w, 1)
    holder = types.SimpleNamespace(_interrupt=False)
    t = {"indices_grid": pc}
    t.update({"sd." + k: v for k, v in sd.items()})
    meta = dict(cfg=cfg, grid=(f, h, w), B=B, T=T, stored_blocks=STORED_BLOCKS, skip_blocks=[1, 2], cases=[])
    x, enc, mask, ts = mg.dit_inputs(cfg, f, h, w, B, T, 161)
    _, _, _, ts_tok = mg.dit_inputs(cfg, f, h, w, B, T, 161, per_token_timestep=True)
    t.update({"x": x, "enc": enc, "mask": mask, "ts": ts, "ts_tok": ts_tok})
    for name, layers, per_token, strategy in CASES:
        model = mg.ref_t3.Transformer3DModel(**dict(cfg, num_layers=layers)).eval()
        model.load_state_dict(state_dict_for(sd, layers))
        kw = dict(encoder_attention_mask=mask, latent_shape=(f, h, w), ltxv_model=holder, return_dict=False,
                  timestep=ts_tok if per_token else ts)
        if strategy is not None:
            kw["skip_layer_strategy"] = getattr(mg.SkipLayerStrategy, strategy)
        m32 = model.float()
        skip32 = m32.create_skip_layer_mask(1, 3, 2, [1, 2]) if strategy is not None else None
        out32 = m32(x.clone(), freqs_cis=m32.precompute_freqs_cis(pc), encoder_hidden_states=enc, skip_layer_mask=skip32, **kw)[0]
        mb = model.to(BF)
        fb = mb.precompute_freqs_cis(pc)
        skip = mb.create_skip_layer_mask(1, 3, 2, [1, 2]) if strategy is not None else None   # in the model's dtype (:171-186)
        plain = mb(x.to(BF), freqs_cis=fb, encoder_hidden_states=enc.to(BF), skip_layer_mask=skip, **kw)[0]
        with torch.autocast("cpu", dtype=BF):
            # pipeline_ltx_video.py:1152-1177: fp32 latents in, mixed=True
            mixed = mb(x.clone(), freqs_cis=fb, encoder_hidden_states=enc.to(BF), skip_layer_mask=skip, mixed=True, **kw)[0]
        assert mixed.dtype == BF and out32.dtype == torch.float32
        t[f"{name}.fp32"], t[f"{name}.bf16"], t[f"{name}.mixed"] = out32, plain, mixed
        if skip is not None:
            t["skip_layer_mask"] = skip.float()

        def rel(a):
            return float((a.float() - out32).norm() / out32.norm())
        meta["cases"].append(dict(name=name, layers=layers, per_token=per_token, strategy=strategy,
                                  rel_bf16=rel(plain), rel_mixed=rel(mixed)))
        print(f"  {name}: rel L2 vs fp32: plain bf16 {rel(plain):.2e}, mixed {rel(mixed):.2e}")
    out = os.path.join(ROOT, "tests", "golden")
    tensors = {k: v.detach().clone().contiguous() for k, v in t.items()}
    save_file(tensors, os.path.join(out, "g16_mixed.safetensors"))
    with open(os.path.join(out, "g16_mixed.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    print(f"  g16_mixed: {len(tensors)} tensors, {sum(v.numel() * v.element_size() for v in tensors.values()) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
