"""Plain-torch restatement of the reference's ``mixed=True`` DiT forward.  TEST INFRASTRUCTURE ONLY.

``Transformer3DModel.forward(mixed=True)`` under ``torch.autocast`` (pipeline_ltx_video.py:1152-1177) keeps the residual
stream, the AdaLN values and the output norm in fp32 and runs every linear, the q/k norms and attention in the autocast
dtype.  What is rounded where is uneven, and this file states it op for op on top of the leaves of ``oracle.dit``:

  transformer3d.py:418,428-433   patchify_proj / adaln_single are linears under autocast: their outputs are ``ld``
  transformer3d.py:439-442       hidden_states, timestep, embedded_timestep ``.float()``; the text states stay ``ld``
  attention.py:233-251           norm1 of an fp32 tensor, ``table (ld) + timestep (fp32)``, ``*= 1 + scale; += shift``: fp32;
                                 the first rounding is autocast's cast at to_q / to_k / to_v
  attention.py:285               ``attn_output *= gate_msa`` IN PLACE on the ``ld`` attention output: the product is rounded
  attention.py:288, 310          ``hidden_states += attn_output``: fp32 += ld
  attention.py:294-309           attn2 reads the fp32 stream, cast at to_q
  attention.py:334-351           ``h_chunk[...] = ff.net[2](...)`` stores the ``ld`` result into the fp32 norm buffer, so
                                 ``ff_output *= gate_mlp`` and the sum are fp32
  attention.py:355-362           the TransformerBlock blend on fp32 states
  transformer3d.py:489-503       norm_out and the modulation in fp32, proj_out under autocast returns ``ld``

``ld`` (the "linear dtype") is the autocast dtype: ``torch.bfloat16`` gives the reference's mixed rendering, ``torch.float32``
makes every cast a no-op and gives the fp32 truth (= the reference's plain fp32 forward).  ``sd`` holds the weights in
``ld``."""
import torch
import torch.nn.functional as F

from oracle import dit, leaves


def transformer_block_mixed(sd, p, cfg, hidden_states, freqs_cis, encoder_hidden_states, encoder_attention_mask, timestep,
                            ld, skip_layer_mask=None, skip_layer_strategy=None):
    """BasicTransformerBlock.forward (attention.py:205-364) on an fp32 ``hidden_states`` / ``timestep`` under autocast(ld)."""
    assert hidden_states.dtype == torch.float32 and timestep.dtype == torch.float32 and timestep.ndim == 3
    batch_size = hidden_states.shape[0]
    if skip_layer_mask is not None and skip_layer_mask.flatten().min() == 1.0:
        skip_layer_mask = None

    table = sd[p + "scale_shift_table"]                                          # ld
    ada = table[None, None] + timestep.reshape(batch_size, timestep.shape[1], table.shape[0], -1)      # ld + fp32 = fp32
    assert ada.dtype == torch.float32
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = ada.unsqueeze(-2).unbind(dim=2)
    t1 = scale_msa.shape[1]

    norm_h = dit._norm(hidden_states, sd, p + "norm1.", cfg)                     # fp32
    norm_h = dit._flat(dit._frames(norm_h, t1) * (1 + scale_msa) + shift_msa)    # fp32 (:248-249)
    attn_out = dit.attention_processor(sd, p + "attn1.", cfg, norm_h.to(ld), freqs_cis=freqs_cis,
                                       skip_layer_mask=skip_layer_mask, skip_layer_strategy=skip_layer_strategy)
    attn_out = dit._flat((dit._frames(attn_out, t1) * gate_msa).to(ld))          # :285, in place on the ld tensor
    hidden_states = hidden_states + attn_out                                     # :288, fp32

    if (p + "attn2.to_q.weight") in sd:
        attn_out = dit.attention_processor(sd, p + "attn2.", cfg, hidden_states.to(ld), freqs_cis=freqs_cis,
                                           encoder_hidden_states=encoder_hidden_states,
                                           attention_mask=encoder_attention_mask)
        hidden_states = hidden_states + attn_out                                 # :310, fp32 += ld
    original_hidden_states = hidden_states                                       # the alias of :231 after :288, :310

    norm_h = dit._norm(hidden_states, sd, p + "norm2.", cfg)
    norm_h = dit._flat(dit._frames(norm_h, t1) * (1 + scale_mlp) + shift_mlp)    # fp32 (:318-319)
    ff = leaves.gelu_proj(norm_h.to(ld), sd, p + "ff.net.0.", "tanh")
    ff = leaves.linear(ff, sd, p + "ff.net.2.").float()                          # :340, ld result stored into the fp32 buffer
    ff = dit._flat(dit._frames(ff, t1) * gate_mlp)                               # :348, fp32 product
    hidden_states = ff + hidden_states                                           # :351

    if skip_layer_mask is not None and skip_layer_strategy == dit.TRANSFORMER_BLOCK:
        m = skip_layer_mask.view(-1, 1, 1).float()
        hidden_states = hidden_states * m + original_hidden_states * (1.0 - m)
    assert hidden_states.dtype == torch.float32
    return hidden_states


def transformer3d_forward_mixed(sd, cfg, hidden_states, freqs_cis, encoder_hidden_states, timestep, ld,
                                encoder_attention_mask=None, skip_layer_mask=None, skip_layer_strategy=None,
                                latent_shape=None, num_layers=None):
    """Transformer3DModel.forward(joint_pass=True, mixed=True) under autocast(ld) (transformer3d.py:328-507).
    ``freqs_cis`` and ``sd`` in ``ld``; returns the sample [B, N, out_channels] in ``ld``."""
    if encoder_attention_mask is not None and encoder_attention_mask.ndim == 2:
        encoder_attention_mask = ((1 - encoder_attention_mask.float()) * -10000.0).unsqueeze(1)

    hidden_states = leaves.linear(hidden_states.to(ld), sd, "patchify_proj.")    # :418
    if cfg.get("timestep_scale_multiplier"):
        timestep = cfg["timestep_scale_multiplier"] * timestep
    if timestep.shape[-1] > 1:
        timestep = timestep.reshape(timestep.shape[0], -1, latent_shape[-2] * latent_shape[-1])[:, :, 0]
    batch_size = hidden_states.shape[0]
    timestep, embedded_timestep = leaves.adaln_single(timestep.flatten(), sd, "adaln_single.", ld)     # :428-433
    timestep = timestep.view(batch_size, -1, timestep.shape[-1]).float()         # :439-442
    embedded_timestep = embedded_timestep.view(batch_size, -1, embedded_timestep.shape[-1]).float()
    hidden_states = hidden_states.float()

    if "caption_projection.linear_1.weight" in sd:
        encoder_hidden_states = leaves.text_projection(encoder_hidden_states.to(ld), sd, "caption_projection.")
        encoder_hidden_states = encoder_hidden_states.view(batch_size, -1, hidden_states.shape[-1])

    L = cfg["num_layers"] if num_layers is None else num_layers
    for i in range(L):
        hidden_states = transformer_block_mixed(
            sd, f"transformer_blocks.{i}.", cfg, hidden_states, freqs_cis, encoder_hidden_states, encoder_attention_mask,
            timestep, ld, skip_layer_mask=None if skip_layer_mask is None else skip_layer_mask[i],
            skip_layer_strategy=skip_layer_strategy)

    ssv = sd["scale_shift_table"][None, None] + embedded_timestep[:, :, None]    # ld + fp32 = fp32 (:490-492)
    shift, scale = ssv[:, :, 0].unsqueeze(-2), ssv[:, :, 1].unsqueeze(-2)
    hidden_states = F.layer_norm(hidden_states, (hidden_states.shape[-1],), None, None, 1e-6)
    hidden_states = dit._flat(dit._frames(hidden_states, scale.shape[1]) * (1 + scale) + shift)        # fp32 (:500-501)
    return leaves.linear(hidden_states.to(ld), sd, "proj_out.")                  # :503


def run(sd32, cfg, x, enc, mask, ts, frac, grid, ld, device="cpu", **kw):
    """One forward from fp32 host inputs: weights, rope tables and the skip mask cast to ``ld`` on ``device``."""
    sd = {k: v.to(device=device, dtype=ld) for k, v in sd32.items()}
    fc = tuple(t.to(device) for t in dit.precompute_freqs_cis(frac, cfg, ld))
    if kw.get("skip_layer_mask") is not None:
        kw = dict(kw, skip_layer_mask=kw["skip_layer_mask"].to(device=device, dtype=ld))
    out = transformer3d_forward_mixed(sd, cfg, x.to(device), fc, enc.to(device), ts.to(device), ld,
                                      encoder_attention_mask=mask.to(device), latent_shape=grid, **kw)
    return out.cpu()


def oracles(sd32, cfg, x, enc, mask, ts, frac, grid, device="cpu", **kw):
    """(fp32 truth, the reference's mixed rendering) -- what ``assert_parity`` of tests/test_gpu_model.py takes."""
    return (run(sd32, cfg, x, enc, mask, ts, frac, grid, torch.float32, device, **kw),
            run(sd32, cfg, x, enc, mask, ts, frac, grid, torch.bfloat16, device, **kw))
