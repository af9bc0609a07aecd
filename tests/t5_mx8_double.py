"""tests/t5_double.py's encoder with chosen projections in MX-FP8 -- TEST INFRASTRUCTURE ONLY (plain torch, no GPU).

``encoder_forward`` is ``t5_double.encoder_forward`` operation by operation, except that a chosen linear ("qkv", "o", "wi", "wo":
the names of ltxmi/t5_mx8.py) multiplies the quantised-and-de-quantised forms of its input and of its weight, by the format
restatement of tests/mx8_cases.py (scale byte from the block amax, elements RNE to e4m3): what ``T5EncoderModel.quantize`` makes the
GPU compute, with the accumulation and every other operation left in the dtype of the weights.  With no linear chosen every
operation is t5_double's, so the result equals it bit for bit (tests/test_t5_mx8_cpu.py).

  * float64 weights: the truth for the quantised GPU model (the format is part of the function, not of the error);
  * bfloat16 weights: the yardstick, as in tests/test_gpu_t5.py."""
import torch

import mx8_cases as mc
import t5_double as td

LINEARS = ("qkv", "o", "wi", "wo")


def qdq(x):
    """x [..., K] of any floating dtype -> de-quantise(quantise(x)) in that dtype (exact: an e4m3 value times a power of two)."""
    x2 = x.reshape(-1, x.shape[-1])
    s = mc.scale_bytes_real(x2)
    return mc.dequantize(mc.quantize_elements(x2, s), s, x.dtype).reshape(x.shape)


def encoder_forward(sd, cfg, ids, mask=None, linears=LINEARS):
    """sd: HF-named weights, all of one floating dtype -> the last hidden state [B, L, d_model] in that dtype."""
    dt = sd["shared.weight"].dtype
    wide = torch.float64 if dt == torch.float64 else torch.float32
    B, L = ids.shape
    H, dkv, eps = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"]

    def lin(name, h, w):
        return qdq(h) @ qdq(w).t() if name in linears else h @ w.t()

    x = sd["shared.weight"][ids]
    bias = td.position_bias(sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], L, L,
                            cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"])[None]
    if mask is not None:
        bias = bias + ((1.0 - mask.to(dt)) * torch.finfo(dt).min)[:, None, None, :]
    for n in range(cfg["num_layers"]):
        p = f"encoder.block.{n}.layer."
        h = td.layer_norm(x, sd[p + "0.layer_norm.weight"], eps)
        q, k, v = (lin("qkv", h, sd[p + f"0.SelfAttention.{c}.weight"]).view(B, L, H, dkv).transpose(1, 2) for c in "qkv")
        scores = q @ k.transpose(3, 2)
        scores = scores + bias
        w = torch.softmax(scores.to(wide), dim=-1).to(dt)
        ctx = (w @ v).transpose(1, 2).reshape(B, L, H * dkv)
        x = x + lin("o", ctx, sd[p + "0.SelfAttention.o.weight"])
        h = td.layer_norm(x, sd[p + "1.layer_norm.weight"], eps)
        g = td.gelu_new(lin("wi", h, sd[p + "1.DenseReluDense.wi_0.weight"])) * lin("wi", h, sd[p + "1.DenseReluDense.wi_1.weight"])
        x = x + lin("wo", g, sd[p + "1.DenseReluDense.wo.weight"])
    return td.layer_norm(x, sd["encoder.final_layer_norm.weight"], eps)
