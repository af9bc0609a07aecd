"""The T5-v1.1 encoder restated in plain torch on the CPU -- TEST INFRASTRUCTURE ONLY.

``encoder_forward`` follows Hugging Face ``modeling_t5.py`` (T5EncoderModel, eager) operation by operation: embedding,
T5LayerNorm, the bucketed relative bias of block 0 plus the padding mask, unscaled attention with the softmax in float32 (or
wider), the gated tanh-GELU feed-forward in NewGELUActivation's own formula, the residual adds and the final norm.  Every
operation runs in the dtype of the weights it is given:

  * float64 weights: the oracle (tests/test_t5_cpu.py pins it to ``transformers.T5EncoderModel`` in fp32 and to a golden);
  * bfloat16 weights: torch rounds after every operation, which is where HF's eager bf16 run rounds -- the yardstick the GPU
    model's error is measured against (tests/test_gpu_t5.py).

The bucket function here is written on its own, from the description in the T5 paper's mesh-tensorflow code, with Python
integers and math.log on float32-rounded values; tests/test_t5_cpu.py checks it against HF's and against ltxmi's."""
import math

import numpy as np
import torch

TINY = dict(d_model=128, d_kv=64, d_ff=256, num_heads=2, num_layers=2, vocab_size=64, relative_attention_num_buckets=32,
            relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
# one block at T5-v1.1-XXL's widths
XXL_ONE = dict(TINY, d_model=4096, d_ff=10240, num_heads=64, num_layers=1, vocab_size=512)
XXL = dict(XXL_ONE, num_layers=24, vocab_size=32128)


def bucket(d, num_buckets=32, max_distance=128):
    """Bucket of the offset d = key - query, bidirectional."""
    half = num_buckets // 2
    base = half if d > 0 else 0
    n = abs(d)
    max_exact = half // 2
    if n < max_exact:
        return base + n
    # float32 division and log, as a float32 tensor op would do them; the scale factors are Python doubles
    ratio = np.float32(n) / np.float32(max_exact)
    val = np.float32(np.log(ratio)) / np.float32(math.log(max_distance / max_exact)) * np.float32(half - max_exact)
    return base + min(max_exact + int(np.float32(val)), half - 1)


def state_dict_names(cfg):
    names = ["shared.weight", "encoder.final_layer_norm.weight",
             "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    for n in range(cfg["num_layers"]):
        p = f"encoder.block.{n}.layer."
        names += [p + f"0.SelfAttention.{x}.weight" for x in "qkvo"] + [p + "0.layer_norm.weight", p + "1.layer_norm.weight"]
        names += [p + f"1.DenseReluDense.{x}.weight" for x in ("wi_0", "wi_1", "wo")]
    return names


def init_state_dict(cfg, seed=0, stream=1.0, qk_gain=1.0):
    """Seeded fp32 weights (CPU generator).  ``stream``: the scale of the embedding and of the o / wo outputs, i.e. of the
    residual stream (T5's runs into the hundreds); ``qk_gain``: scale of q and k, i.e. of the unscaled logits."""
    g = torch.Generator().manual_seed(seed)
    D, F, H, inner = cfg["d_model"], cfg["d_ff"], cfg["num_heads"], cfg["num_heads"] * cfg["d_kv"]

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    sd = {"shared.weight": rn(cfg["vocab_size"], D, std=stream),
          "encoder.final_layer_norm.weight": 1.0 + rn(D, std=0.1),
          "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight":
              rn(cfg["relative_attention_num_buckets"], H, std=3.0)}
    for n in range(cfg["num_layers"]):
        p = f"encoder.block.{n}.layer."
        sd[p + "0.SelfAttention.q.weight"] = rn(inner, D, std=qk_gain / math.sqrt(D))
        sd[p + "0.SelfAttention.k.weight"] = rn(inner, D, std=qk_gain / math.sqrt(D))
        sd[p + "0.SelfAttention.v.weight"] = rn(inner, D, std=1.0 / math.sqrt(D))
        sd[p + "0.SelfAttention.o.weight"] = rn(D, inner, std=stream / math.sqrt(inner))
        sd[p + "0.layer_norm.weight"] = 1.0 + rn(D, std=0.1)
        sd[p + "1.DenseReluDense.wi_0.weight"] = rn(F, D, std=1.0 / math.sqrt(D))
        sd[p + "1.DenseReluDense.wi_1.weight"] = rn(F, D, std=1.0 / math.sqrt(D))
        sd[p + "1.DenseReluDense.wo.weight"] = rn(D, F, std=stream / math.sqrt(F))
        sd[p + "1.layer_norm.weight"] = 1.0 + rn(D, std=0.1)
    return sd


def tiny_inputs(cfg=TINY, L=24, seed=1):
    """Batch 2, the second row padded to a single valid token."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, cfg["vocab_size"], (2, L), generator=g)
    mask = torch.ones(2, L, dtype=torch.long)
    mask[1, 1:] = 0
    ids[1, 1:] = 0
    return ids, mask


def layer_norm(x, w, eps):
    wide = torch.float64 if x.dtype == torch.float64 else torch.float32
    var = x.to(wide).pow(2).mean(-1, keepdim=True)
    h = x * torch.rsqrt(var + eps)
    if w.dtype in (torch.float16, torch.bfloat16):
        h = h.to(w.dtype)
    return w * h


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def position_bias(table, Lq, Lk, num_buckets, max_distance, negate_offset=False):
    """[H, Lq, Lk] from the [num_buckets, H] table: table[bucket(j - i), h] (negate_offset: bucket(i - j), the wrong sign)."""
    idx = torch.tensor([[bucket((i - j) if negate_offset else (j - i), num_buckets, max_distance) for j in range(Lk)]
                        for i in range(Lq)], dtype=torch.long)
    return table[idx].permute(2, 0, 1)


def encoder_forward(sd, cfg, ids, mask=None, negate_offset=False):
    """sd: HF-named weights, all of one floating dtype -> the last hidden state [B, L, d_model] in that dtype."""
    dt = sd["shared.weight"].dtype
    wide = torch.float64 if dt == torch.float64 else torch.float32
    B, L = ids.shape
    H, dkv, eps = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"]
    x = sd["shared.weight"][ids]
    bias = position_bias(sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], L, L,
                         cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"], negate_offset)[None]
    if mask is not None:
        bias = bias + ((1.0 - mask.to(dt)) * torch.finfo(dt).min)[:, None, None, :]
    for n in range(cfg["num_layers"]):
        p = f"encoder.block.{n}.layer."
        h = layer_norm(x, sd[p + "0.layer_norm.weight"], eps)
        q, k, v = ((h @ sd[p + f"0.SelfAttention.{c}.weight"].t()).view(B, L, H, dkv).transpose(1, 2) for c in "qkv")
        scores = q @ k.transpose(3, 2)
        scores = scores + bias
        w = torch.softmax(scores.to(wide), dim=-1).to(dt)
        ctx = (w @ v).transpose(1, 2).reshape(B, L, H * dkv)
        x = x + ctx @ sd[p + "0.SelfAttention.o.weight"].t()
        h = layer_norm(x, sd[p + "1.layer_norm.weight"], eps)
        g = gelu_new(h @ sd[p + "1.DenseReluDense.wi_0.weight"].t()) * (h @ sd[p + "1.DenseReluDense.wi_1.weight"].t())
        x = x + g @ sd[p + "1.DenseReluDense.wo.weight"].t()
    return layer_norm(x, sd["encoder.final_layer_norm.weight"], eps)


def errors(got, truth):
    """(max abs, rms) of got - truth in float64."""
    d = got.double().cpu() - truth.double().cpu()
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())
