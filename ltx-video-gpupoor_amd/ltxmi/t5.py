"""T5-v1.1 text encoder on the library's kernels: the model the reference pipeline calls in ``encode_prompt``
(pipeline_ltx_video.py:405-417 for the prompt, :449-461 for the negative one; ltxv.py:200-209 loads the bf16 XXL encoder).

The arithmetic restated is the eager bf16 forward of Hugging Face ``transformers``' ``modeling_t5.py`` (T5EncoderModel):
embedding, per block T5LayerNorm -> unscaled self-attention with the bucketed relative position bias of block 0 and the
padding mask -> residual, T5LayerNorm -> gated tanh-GELU feed-forward -> residual, and the final T5LayerNorm.  Parameter
names are HF's, so its state dict loads with ``strict=True``.  Nine launches per block:

    norm, QKV GEMM, attention, o GEMM + residual, norm, [wi_0; wi_1] GEMM, gated GELU, wo GEMM + residual  (+ the final norm)

Where the rounding differs from HF's eager bf16 run, it is towards fewer roundings: the scores stay fp32 from the matrix
pipe to the softmax (HF rounds q k^T, and again after adding the bias, to bf16), and the residual add happens on the fp32
accumulator of the o / wo GEMM (HF rounds the linear's output, then the sum).  The norms and the gated activation round
exactly where T5LayerNorm and T5DenseGatedActDense round.

``T5EncoderModel.quantize()`` runs the four projections of every block in MX-FP8 (ltxmi/t5_mx8.py); a model that was never
quantised makes exactly the launches above.

The tokenizer (sentencepiece, on the CPU) stays the caller's."""
import collections
import math

import torch
from torch import nn

from . import ops, t5_mx8
from .derived import DerivedOwner

MAX_TOKENS = 512                     # ltxmi_attention_relbias_bf16: a query's score row is held in registers

T5EncoderOutput = collections.namedtuple("T5EncoderOutput", ["last_hidden_state"])

_CONFIG_DEFAULTS = dict(relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6,
                        feed_forward_proj="gated-gelu", is_decoder=False)
_CONFIG_REQUIRED = ("d_model", "d_kv", "d_ff", "num_heads", "num_layers", "vocab_size")


class T5Config:
    """The fields of HF's T5Config this encoder reads (a dict, an HF config object or keyword arguments)."""

    def __init__(self, config=None, **kw):
        if config is None:
            src = {}
        elif isinstance(config, dict):
            src = dict(config)
        else:
            src = {k: getattr(config, k) for k in (*_CONFIG_REQUIRED, *_CONFIG_DEFAULTS) if hasattr(config, k)}
        src.update(kw)
        missing = [k for k in _CONFIG_REQUIRED if k not in src]
        if missing:
            raise ValueError(f"ltxmi.T5Config: missing {missing}")
        for k in _CONFIG_REQUIRED:
            setattr(self, k, int(src[k]))
        for k, default in _CONFIG_DEFAULTS.items():
            setattr(self, k, type(default)(src.get(k, default)))
        if self.feed_forward_proj != "gated-gelu":
            raise NotImplementedError(f"ltxmi.T5EncoderModel: feed_forward_proj={self.feed_forward_proj!r} is not on this path "
                                      "(T5 v1.1's gated-gelu only)")
        if self.d_kv != 64:
            raise NotImplementedError(f"ltxmi.T5EncoderModel: d_kv={self.d_kv} is not on this path (the attention kernel takes "
                                      "head_dim 64)")
        if self.is_decoder:
            raise NotImplementedError("ltxmi.T5EncoderModel: is_decoder is not on this path (encoder only)")

    def to_dict(self):
        return {k: getattr(self, k) for k in (*_CONFIG_REQUIRED, *_CONFIG_DEFAULTS)}


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """HF's bidirectional ``T5Attention._relative_position_bucket`` restated: relative_position = key - query (a long
    tensor); half the buckets for positive offsets, exact below num_buckets / 4, logarithmic up to max_distance, with the
    float32 log and the truncation towards zero as torch does them on the CPU."""
    rel = torch.as_tensor(relative_position, dtype=torch.long).cpu()
    half = num_buckets // 2
    buckets = (rel > 0).to(torch.long) * half
    n = rel.abs()
    max_exact = half // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (half - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, half - 1))
    return buckets + torch.where(n < max_exact, n, large)


def build_rel_bias(weight, Lq, Lk, num_buckets=32, max_distance=128):
    """The ``rel_bias`` operand of ``ops.attention_relbias`` from ``relative_attention_bias.weight`` [num_buckets, H]:
    (fp32 [H, Lq + Lk - 1] on the weight's device, center = Lq - 1) with operand[h, center + d] = weight[bucket(d), h] for
    every offset d = key - query of an Lq x Lk call."""
    d = torch.arange(-(Lq - 1), Lk, dtype=torch.long)
    idx = relative_position_bucket(d, num_buckets, max_distance).to(weight.device)
    return weight.detach()[idx].to(torch.float32).t().contiguous(), Lq - 1


class T5LayerNorm(nn.Module):
    def __init__(self, d_model, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d_model))
        self.variance_epsilon = eps

    def forward(self, x, out=None):
        return ops.rmsnorm_weight(x, self.weight, self.variance_epsilon, out=out)


class _Packs(DerivedOwner):
    """Stacked GEMM operands ([q; k; v], [wi_0; wi_1]) built on first use and cached against their source parameters
    (ltxmi/derived.py), as the DiT's Attention does."""

    def _pack(self, slot, mods):
        return self._packed_linears(slot, mods)[0]

    def _share_packed(self, slot, mods):
        """For a frozen encoder (``loading.load_t5_encoder``): build the stacked operand once and re-point the members'
        weights at its row blocks, so that the operand is no second copy of them.  ``.to()`` / ``load_state_dict`` drop the
        arrangement (the next forward then packs a copy, as for a model built by hand)."""
        with torch.no_grad():
            packed = torch.cat([m.weight.detach() for m in mods], 0).contiguous()
        row = 0
        for m in mods:
            n = m.weight.shape[0]
            m.weight = nn.Parameter(packed[row:row + n], requires_grad=False)
            row += n
        self.derived(slot).put([t for m in mods for t in (m.weight, m.bias)], (), (packed, None))


class T5Attention(_Packs, nn.Module):
    def __init__(self, cfg, has_relative_attention_bias):
        super().__init__()
        inner = cfg.num_heads * cfg.d_kv
        self.n_heads, self.d_kv, self.inner_dim = cfg.num_heads, cfg.d_kv, inner
        self.q = nn.Linear(cfg.d_model, inner, bias=False)
        self.k = nn.Linear(cfg.d_model, inner, bias=False)
        self.v = nn.Linear(cfg.d_model, inner, bias=False)
        self.o = nn.Linear(inner, cfg.d_model, bias=False)
        if has_relative_attention_bias:
            self.relative_attention_bias = nn.Embedding(cfg.relative_attention_num_buckets, cfg.num_heads)

    def share_packed(self):
        self._share_packed("qkv", [self.q, self.k, self.v])

    def forward(self, normed, residual, B, L, rel, key_bias):
        """normed, residual: [B * L, d_model]; the residual stream is updated in place and returned."""
        qkv = ops.gemm(normed, self._pack("qkv", [self.q, self.k, self.v])).view(B, L, 3, self.n_heads, self.d_kv)
        ctx = ops.attention_relbias(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], rel_bias=rel[0], rel_center=rel[1],
                                    key_bias=key_bias, softmax_scale=1.0)
        return ops.gemm(ctx.view(B * L, self.inner_dim), self.o.weight, out=residual, epilogue=ops.EPI_GATE_RESIDUAL,
                        residual=residual)


class T5LayerSelfAttention(nn.Module):
    def __init__(self, cfg, has_relative_attention_bias):
        super().__init__()
        self.SelfAttention = T5Attention(cfg, has_relative_attention_bias)
        self.layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)

    def forward(self, x, B, L, rel, key_bias):
        if "_mx8" in self.SelfAttention.__dict__:                # T5EncoderModel.quantize(): ltxmi/t5_mx8.py
            return t5_mx8.self_attention(self.SelfAttention, self.layer_norm, x, B, L, rel, key_bias)
        return self.SelfAttention(self.layer_norm(x), x, B, L, rel, key_bias)


class T5DenseGatedActDense(_Packs, nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.wi_0 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wi_1 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wo = nn.Linear(cfg.d_ff, cfg.d_model, bias=False)

    def share_packed(self):
        self._share_packed("wi", [self.wi_0, self.wi_1])

    def forward(self, normed, residual):
        h = ops.gemm(normed, self._pack("wi", [self.wi_0, self.wi_1]))
        return ops.gemm(ops.gated_gelu(h), self.wo.weight, out=residual, epilogue=ops.EPI_GATE_RESIDUAL, residual=residual)


class T5LayerFF(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.DenseReluDense = T5DenseGatedActDense(cfg)
        self.layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)

    def forward(self, x):
        if "_mx8" in self.DenseReluDense.__dict__:               # T5EncoderModel.quantize(): ltxmi/t5_mx8.py
            return t5_mx8.feed_forward(self.DenseReluDense, self.layer_norm, x)
        return self.DenseReluDense(self.layer_norm(x), x)


class T5Block(nn.Module):
    def __init__(self, cfg, has_relative_attention_bias):
        super().__init__()
        self.layer = nn.ModuleList([T5LayerSelfAttention(cfg, has_relative_attention_bias), T5LayerFF(cfg)])


class T5Stack(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.block = nn.ModuleList([T5Block(cfg, i == 0) for i in range(cfg.num_layers)])
        self.final_layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)


_REFUSED = {
    "inputs_embeds": "the encoder starts from token ids",
    "head_mask": "every head takes part",
    "output_attentions": "the attention weights never leave the kernel",
    "output_hidden_states": "only the last hidden state is kept",
    "decoder_input_ids": "encoder only", "decoder_attention_mask": "encoder only", "decoder_inputs_embeds": "encoder only",
    "encoder_hidden_states": "encoder only", "encoder_attention_mask": "encoder only", "encoder_outputs": "encoder only",
    "past_key_values": "encoder only, no cache", "use_cache": "encoder only, no cache", "cache_position": "encoder only, no cache",
    "cross_attn_head_mask": "encoder only", "decoder_head_mask": "encoder only",
}


class T5EncoderModel(DerivedOwner, nn.Module):
    """``transformers.T5EncoderModel`` for inference on the GPU, with the HF call protocol ``encode_prompt`` uses:
    ``model(input_ids, attention_mask=mask)[0]`` is the last hidden state [B, L, d_model] in bf16."""

    def __init__(self, config=None, **kw):
        super().__init__()
        self.config = cfg = config if isinstance(config, T5Config) and not kw else T5Config(config, **kw)
        self.shared = nn.Embedding(cfg.vocab_size, cfg.d_model)
        self.encoder = T5Stack(cfg)

    @property
    def dtype(self):
        return self.shared.weight.dtype

    @property
    def device(self):
        return self.shared.weight.device

    def load_state_dict(self, state_dict, strict=True, **kw):
        """HF's names; ``encoder.embed_tokens.weight`` (HF ties it to ``shared.weight`` and saves both) is an alias."""
        self._refuse_freed("load_state_dict")
        sd = dict(state_dict)
        alias = sd.pop("encoder.embed_tokens.weight", None)
        if alias is not None:
            sd.setdefault("shared.weight", alias)
        return super().load_state_dict(sd, strict=strict, **kw)

    def state_dict(self, *args, **kwargs):
        self._refuse_freed("state_dict")
        return super().state_dict(*args, **kwargs)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        dev = self.shared.weight.device
        for mod in self._quantized_modules():        # weights held by quantize(keep_bf16=False) follow the device (never a dtype)
            st = mod.__dict__["_mx8"]
            if st.sealed is not None:
                st.sealed = {name: tuple(t.to(dev) for t in pair) for name, pair in st.sealed.items()}
        return out

    # ------------------------------------------------------------------ MX-FP8 projections (ltxmi/t5_mx8.py)
    def _linear_owners(self):
        for i, block in enumerate(self.encoder.block):
            yield f"encoder.block.{i}.layer.0.SelfAttention", block.layer[0].SelfAttention, t5_mx8.ATTENTION_LINEARS
            yield f"encoder.block.{i}.layer.1.DenseReluDense", block.layer[1].DenseReluDense, t5_mx8.FF_LINEARS

    def _quantized_modules(self):
        return [mod for _, mod, _ in self._linear_owners() if "_mx8" in mod.__dict__]

    def quantize(self, keep_bf16: bool = True, linears=None):
        """Run the projections of every block in MX-FP8 (e4m3 elements, one scale per 32 along K; the block-scaled MFMA) on the
        small-M GEMM ``ops.gemm_mx8_skinny``.  ``linears``: a subset of ``t5_mx8.LINEARS`` = ("qkv", "o", "wi", "wo"); None takes
        ``t5_mx8.DEFAULT_LINEARS``, the measured choice.  The weights are quantised from the bf16 tensors as they stand; the
        embedding, the relative-bias table and the norm weights stay bf16.  ``keep_bf16=True``: the bf16 parameters stay,
        ``state_dict()`` is unchanged, an in-place edit of a weight quantises it again, ``unquantize()`` gives the model back bit
        for bit.  ``keep_bf16=False``: the bf16 weights of the chosen linears are freed; ``unquantize``, ``state_dict`` and
        ``load_state_dict`` then raise."""
        if self.quantized:
            raise RuntimeError("ltxmi: T5EncoderModel.quantize(): the encoder is quantised already; unquantize() first")
        chosen = t5_mx8.resolve(linears)
        plan = []
        for path, mod, names in self._linear_owners():
            mine = [n for n in names if n in chosen]
            for n in mine:
                t5_mx8.check(mod, n, f"{path}.{n}")
            if mine:
                plan.append((mod, mine))
        if not keep_bf16 and not self.shared.weight.is_cuda:
            raise TypeError("ltxmi: T5EncoderModel.quantize(keep_bf16=False): the weights are quantised on the GPU; move the "
                            f"encoder there first (it is on {self.shared.weight.device})")
        for mod, mine in plan:
            mod.__dict__["_mx8"] = t5_mx8.State(mine)
        self.__dict__["_mx8_linears"] = chosen
        if not keep_bf16:
            for mod, _ in plan:
                t5_mx8.seal(mod)
        return self

    def unquantize(self):
        """Back to the bf16 projections: the encoder computes what it computed before ``quantize``, bit for bit."""
        self._refuse_freed("unquantize")
        for mod in self._quantized_modules():
            del mod.__dict__["_mx8"]
        self.__dict__.pop("_mx8_linears", None)
        return self

    @property
    def quantized(self):
        return bool(self.__dict__.get("_mx8_linears"))

    @property
    def quantized_linears(self):
        return tuple(self.__dict__.get("_mx8_linears", ()))

    def _refuse_freed(self, what):
        if any(mod.__dict__["_mx8"].sealed is not None for mod in self._quantized_modules()):
            raise RuntimeError(f"ltxmi: T5EncoderModel.{what}(): quantize(keep_bf16=False) freed the bf16 weights of the quantised "
                               "linears (" + ", ".join(self.quantized_linears) + "); reload the encoder")

    def rel_bias(self, L):
        """Block 0's bias table expanded over the offsets of an L x L call, once per (L, weight version); every block reads it."""
        w = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        cfg = self.config
        return self.derived("rel_bias").get((w,), (L,), lambda: build_rel_bias(
            w, L, L, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance))

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, return_dict=None, **kwargs):
        for name, value in kwargs.items():
            if value is None or value is False:
                continue
            raise NotImplementedError(f"ltxmi.T5EncoderModel: {name} is not on this path "
                                      f"({_REFUSED.get(name, 'not an argument of the encoder forward')})")
        if input_ids is None:
            raise NotImplementedError("ltxmi.T5EncoderModel: inputs_embeds is not on this path (the encoder starts from token ids)")
        if input_ids.dim() != 2:
            raise ValueError(f"ltxmi.T5EncoderModel: input_ids must be [batch, tokens], got {tuple(input_ids.shape)}")
        B, L = input_ids.shape
        if L > MAX_TOKENS:
            raise NotImplementedError(f"ltxmi.T5EncoderModel: {L} tokens is not on this path (at most {MAX_TOKENS}: the attention "
                                      "kernel holds a query's score row in registers)")
        if self.dtype != torch.bfloat16:
            raise TypeError(f"ltxmi.T5EncoderModel: the encoder runs in bfloat16, the weights are {self.dtype} (use .to(torch.bfloat16))")
        dev = self.device
        key_bias = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, L):
                raise ValueError(f"ltxmi.T5EncoderModel: attention_mask must be [batch, tokens] = {(B, L)}")
            # HF adds (1 - mask) * finfo(dtype).min to the scores; in this library that value means "the key is removed"
            key_bias = torch.zeros((B, L), dtype=torch.float32, device=dev).masked_fill_(attention_mask.to(dev) == 0, -math.inf)
        x = ops.embedding(input_ids.to(device=dev, dtype=torch.long), self.shared.weight).view(B * L, self.config.d_model)
        rel = self.rel_bias(L)
        for block in self.encoder.block:
            x = block.layer[0](x, B, L, rel, key_bias)
            x = block.layer[1](x)
        out = self.encoder.final_layer_norm(x).view(B, L, self.config.d_model)
        return T5EncoderOutput(out)
