"""``Transformer3DModel`` -- the LTX-Video DiT wrapper on libltxmi kernels.

Drop-in for ltx_video/models/transformers/transformer3d.py:46-507: same constructor arguments
(:50-81), same parameter names (so ``load_state_dict`` of a reference checkpoint works, incl.
the ``model.diffusion_model.`` prefix strip :257-269), same ``forward`` signature and return
convention (:328-345, :504-507), ``precompute_freqs_cis`` (:202-255) and
``create_skip_layer_mask`` (:171-186).

Weights live fully in HBM (3.85 GB bf16 for the 2B config): the reference's mmgp block
offloading has no counterpart here.
"""
import contextlib
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import torch
from torch import nn

from . import attn_mx8, ff_mx8, lora, ops
from .attention import BasicTransformerBlock, SkipLayerStrategy
from .derived import DerivedOwner, cache_key

BF16 = torch.bfloat16


@dataclass
class Transformer3DModelOutput:
    sample: torch.Tensor


class _TimestepEmbedder(nn.Module):            # diffusers TimestepEmbedding: keys linear_1 / linear_2
    def __init__(self, in_channels, dim):
        super().__init__()
        self.linear_1 = nn.Linear(in_channels, dim)
        self.linear_2 = nn.Linear(dim, dim)


class _CombinedTimestepEmbeddings(nn.Module):  # diffusers PixArtAlphaCombinedTimestepSizeEmbeddings
    def __init__(self, dim):
        super().__init__()
        self.timestep_embedder = _TimestepEmbedder(256, dim)

    def forward(self, timestep_f32):
        """timestep_f32: fp32 [n], already scaled.  sinusoid(256, flip, shift 0) -> linear_1 ->
        SiLU -> linear_2 (transformer3d.py:428-433 via AdaLayerNormSingle)."""
        proj = ops.timestep_embedding(timestep_f32.contiguous(), 256)
        te = self.timestep_embedder
        h = ops.gemm(proj, te.linear_1.weight, te.linear_1.bias, epilogue=ops.EPI_SILU)
        return ops.gemm(h, te.linear_2.weight, te.linear_2.bias)


class AdaLayerNormSingle(nn.Module):           # keys emb.timestep_embedder.linear_{1,2}, linear
    def __init__(self, embedding_dim, use_additional_conditions=False):
        super().__init__()
        assert not use_additional_conditions
        self.emb = _CombinedTimestepEmbeddings(embedding_dim)
        self.linear = nn.Linear(embedding_dim, 6 * embedding_dim, bias=True)

    def forward(self, timestep_f32):
        emb = self.emb(timestep_f32)
        return ops.gemm(ops.silu(emb), self.linear.weight, self.linear.bias), emb


class PixArtAlphaTextProjection(nn.Module):    # keys linear_1 / linear_2, GELU-tanh between
    def __init__(self, in_features, hidden_size):
        super().__init__()
        self.linear_1 = nn.Linear(in_features, hidden_size)
        self.linear_2 = nn.Linear(hidden_size, hidden_size)

    def forward(self, caption):
        h = ops.gemm(caption.reshape(-1, caption.shape[-1]), self.linear_1.weight, self.linear_1.bias,
                     epilogue=ops.EPI_GELU_TANH)
        return ops.gemm(h, self.linear_2.weight, self.linear_2.bias)


class _Config(dict):
    __getattr__ = dict.__getitem__


class Transformer3DModel(DerivedOwner, nn.Module):
    def __init__(self, num_attention_heads: int = 16, attention_head_dim: int = 88,
                 in_channels: Optional[int] = None, out_channels: Optional[int] = None, num_layers: int = 1,
                 dropout: float = 0.0, norm_num_groups: int = 32, cross_attention_dim: Optional[int] = None,
                 attention_bias: bool = False, num_vector_embeds: Optional[int] = None,
                 activation_fn: str = "geglu", num_embeds_ada_norm: Optional[int] = None,
                 use_linear_projection: bool = False, only_cross_attention: bool = False,
                 double_self_attention: bool = False, upcast_attention: bool = False,
                 adaptive_norm: str = "single_scale_shift", standardization_norm: str = "layer_norm",
                 norm_elementwise_affine: bool = True, norm_eps: float = 1e-5, attention_type: str = "default",
                 caption_channels: int = None, use_tpu_flash_attention: bool = False,
                 qk_norm: Optional[str] = None, positional_embedding_type: str = "rope",
                 positional_embedding_theta: Optional[float] = None,
                 positional_embedding_max_pos: Optional[List[int]] = None,
                 timestep_scale_multiplier: Optional[float] = None, causal_temporal_positioning: bool = False,
                 **ignored):
        super().__init__()
        self.config = _Config({k: v for k, v in locals().items() if k not in ("self", "ignored", "__class__")})
        if use_tpu_flash_attention:
            raise NotImplementedError("TPU flash attention does not exist on MI355X")
        if positional_embedding_type != "rope":
            raise ValueError("Absolute positional embedding is no longer supported")     # transformer3d.py:98-99
        if positional_embedding_theta is None or positional_embedding_max_pos is None:
            raise ValueError("rope needs positional_embedding_theta and positional_embedding_max_pos")
        self.num_attention_heads = num_attention_heads
        self.attention_head_dim = attention_head_dim
        inner_dim = num_attention_heads * attention_head_dim
        self.inner_dim = inner_dim
        self.in_channels = in_channels
        self.patchify_proj = nn.Linear(in_channels, inner_dim, bias=True)
        self.positional_embedding_theta = positional_embedding_theta
        self.positional_embedding_max_pos = positional_embedding_max_pos
        self.use_rope = True
        self.timestep_scale_multiplier = timestep_scale_multiplier
        self.transformer_blocks = nn.ModuleList([
            BasicTransformerBlock(inner_dim, num_attention_heads, attention_head_dim, dropout=dropout,
                                  cross_attention_dim=cross_attention_dim, activation_fn=activation_fn,
                                  num_embeds_ada_norm=num_embeds_ada_norm, attention_bias=attention_bias,
                                  only_cross_attention=only_cross_attention,
                                  double_self_attention=double_self_attention, upcast_attention=upcast_attention,
                                  adaptive_norm=adaptive_norm, standardization_norm=standardization_norm,
                                  norm_elementwise_affine=norm_elementwise_affine, norm_eps=norm_eps,
                                  attention_type=attention_type, qk_norm=qk_norm, use_rope=True)
            for _ in range(num_layers)])
        self.out_channels = in_channels if out_channels is None else out_channels
        self.scale_shift_table = nn.Parameter(torch.randn(2, inner_dim) / inner_dim ** 0.5)
        self.proj_out = nn.Linear(inner_dim, self.out_channels)
        self.adaln_single = AdaLayerNormSingle(inner_dim, use_additional_conditions=False)
        self.caption_projection = None
        if caption_channels is not None:
            self.caption_projection = PixArtAlphaTextProjection(caption_channels, inner_dim)

    # ------------------------------------------------------------------ properties
    @property
    def dtype(self):
        return self.patchify_proj.weight.dtype

    @property
    def device(self):
        return self.patchify_proj.weight.device

    @classmethod
    def from_config(cls, config):
        return cls(**{k: v for k, v in dict(config).items() if not k.startswith("_")})

    @classmethod
    def from_pretrained(cls, pretrained_model_path, *args, device="cuda", dtype=torch.bfloat16, **kwargs):
        """transformer3d.py:271-326: diffusers directory or single-file safetensors with a config blob."""
        from .loading import load_transformer
        return load_transformer(pretrained_model_path, device=device, dtype=dtype)

    def load_state_dict(self, state_dict: Dict, *args, **kwargs):              # transformer3d.py:257-269
        if any(k.startswith("model.diffusion_model.") for k in state_dict.keys()):
            state_dict = {k.replace("model.diffusion_model.", ""): v for k, v in state_dict.items()
                          if k.startswith("model.diffusion_model.")}
        self._refuse_ff_freed("load_state_dict")
        self._refuse_attn_freed("load_state_dict")
        st = lora.fused_state(self)
        if st is not None:
            if st.adapters and st.base:
                # the base copies would be those of the weights being replaced
                raise RuntimeError("unfuse_lora() first")
            del self.__dict__["_lora_fused"]         # only keep_base=False merges: the load replaces them, nothing is owed
        return super().load_state_dict(state_dict, *args, **kwargs)

    # ------------------------------------------------------------------ LoRA adapters (ltxmi/lora.py)
    def attach_lora(self, adapter, weight: float = 1.0, name: Optional[str] = None, strict: bool = True, mx8: bool = False):
        """Run ``adapter`` (``loading.load_lora``) unmerged on top of the base weights, at strength ``weight``; several
        adapters may be active at once.  Targets are the ten linears of every block.  An adapter that names another linear
        (patchify_proj, adaln_single.*, caption_projection.*, proj_out): ``strict=True`` raises and lists them,
        ``strict=False`` skips them.  Returns the list of skipped linears.  The reference: inference.py:483-493.
        ``mx8=True``: the adapter may name linears that ``quantize_ff`` / ``quantize_attention`` run in MX-FP8 (with the default
        that is refused); on those it runs as an MX-FP8 operand pair -- ``down``, ``T`` and ``bf16(s up)`` quantised, the K loop
        of the linear's own call continued (``lora.pair_mx8``) -- and on every other linear in bf16 as before.  It works on
        ``keep_bf16=False`` models.  The order is quantise, then attach; ``unquantize_*`` turns the pairs concerned into bf16 ones."""
        mine, other = lora.split_targets(adapter, len(self.transformer_blocks))
        if other and strict:
            raise ValueError("ltxmi: the adapter names linears outside the transformer blocks, which carry no adapter here: "
                             + ", ".join(other))
        lora.check_shapes(self, adapter, mine)
        if not mx8:
            self._refuse_ff_quantized(mine.values(), "attach_lora")
            self._refuse_attn_quantized(mine.values(), "attach_lora")
        active = self.__dict__.setdefault("_lora_adapters", lora.OrderedDict())
        if name is None:
            name = f"lora{len(active)}"
            while name in active:
                name += "_"
        if name in active:
            raise ValueError(f"ltxmi: an adapter named '{name}' is attached already")
        active[name] = [adapter, float(weight), mine]
        try:
            lora.rebuild(self)
        except Exception:
            del active[name]
            lora.rebuild(self)
            raise
        return other

    def set_lora_weights(self, weights: Dict[str, float]):
        """New strengths for attached adapters, by name; the base weights are not touched."""
        active = self.__dict__.get("_lora_adapters") or {}
        for name in weights:
            if name not in active:
                raise KeyError(f"ltxmi: no adapter named '{name}' is attached")
        for name, w in weights.items():
            active[name][1] = float(w)
        lora.rebuild(self)

    def detach_lora(self, name: Optional[str] = None):
        """Detach one adapter, or all of them: the model computes what it computed before ``attach_lora``, bit for bit."""
        active = self.__dict__.get("_lora_adapters") or {}
        if name is None:
            active.clear()
        elif name not in active:
            raise KeyError(f"ltxmi: no adapter named '{name}' is attached")
        else:
            del active[name]
        lora.rebuild(self)

    def lora_names(self):
        return list(self.__dict__.get("_lora_adapters") or {})

    # ------------------------------------------------------------------ LoRA adapters fused into the weights
    def fuse_lora(self, adapter, weight: float = 1.0, name: Optional[str] = None, keep_base: bool = True):
        """Fold ``adapter`` (``loading.load_lora``) into the weight of every linear it names, at strength ``weight``: the
        forward afterwards is the forward of a model without adapters, on ``bf16(W + sum s B A)`` -- one rounding, from an
        fp32 sum that includes the base weight, for ALL fused adapters of a linear together (``lora.merged_weight``).  Every
        linear of the model may be named, the seven outside the blocks included.  ``keep_base=True`` keeps a bf16 copy of the
        base weight of each fused linear, which is what ``unfuse_lora``, ``set_fused_lora_weights`` and a further
        ``fuse_lora`` on the same linear merge from; ``keep_base=False`` merges in place and keeps nothing, and those three
        then raise for the linears concerned.  Fused and attached adapters may coexist: the attached ones run on top."""
        paths = lora.fuse_paths(self, adapter)
        self._refuse_ff_quantized(paths, "fuse_lora")
        self._refuse_attn_quantized(paths, "fuse_lora")
        st = lora.fused_state(self)
        fused = st.adapters if st else {}
        if name is None:
            name = f"lora{len(fused)}"
            while name in fused:
                name += "_"
        if name in fused:
            raise ValueError(f"ltxmi: an adapter named '{name}' is fused already")
        self._refuse_sealed(paths, "fuse_lora")
        lora.check_mergeable(self, paths)                # before the first weight is written
        st = lora.fused_state(self, create=True)
        st.adapters[name] = [adapter, float(weight), paths]
        try:
            lora.remerge(self, paths, keep_base=keep_base)
        except Exception:
            if not st.sealed.intersection(paths):        # (nothing merged in place yet: back to the state before the call)
                del st.adapters[name]
                lora.remerge(self, paths)
            raise

    def _refuse_sealed(self, paths, what):
        st = lora.fused_state(self)
        gone = sorted(st.sealed.intersection(paths)) if st else []
        if gone:
            raise RuntimeError(f"ltxmi: {what}: an adapter was fused with keep_base=False into {gone[0]}"
                               + (f" and {len(gone) - 1} more linears" if len(gone) > 1 else "")
                               + "; the base weight is gone, so nothing can be merged from it again -- reload the checkpoint")

    def set_fused_lora_weights(self, weights: Dict[str, float]):
        """New strengths for fused adapters, by name: the linears they name are merged again from their bases, and hold the
        bits a fresh ``fuse_lora`` at those strengths gives."""
        st = lora.fused_state(self)
        fused = st.adapters if st else {}
        for name in weights:
            if name not in fused:
                raise KeyError(f"ltxmi: no adapter named '{name}' is fused")
        paths = list(dict.fromkeys(p for name in weights for p in fused[name][2]))
        self._refuse_sealed(paths, "set_fused_lora_weights")
        self._refuse_ff_quantized(paths, "set_fused_lora_weights", freed_only=True)
        self._refuse_attn_quantized(paths, "set_fused_lora_weights", freed_only=True)
        for name, w in weights.items():
            fused[name][1] = float(w)
        lora.remerge(self, paths)

    def unfuse_lora(self, name: Optional[str] = None):
        """Remove one fused adapter, or all of them, and merge what remains again; a linear no fused adapter names any more
        gets its base weight back bit for bit, and its base copy is freed."""
        st = lora.fused_state(self)
        fused = st.adapters if st else {}
        if name is not None and name not in fused:
            raise KeyError(f"ltxmi: no adapter named '{name}' is fused")
        names = list(fused) if name is None else [name]
        paths = list(dict.fromkeys(p for n in names for p in fused[n][2]))
        self._refuse_sealed(paths, "unfuse_lora")
        self._refuse_ff_quantized(paths, "unfuse_lora", freed_only=True)
        self._refuse_attn_quantized(paths, "unfuse_lora", freed_only=True)
        for n in names:
            del fused[n]
        lora.remerge(self, paths)
        if st is not None and not st.adapters and not st.sealed:
            del self.__dict__["_lora_fused"]

    def fused_lora_names(self):
        st = lora.fused_state(self)
        return list(st.adapters) if st else []

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        if self._ff_freed():                     # the held MX-FP8 weights follow the device (never a dtype: they are e4m3 / E8M0)
            dev = self.patchify_proj.weight.device
            for b in self.transformer_blocks:
                st = b.ff.__dict__["_mx8"]
                st.sealed = tuple(tuple(t.to(dev) for t in pair) for pair in st.sealed)
        for attn in self._quantized_attentions():    # the same for the attention linears held by quantize_attention(keep_bf16=False)
            st = attn.__dict__["_mx8"]
            if st.sealed is not None:
                dev = self.patchify_proj.weight.device
                st.sealed = {k: tuple(None if t is None else t.to(dev) for t in v) for k, v in st.sealed.items()}
        st = lora.fused_state(self)
        if st is not None:
            st.base = {path: fn(t) for path, t in st.base.items()}     # the base copies follow the weights (no parameters, no buffers)
        if self.__dict__.get("_lora_adapters"):
            lora.rebuild(self)                   # the per-linear state follows the weights' device
        return out

    # ------------------------------------------------------------------ MX-FP8 feed-forward (ltxmi/ff_mx8.py)
    FF_LINEARS = ("ff.net.0.proj", "ff.net.2")

    def quantize_ff(self, keep_bf16: bool = True):
        """Run the feed-forward pair of every block in MX-FP8 (e4m3 elements, one scale per 32 along K; the block-scaled MFMA):
        quantise(norm) -> FF1 (GELU, written as MX-FP8) -> FF2 (gate + residual; a plain bf16 output on the fp32 stream).  The
        weights are quantised from the bf16 tensors as they stand -- after ``fuse_lora``, the fused ones.  ``keep_bf16=True``: the
        bf16 parameters stay, ``state_dict()`` is unchanged, an in-place edit of a weight quantises it again, ``unquantize_ff()``
        gives the model back bit for bit.  ``keep_bf16=False``: the bf16 feed-forward weights are freed (5/8 of a block's linear
        bytes become 5/16); ``unquantize_ff``, ``state_dict`` and ``load_state_dict`` then raise.  Adapters on the attention
        linears are unaffected; one on a feed-forward linear has to be detached (or fused) first."""
        if self.ff_quantized:
            raise RuntimeError("ltxmi: quantize_ff(): the feed-forward is quantised already; unquantize_ff() first")
        ffs = [b.ff for b in self.transformer_blocks]
        for i, ff in enumerate(ffs):
            ff_mx8.check(ff)
            if lora.has_slot(ff, "ff1") or lora.has_slot(ff, "ff2"):
                raise RuntimeError(f"ltxmi: quantize_ff(): an adapter is attached to transformer_blocks.{i}.ff; detach_lora() "
                                   "first, or fuse_lora() it into the weights")
        for ff in ffs:
            ff.__dict__["_mx8"] = ff_mx8.FFState()
        if not keep_bf16:
            for ff in ffs:
                st = ff.__dict__["_mx8"]
                st.sealed = ff_mx8.weights(ff)
                st.cache.clear()
                for lin in (ff.net[0].proj, ff.net[2]):
                    lin.weight.data = torch.empty(0, dtype=lin.weight.dtype, device=lin.weight.device)
            st = lora.fused_state(self)
            if st is not None:                       # base copies of freed weights are of no use any more
                for path in [p for p in st.base if p.endswith(self.FF_LINEARS)]:
                    del st.base[path]
                    st.sealed.add(path)

    def unquantize_ff(self):
        """Back to the bf16 feed-forward: the model computes what it computed before ``quantize_ff``, bit for bit."""
        self._refuse_ff_freed("unquantize_ff")
        for b in self.transformer_blocks:
            b.ff.__dict__.pop("_mx8", None)
        self._rebuild_mx8_lora()

    @property
    def ff_quantized(self) -> bool:
        return any("_mx8" in b.ff.__dict__ for b in self.transformer_blocks)

    def _ff_freed(self):
        return any(b.ff.__dict__["_mx8"].sealed is not None for b in self.transformer_blocks if "_mx8" in b.ff.__dict__)

    def _refuse_ff_freed(self, what):
        if self._ff_freed():
            raise RuntimeError(f"ltxmi: {what}(): quantize_ff(keep_bf16=False) freed the bf16 feed-forward weights; reload the "
                               "checkpoint")

    def _refuse_ff_quantized(self, paths, what, freed_only=False):
        if (self._ff_freed() if freed_only else self.ff_quantized) and any(p.endswith(self.FF_LINEARS) for p in paths):
            raise RuntimeError(f"ltxmi: {what}(): the feed-forward is quantised and the adapter names ff.net.0.proj / ff.net.2; "
                               "unquantize_ff() first")

    # ------------------------------------------------------------------ MX-FP8 attention linears (ltxmi/attn_mx8.py)
    def quantize_attention(self, keep_bf16: bool = True, linears=None):
        """Run the per-step attention linears of every block in MX-FP8, the second switch beside ``quantize_ff`` (they compose, in
        either order).  ``linears``: a subset of ``attn_mx8.LINEARS`` = ("attn1.qkv", "attn1.to_out", "attn2.to_q",
        "attn2.to_out"); None takes ``attn_mx8.DEFAULT_LINEARS``, the measured choice.  attn1.qkv takes its input quantised
        straight from norm1 (``ops.norm_modulate_mx8``) and emits q's row sums; the to_out linears quantise the attention output
        and keep their gate + residual epilogue; ``attn2.to_k`` / ``to_v`` (once per generation) stay bf16.  The weights are
        quantised from the bf16 tensors as they stand -- after ``fuse_lora``, the fused ones.  ``keep_bf16`` as in
        ``quantize_ff``: True keeps the parameters (``state_dict()`` unchanged, an in-place edit quantises again,
        ``unquantize_attention()`` gives the model back bit for bit); False frees the bf16 weights of the chosen linears, and
        ``unquantize_attention``, ``state_dict`` and ``load_state_dict`` then raise.  An adapter attached to a chosen linear has
        to be detached (or fused) first; the sequence-parallel processors refuse a quantised attention."""
        from .attention import AttnProcessor2_0
        if self.attention_quantized:
            raise RuntimeError("ltxmi: quantize_attention(): the attention is quantised already; unquantize_attention() first")
        chosen = attn_mx8.resolve(linears)
        plan = []                                    # (attention module, {"proj": bool, "out": bool})
        for i, b in enumerate(self.transformer_blocks):
            for owner in ("attn1", "attn2"):
                attn = getattr(b, owner, None)
                names = [n for n in chosen if attn_mx8.PARTS[n][0] == owner]
                if attn is None or not names:
                    continue
                if type(attn.processor) is not AttnProcessor2_0:
                    raise NotImplementedError(f"ltxmi: quantize_attention(): transformer_blocks.{i}.{owner} runs "
                                              f"{type(attn.processor).__name__}; the MX-FP8 linears are AttnProcessor2_0's "
                                              "(disable_sequence_parallel() first)")
                for n in names:
                    attn_mx8.check(attn, attn_mx8.PARTS[n][1], f"transformer_blocks.{i}.{n}")
                    if lora.has_slot(attn, attn_mx8.LORA_SLOTS[n]):
                        raise RuntimeError(f"ltxmi: quantize_attention(): an adapter is attached to transformer_blocks.{i}.{n}; "
                                           "detach_lora() first, or fuse_lora() it into the weights")
                which = {attn_mx8.PARTS[n][1] for n in names}
                plan.append((attn, "proj" in which, "out" in which))
        for attn, proj, out in plan:
            attn.__dict__["_mx8"] = attn_mx8.AttnState(proj, out)
        self.__dict__["_mx8_attn_linears"] = chosen
        if not keep_bf16:
            for attn, _, _ in plan:
                attn_mx8.seal(attn)
            st = lora.fused_state(self)
            if st is not None:                       # base copies of freed weights are of no use any more
                for path in [p for p in st.base if p.endswith(self._attn_lora_suffixes())]:
                    del st.base[path]
                    st.sealed.add(path)

    def unquantize_attention(self):
        """Back to the bf16 attention linears: the model computes what it computed before ``quantize_attention``, bit for bit."""
        self._refuse_attn_freed("unquantize_attention")
        for attn in self._quantized_attentions():
            del attn.__dict__["_mx8"]
        self.__dict__.pop("_mx8_attn_linears", None)
        self._rebuild_mx8_lora()

    def _rebuild_mx8_lora(self):
        """After an ``unquantize_*``: adapters attached with ``mx8=True`` to the linears concerned become bf16 pairs, as if
        attached to the unquantised model.  Nothing is rebuilt (and no epoch moves) when no such pair exists."""
        owners = [o for b in self.transformer_blocks for o in (b.ff, b.attn1, getattr(b, "attn2", None)) if o is not None]
        if any(isinstance(s, lora.LoraSlotMx8) and not lora.runs_mx8(o, n)
               for o in owners for n, s in (o.__dict__.get("_lora") or {}).items()):
            lora.rebuild(self)

    @property
    def attention_quantized(self) -> bool:
        return bool(self.__dict__.get("_mx8_attn_linears"))

    def _quantized_attentions(self):
        return [a for b in self.transformer_blocks for a in (b.attn1, getattr(b, "attn2", None))
                if a is not None and "_mx8" in a.__dict__]

    def _attn_lora_suffixes(self):
        """The module-path endings by which an adapter names a quantised attention linear."""
        return tuple(p for n in self.__dict__.get("_mx8_attn_linears", ()) for p in attn_mx8.PARTS[n][2])

    def _attn_freed(self):
        return any(a.__dict__["_mx8"].sealed is not None for a in self._quantized_attentions())

    def _refuse_attn_freed(self, what):
        if self._attn_freed():
            raise RuntimeError(f"ltxmi: {what}(): quantize_attention(keep_bf16=False) freed the bf16 weights of the quantised "
                               "attention linears; reload the checkpoint")

    def _refuse_attn_quantized(self, paths, what, freed_only=False):
        if (self._attn_freed() if freed_only else self.attention_quantized) and any(p.endswith(self._attn_lora_suffixes()) for p in paths):
            raise RuntimeError(f"ltxmi: {what}(): the adapter names an attention linear that quantize_attention() runs in MX-FP8 ("
                               + ", ".join(self.__dict__["_mx8_attn_linears"]) + "); unquantize_attention() first")

    def state_dict(self, *args, **kwargs):
        self._refuse_ff_freed("state_dict")
        self._refuse_attn_freed("state_dict")
        return super().state_dict(*args, **kwargs)

    # ------------------------------------------------------------------ helpers kept verbatim
    def create_skip_layer_mask(self, batch_size: int, num_conds: int, ptb_index: int,
                               skip_block_list: Optional[List[int]] = None):     # transformer3d.py:171-186
        if skip_block_list is None or len(skip_block_list) == 0:
            return None
        num_layers = len(self.transformer_blocks)
        host = torch.ones((num_layers, batch_size * num_conds), dtype=torch.float32)
        for block_idx in skip_block_list:
            host[block_idx, ptb_index::num_conds] = 0
        mask = host.to(device=self.device, dtype=self.dtype)
        mask._ltxmi_host_rows = [[float(x) for x in row] for row in host.tolist()]
        return mask

    def get_fractional_positions(self, indices_grid):                          # transformer3d.py:192-200
        return torch.stack([indices_grid[:, i] / self.positional_embedding_max_pos[i] for i in range(3)], dim=-1)

    def precompute_freqs_cis(self, indices_grid, spacing="exp"):
        """transformer3d.py:202-255 -- once per generation, fp32 math, tables cast to the model
        dtype.  Host-side torch (not on the per-step path)."""
        if spacing != "exp":
            raise NotImplementedError("only the default 'exp' spacing is on this path")
        dtype = torch.float32
        dim = self.inner_dim
        theta = self.positional_embedding_theta
        frac = self.get_fractional_positions(indices_grid)
        indices = theta ** torch.linspace(math.log(1, theta), math.log(theta, theta), dim // 6,
                                          device=frac.device, dtype=dtype)
        indices = indices.to(dtype=dtype) * math.pi / 2
        freqs = (indices * (frac.unsqueeze(-1) * 2 - 1)).transpose(-1, -2).flatten(2)
        cos_freq = freqs.cos().repeat_interleave(2, dim=-1)
        sin_freq = freqs.sin().repeat_interleave(2, dim=-1)
        if dim % 6 != 0:
            cos_freq = torch.cat([torch.ones_like(cos_freq[:, :, : dim % 6]), cos_freq], dim=-1)
            sin_freq = torch.cat([torch.zeros_like(cos_freq[:, :, : dim % 6]), sin_freq], dim=-1)
        return cos_freq.to(self.dtype).contiguous(), sin_freq.to(self.dtype).contiguous()

    def _stacked_text_kv(self, ehs):
        """Every layer's text keys / values of this forward in ONE GEMM (attention.py:1042-1048 runs the projections once per
        block): ``ehs`` [B, T, D] against the stacked [to_k; to_v] of all cross-attention layers -> [B T, L 2D], each layer's
        key half RMS-normalised in place (k_norm, :1040-1041), each block's attn2 handed its column slice (a strided view, read
        by the attention kernel through its strides).  The values are those of the per-layer projections bit for bit: all GEMM
        kernels accumulate over K in the same order.  Stacked weights: built once, rebuilt when any source tensor changes."""
        blocks = [b for b in self.transformer_blocks if getattr(b, "attn2", None) is not None]
        if not blocks or ehs.dim() != 3 or not ehs.is_contiguous():
            return
        if any(lora.has_slot(b.attn2, "kv") for b in blocks):
            return          # an adapter on a to_k / to_v: the per-layer projections carry it (once per generation)
        packs = [b.attn2.packed_kv() for b in blocks]
        if any(bk is None for _, bk in packs) or len({tuple(w.shape) for w, _ in packs}) != 1:
            return

        def stack():
            with torch.no_grad():
                return torch.cat([w for w, _ in packs], 0).contiguous(), torch.cat([bk for _, bk in packs], 0).contiguous()
        w_all, b_all = self.derived("stacked_kv").get([t for pack in packs for t in pack], (), stack)
        Bk, Lk, _ = ehs.shape
        two_d = packs[0][0].shape[0]
        kv_all = ops.gemm(ehs.reshape(Bk * Lk, -1), w_all, b_all)                       # [B T, L 2D]
        for i, b in enumerate(blocks):
            kv = kv_all[:, i * two_d:(i + 1) * two_d]
            ops.rmsnorm_rope_(kv[:, :two_d // 2], b.attn2.k_norm.weight, b.attn2.k_norm.eps)
            b.attn2.__dict__["_text_kv_ready"] = (ehs, cache_key((ehs,)), kv, lora.epoch(b.attn2))

    def _run_blocks_microbatched(self, hidden_states, slices, freqs_cis, attention_mask, encoder_hidden_states,
                                 encoder_attention_mask, temb, cross_attention_kwargs, class_labels, layer_mask,
                                 skip_layer_strategy, ltxv_model):
        """The block loop over micro-batches of batch rows, micro-batch i on side stream i (plain sequential on the CPU).
        The host issues block b of every micro-batch before block b + 1 of any, so the collectives of the slices
        interleave in one fixed order on every rank.  The blocks update ``hidden_states`` in place through the row views.
        Returns True when interrupted."""
        B = hidden_states.shape[0]
        on_gpu = hidden_states.is_cuda
        streams = None
        # Everything that is created lazily and SHARED between the slices is created here, on the main stream, before the
        # side streams fork from it: the packed projection weights (``Attention._pack`` caches whatever the first caller
        # built -- on a fresh model, or after a reload / LoRA merge invalidated the packs, slice 1 on stream 1 would
        # otherwise take slice 0's cache entry while stream 0's torch.cat may still be writing it).
        for block in self.transformer_blocks:
            block.prepare_shared_state()
        if on_gpu:
            main = torch.cuda.current_stream()
            key = (hidden_states.device, len(slices))
            pool = self.__dict__.setdefault("_mb_streams", {})
            streams = pool.get(key)
            if streams is None:
                streams = pool[key] = [torch.cuda.Stream(device=hidden_states.device) for _ in slices]
            for st in streams:
                st.wait_stream(main)

        def rows(t, sl):
            return t if (t is None or t.shape[0] != B) else t[sl]

        interrupted = False
        for block_idx, block in enumerate(self.transformer_blocks):
            for i, sl in enumerate(slices):
                ctx = torch.cuda.stream(streams[i]) if on_gpu else contextlib.nullcontext()
                with ctx:
                    block(hidden_states[sl], freqs_cis=tuple(rows(t, sl) for t in freqs_cis), attention_mask=attention_mask,
                          encoder_hidden_states=rows(encoder_hidden_states, sl),
                          encoder_attention_mask=rows(encoder_attention_mask, sl), timestep=temb[sl],
                          cross_attention_kwargs=cross_attention_kwargs, class_labels=class_labels,
                          skip_layer_mask=layer_mask(block_idx, sl), skip_layer_strategy=skip_layer_strategy)
            if ltxv_model is not None and ltxv_model._interrupt:
                interrupted = True
                break
        if on_gpu:
            for st in streams:
                main.wait_stream(st)
        return interrupted

    # ------------------------------------------------------------------ forward
    def forward(self, hidden_states: torch.Tensor, freqs_cis: list,
                encoder_hidden_states: Optional[torch.Tensor] = None, timestep: Optional[torch.Tensor] = None,
                class_labels: Optional[torch.LongTensor] = None, cross_attention_kwargs: Dict[str, Any] = None,
                attention_mask: Optional[torch.Tensor] = None, encoder_attention_mask: Optional[torch.Tensor] = None,
                skip_layer_mask: Optional[torch.Tensor] = None,
                skip_layer_strategy: Optional[SkipLayerStrategy] = None, latent_shape=None, joint_pass=True,
                ltxv_model=None, mixed=False, return_dict: bool = True, stg_alias_blocks: int = 0,
                stg_alias_rows: int = 1, _microbatches=None):
        """``stg_alias_blocks`` (extension, default off): the caller guarantees that the LAST batch row has
        exactly the inputs of the row before it (the STG "perturbed" row is the text row until its first
        skipped block, pipeline_ltx_video.py:1035-1051) -- the first ``stg_alias_blocks`` blocks then run on
        B - 1 rows and the last row is filled in by a copy.  Bit-identical to running all rows: every kernel
        computes a row independently of the others, the GEMM kernels all accumulate over K in the same order and share
        their epilogue arithmetic (so the tile choice made from M does not matter), and the request is ignored when
        B - 1 and B rows would be served by different self-attention kernels (``ops.attention_kernel_id``).
        ``stg_alias_rows`` = r (default 1: the above): with r videos in the call the batch is chunked (uncond x r, text x r,
        perturbed x r), so the last r rows have the inputs of the r rows before them; the leading blocks run on B - r rows
        and the last r rows are filled by one copy.
        ``_microbatches`` (extension, set by ltxmi.distributed): a list of batch-row slices; the block loop then runs
        every block once per slice, each slice on a stream of its own, so that one slice's collectives (sequence
        parallelism) are hidden behind the other slices' kernels.  Rows are independent: same result.
        ``mixed`` (transformer3d.py:439-442): the residual stream is fp32 from the input projection to the output norm, the
        linears, q/k norms and attention stay bf16 (``BasicTransformerBlock._forward_stream32``); the output is bf16 either
        way.  Sequence parallelism (ltxmi.distributed) refuses it."""
        if self.dtype != BF16:
            raise TypeError("ltxmi.Transformer3DModel runs in bfloat16 only: call .to(torch.bfloat16)")
        if attention_mask is not None:
            raise NotImplementedError("a self-attention mask is not on this path")
        dtype = self.dtype
        hidden_states = hidden_states.to(dtype)
        B, N, _ = hidden_states.shape
        D = self.inner_dim

        # mask -> additive bias (keep +0 / discard -10000), transformer3d.py:411-415
        if encoder_attention_mask is not None and encoder_attention_mask.ndim == 2:
            encoder_attention_mask = ((1 - encoder_attention_mask.to(dtype)) * -10000.0).unsqueeze(1)

        # 1. input projection
        hidden_states = ops.gemm(hidden_states.reshape(B * N, -1), self.patchify_proj.weight,
                                 self.patchify_proj.bias).view(B, N, D)

        # timestep: [B,1] (t2v) or per-token [B,N] -> per-frame [B,F] (:420-425)
        timestep = timestep.to(torch.float32)
        if self.timestep_scale_multiplier:
            timestep = self.timestep_scale_multiplier * timestep
        if timestep.shape[-1] > 1:
            timestep = timestep.reshape(timestep.shape[0], -1, latent_shape[-2] * latent_shape[-1])[:, :, 0]
        temb, embedded_timestep = self.adaln_single(timestep.flatten())
        temb = temb.view(B, -1, 6 * D)
        embedded_timestep = embedded_timestep.view(B, -1, D)
        if mixed:
            # transformer3d.py:439-442: the residual stream goes to fp32 here (exact: the values are bf16's) and stays fp32
            # through the blocks and the output norm.  `timestep` and `embedded_timestep` are upcast there too: their values
            # stay bf16's, and the row kernels of the fp32 stream widen them on load, so they keep their storage.
            hidden_states = hidden_states.float()

        # 2. text projection
        if self.caption_projection is not None:
            # the prompt does not change between the denoise steps of a generation: project it once per
            # (prompt tensor, weights and biases) and hand the SAME tensor to the blocks, whose text K/V caches key on it
            ehs = encoder_hidden_states
            cp = self.caption_projection
            encoder_hidden_states = self.derived("caption", 4, True).get(
                (ehs, cp.linear_1.weight, cp.linear_1.bias, cp.linear_2.weight, cp.linear_2.bias), (),
                lambda: cp(ehs.to(dtype)).view(B, -1, D), enabled=ops.STEP_INVARIANT_CACHING)

        if joint_pass and ops.STACKED_TEXT_KV and not ops.STEP_INVARIANT_CACHING and encoder_hidden_states is not None:
            self._stacked_text_kv(encoder_hidden_states)

        host_rows = None
        if skip_layer_mask is not None:
            host_rows = getattr(skip_layer_mask, "_ltxmi_host_rows", None)
            if host_rows is None:                      # one D2H copy per forward instead of one per block
                host_rows = [[float(x) for x in row] for row in skip_layer_mask.float().cpu().tolist()]

        def layer_mask(block_idx, sl=None):
            if skip_layer_mask is None:
                return None
            m = skip_layer_mask[block_idx] if sl is None else skip_layer_mask[block_idx, sl]
            rows = host_rows[block_idx]
            m._ltxmi_host = rows if sl is None else rows[sl]
            return m

        first_block = 0
        r = int(stg_alias_rows)
        if stg_alias_blocks and r < 1:
            raise ValueError(f"ltxmi.Transformer3DModel: stg_alias_rows={stg_alias_rows} must be at least 1")
        if joint_pass and stg_alias_blocks and B >= 2 * r:
            heads, dh = self.num_attention_heads, self.attention_head_dim
            if ops.attention_kernel_id(B, heads, N, N, dh) != ops.attention_kernel_id(B - r, heads, N, N, dh):
                stg_alias_blocks = 0                                        # a sub-batch would not reproduce the full batch's bits
        if joint_pass and stg_alias_blocks and B >= 2 * r:
            first_block = min(int(stg_alias_blocks), len(self.transformer_blocks))
            keep = slice(0, B - r)
            hs = hidden_states[keep]                                        # a view: the blocks update it in place
            for block_idx in range(first_block):
                self.transformer_blocks[block_idx](
                    hs, freqs_cis=freqs_cis, attention_mask=attention_mask,
                    encoder_hidden_states=encoder_hidden_states[keep],
                    encoder_attention_mask=None if encoder_attention_mask is None else encoder_attention_mask[keep],
                    timestep=temb[keep], cross_attention_kwargs=cross_attention_kwargs, class_labels=class_labels,
                    skip_layer_mask=layer_mask(block_idx, keep), skip_layer_strategy=skip_layer_strategy)
                if ltxv_model is not None and ltxv_model._interrupt:
                    return [None]
            hidden_states[B - r:].copy_(hidden_states[B - 2 * r:B - r])
        if joint_pass and _microbatches and len(_microbatches) > 1 and first_block == 0:
            if self._run_blocks_microbatched(hidden_states, _microbatches, freqs_cis, attention_mask, encoder_hidden_states,
                                             encoder_attention_mask, temb, cross_attention_kwargs, class_labels,
                                             layer_mask, skip_layer_strategy, ltxv_model):
                return [None]
        elif joint_pass:
            for block_idx, block in enumerate(self.transformer_blocks):
                if block_idx < first_block:
                    continue
                hidden_states = block(hidden_states, freqs_cis=freqs_cis, attention_mask=attention_mask,
                                      encoder_hidden_states=encoder_hidden_states,
                                      encoder_attention_mask=encoder_attention_mask, timestep=temb,
                                      cross_attention_kwargs=cross_attention_kwargs, class_labels=class_labels,
                                      skip_layer_mask=layer_mask(block_idx),
                                      skip_layer_strategy=skip_layer_strategy)
                if ltxv_model is not None and ltxv_model._interrupt:        # cooperative cancel, :468-469
                    return [None]
        else:
            # one cond at a time so a perturbed (STG) row can skip attention entirely (:471-487)
            for block_idx, block in enumerate(self.transformer_blocks):
                for i in range(B):
                    block(hidden_states[i:i + 1], freqs_cis=freqs_cis, attention_mask=attention_mask,
                          encoder_hidden_states=encoder_hidden_states[i:i + 1],
                          encoder_attention_mask=encoder_attention_mask[i:i + 1], timestep=temb[i:i + 1],
                          cross_attention_kwargs=cross_attention_kwargs, class_labels=class_labels,
                          skip_layer_mask=layer_mask(block_idx, slice(i, i + 1)),
                          skip_layer_strategy=skip_layer_strategy)
                    if ltxv_model is not None and ltxv_model._interrupt:
                        return [None]

        for block in self.transformer_blocks:                                    # this forward's hand-over ends here
            if getattr(block, "attn2", None) is not None:
                block.attn2.__dict__.pop("_text_kv_ready", None)

        # 3. output: LayerNorm (no affine, 1e-6) -> (1 + scale) x + shift -> proj_out (:489-503)
        T1 = embedded_timestep.shape[1]
        emb2 = embedded_timestep.reshape(B * T1, D)
        if mixed:
            normed = torch.empty((B, N, D), dtype=dtype, device=hidden_states.device)
            ops.norm_modulate_f32in(hidden_states.view(B * N, D), normed.view(B * N, D), 1e-6, ops.NORM_LAYER,
                                    self.scale_shift_table[1], emb2, self.scale_shift_table[0], emb2, N // T1)
        else:
            normed = torch.empty_like(hidden_states)
            ops.norm_modulate(hidden_states.view(B * N, D), normed.view(B * N, D), 1e-6, ops.NORM_LAYER,
                              self.scale_shift_table[1], emb2, self.scale_shift_table[0], emb2, N // T1)
        out = ops.gemm(normed.view(B * N, D), self.proj_out.weight, self.proj_out.bias).view(B, N, -1)
        if not return_dict:
            return (out,)
        return Transformer3DModelOutput(sample=out)
