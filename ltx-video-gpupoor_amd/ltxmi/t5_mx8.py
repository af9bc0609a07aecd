"""The four projections of a T5 block in MX-FP8 (the counterpart of ltxmi/ff_mx8.py and ltxmi/attn_mx8.py for the text encoder):
the per-module state that ``T5EncoderModel.quantize`` sets, and the launches a block makes when it is set.

Four linears of a block can be chosen, by these names:
  qkv   the stacked [q; k; v] projection; its input comes quantised from ``ops.rmsnorm_weight_mx8`` (no bf16 norm output exists);
  o     the attention output projection, residual into the stream; the attention context is quantised by ``ops.quantize_mx8``;
  wi    the stacked [wi_0; wi_1] projection, its input from ``ops.rmsnorm_weight_mx8`` as well;
  wo    the feed-forward output projection, residual into the stream; its input comes quantised from ``ops.gated_gelu_mx8``.
With all four a block is 9 launches (norm, qkv, attention, quantise, o, norm, wi, gated GELU, wo), one more than the bf16 block.
``shared.weight``, the relative-bias table and the norm weights stay bf16.

Up to ``ops.MXT_MAX_ROWS`` rows (batch x tokens) a quantised linear runs on ``ops.gemm_mx8_skinny``, above it on ``ops.gemm_mx8``;
the two give the same bits, so the choice is invisible.

A quantised ``T5Attention`` / ``T5DenseGatedActDense`` carries ``__dict__["_mx8"]``, a ``State`` that says which of its two linears
are quantised; without it the module's calls are the ones they were.  ``keep_bf16=True``: the bf16 parameters stay and the
quantised weights live in a ``derived.DerivedCache`` keyed on the parameters' storage and version, so an in-place edit quantises
again on the next forward and ``.to()`` is followed.  ``keep_bf16=False``: the quantised weights are held here (``sealed``) and the
bf16 weights of the chosen linears are freed, the stacked bf16 operands of ``loading.load_t5_encoder`` with them."""
import torch

from . import derived, ops

LINEARS = ("qkv", "o", "wi", "wo")
# The default of ``quantize(linears=None)``: the linears whose quantised call, the quantiser pass it needs included, was faster
# than the bf16 call it replaces at both measured row counts (profiles/t5_mx8.md).
DEFAULT_LINEARS = ("qkv", "o", "wi", "wo")
ATTENTION_LINEARS, FF_LINEARS = ("qkv", "o"), ("wi", "wo")


def resolve(linears):
    """``linears`` of ``quantize`` -> the chosen names in the order of ``LINEARS``; raises on an unknown name."""
    if linears is None:
        return DEFAULT_LINEARS
    chosen = tuple(linears)
    unknown = [n for n in chosen if n not in LINEARS]
    if unknown:
        raise ValueError(f"ltxmi: T5EncoderModel.quantize(): unknown linear {unknown[0]!r}; the choices are {', '.join(LINEARS)}")
    return tuple(n for n in LINEARS if n in chosen)


class State:
    __slots__ = ("chosen", "cache", "sealed")

    def __init__(self, chosen):
        self.chosen = frozenset(chosen)
        self.cache, self.sealed = derived.DerivedCache(capacity=2, layout=False), None


def modules(mod, name):
    """The ``nn.Linear`` members behind linear ``name`` of a ``T5Attention`` / ``T5DenseGatedActDense``."""
    return {"qkv": lambda: [mod.q, mod.k, mod.v], "o": lambda: [mod.o], "wi": lambda: [mod.wi_0, mod.wi_1], "wo": lambda: [mod.wo]}[name]()


def check(mod, name, where):
    """The shapes ``ltxmi_gemm_mx8`` takes (K % 128 == 0, N % 32 == 0) and bf16 weights, for linear ``name``."""
    for lin in modules(mod, name):
        w = lin.weight
        if w.dim() != 2 or w.shape[1] % 128 or w.shape[0] % 32:
            raise ValueError(f"ltxmi: T5EncoderModel.quantize(): {where} is {tuple(w.shape)}; the MX-FP8 GEMM needs in_features % 128 == 0 "
                             "and out_features % 32 == 0")
        if w.dtype != torch.bfloat16:
            raise TypeError(f"ltxmi: T5EncoderModel.quantize(): {where}.weight must be bfloat16, got {w.dtype}")


def weights(mod, name):
    """(wq, w_scales) of quantised linear ``name``; a stacked projection is quantised member by member into one [N, K] operand
    (a row's blocks are its own, so that is the stacked operand quantised), and no bf16 pack is built for it."""
    st = mod.__dict__["_mx8"]
    if st.sealed is not None:
        return st.sealed[name]
    ws = [m.weight for m in modules(mod, name)]

    def build():
        with torch.no_grad():
            if len(ws) == 1:
                return ops.quantize_mx8(ws[0])
            n, K = sum(w.shape[0] for w in ws), ws[0].shape[1]
            q = torch.empty((n, K), dtype=ops.E4M3, device=ws[0].device)
            s = torch.empty((n, K // 32), dtype=torch.uint8, device=ws[0].device)
            r = 0
            for w in ws:
                ops.quantize_mx8(w, out=(q[r:r + w.shape[0]], s[r:r + w.shape[0]]))
                r += w.shape[0]
            return q, s
    return st.cache.get(ws, (name,), build)


def seal(mod):
    """keep_bf16=False: hold the quantised weights here and free the bf16 weights of the chosen linears."""
    st = mod.__dict__["_mx8"]
    held = {name: weights(mod, name) for name in LINEARS if name in st.chosen}
    st.sealed = held
    st.cache.clear()
    for name in held:
        for lin in modules(mod, name):
            lin.weight.data = torch.empty(0, dtype=lin.weight.dtype, device=lin.weight.device)
    mod.invalidate_packed()                      # a stacked bf16 operand of a freed projection goes with it


def linear(mod, name, xq, **kw):
    """(e4m3, scales) rows @ quantised linear ``name``; the keywords are ``out``, ``epilogue`` and ``residual``."""
    wq, ws = weights(mod, name)
    if xq[0].shape[0] <= ops.MXT_MAX_ROWS:
        return ops.gemm_mx8_skinny(*xq, wq, ws, **kw)
    return ops.gemm_mx8(*xq, wq, ws, **kw)


def self_attention(att, norm, x, B, L, rel, key_bias):
    """``T5LayerSelfAttention.forward`` for a ``T5Attention`` that carries a ``State``: x [B * L, d_model], updated in place."""
    st = att.__dict__["_mx8"]
    if "qkv" in st.chosen:
        qkv = linear(att, "qkv", ops.rmsnorm_weight_mx8(x, norm.weight, norm.variance_epsilon))
    else:
        qkv = ops.gemm(norm(x), att._pack("qkv", [att.q, att.k, att.v]))
    qkv = qkv.view(B, L, 3, att.n_heads, att.d_kv)
    ctx = ops.attention_relbias(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], rel_bias=rel[0], rel_center=rel[1], key_bias=key_bias,
                                softmax_scale=1.0).view(B * L, att.inner_dim)
    if "o" in st.chosen:
        return linear(att, "o", ops.quantize_mx8(ctx), out=x, epilogue=ops.EPI_GATE_RESIDUAL, residual=x)
    return ops.gemm(ctx, att.o.weight, out=x, epilogue=ops.EPI_GATE_RESIDUAL, residual=x)


def feed_forward(ff, norm, x):
    """``T5LayerFF.forward`` for a ``T5DenseGatedActDense`` that carries a ``State``: x [rows, d_model], updated in place."""
    st = ff.__dict__["_mx8"]
    if "wi" in st.chosen:
        h = linear(ff, "wi", ops.rmsnorm_weight_mx8(x, norm.weight, norm.variance_epsilon))
    else:
        h = ops.gemm(norm(x), ff._pack("wi", [ff.wi_0, ff.wi_1]))
    if "wo" in st.chosen:
        return linear(ff, "wo", ops.gated_gelu_mx8(h), out=x, epilogue=ops.EPI_GATE_RESIDUAL, residual=x)
    return ops.gemm(ops.gated_gelu(h), ff.wo.weight, out=x, epilogue=ops.EPI_GATE_RESIDUAL, residual=x)
