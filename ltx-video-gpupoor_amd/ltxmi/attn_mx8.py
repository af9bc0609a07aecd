"""The per-step attention linears of a DiT block in MX-FP8 (the counterpart of ltxmi/ff_mx8.py): the per-``Attention`` state that
``Transformer3DModel.quantize_attention`` sets, and the launches ``AttnProcessor2_0`` makes when it is set.

Four linears of a block can be chosen, by these names:
  attn1.qkv      the packed [to_q; to_k; to_v] projection of the self-attention; its input comes quantised from
                 ``ops.norm_modulate_mx8`` (no bf16 norm1 output exists), and its epilogue emits q's row sums of squares;
  attn1.to_out   to_out.0 of the self-attention, gate + residual into the stream;
  attn2.to_q     to_q of the cross-attention (the stream is quantised for it), with q's row sums;
  attn2.to_out   to_out.0 of the cross-attention, residual into the stream.
``attn2.to_k`` / ``to_v`` run once per generation on the text and stay bf16.

A quantised ``Attention`` carries ``__dict__["_mx8"]``, an ``AttnState`` that says which of its two linears (``proj``: the q / qkv
projection, ``out``: to_out.0) are quantised; without it the processor's calls are the ones they were.  ``keep_bf16=True``: the
bf16 parameters stay and the quantised weights live in a ``derived.DerivedCache`` keyed on the parameters' storage and version,
so an in-place edit (a fused-LoRA re-merge, ``copy_``) quantises again on the next forward.  ``keep_bf16=False``: the quantised
weights are held here (``sealed``) and the bf16 weights of the chosen linears are freed; the biases stay."""
import torch

from . import derived, lora, ops

LINEARS = ("attn1.qkv", "attn1.to_out", "attn2.to_q", "attn2.to_out")
# The default of ``quantize_attention(linears=None)``: the linears whose quantised form, the quantiser pass it needs included,
# was faster than the bf16 form at D = 2048 with its median outside the bf16 leg's spread (profiles/mx8_attention.md).
DEFAULT_LINEARS = ("attn1.qkv", "attn2.to_q", "attn2.to_out")
# linear name -> (attention, which of its two linears, the module paths below the block an adapter names it by)
PARTS = {"attn1.qkv": ("attn1", "proj", ("attn1.to_q", "attn1.to_k", "attn1.to_v")), "attn1.to_out": ("attn1", "out", ("attn1.to_out.0",)),
         "attn2.to_q": ("attn2", "proj", ("attn2.to_q",)), "attn2.to_out": ("attn2", "out", ("attn2.to_out.0",))}
LORA_SLOTS = {"attn1.qkv": "qkv", "attn1.to_out": "out", "attn2.to_q": "q", "attn2.to_out": "out"}


def resolve(linears):
    """``linears`` of ``quantize_attention`` -> the chosen names in the order of ``LINEARS``; raises on an unknown name."""
    if linears is None:
        return DEFAULT_LINEARS
    chosen = tuple(linears)
    unknown = [n for n in chosen if n not in LINEARS]
    if unknown:
        raise ValueError(f"ltxmi: quantize_attention(): unknown linear {unknown[0]!r}; the choices are {', '.join(LINEARS)}")
    return tuple(n for n in LINEARS if n in chosen)


class AttnState:
    __slots__ = ("proj", "out", "cache", "sealed")

    def __init__(self, proj, out):
        self.proj, self.out = proj, out
        self.cache, self.sealed = derived.DerivedCache(capacity=2, layout=False), None


def _modules(attn, which):
    if which == "out":
        return [attn.to_out[0]]
    return [attn.to_q] if attn.is_cross_attention else [attn.to_q, attn.to_k, attn.to_v]


def check(attn, which, name):
    """The shapes ``ltxmi_gemm_mx8`` takes (K % 128 == 0, N % 32 == 0) and CUDA bf16 weights, for linear ``name``."""
    for lin in _modules(attn, which):
        w = lin.weight
        if w.dim() != 2 or w.shape[1] % 128 or w.shape[0] % 32:
            raise ValueError(f"ltxmi: quantize_attention(): {name} is {tuple(w.shape)}; the MX-FP8 GEMM needs in_features % 128 == 0 "
                             "and out_features % 32 == 0")
        if w.dtype != torch.bfloat16 or not w.is_cuda:
            raise TypeError(f"ltxmi: quantize_attention(): {name}.weight must be a CUDA bfloat16 tensor, got {w.dtype} on {w.device}")


def weights(attn, which):
    """(wq, w_scales, bias) of a quantised linear of ``attn``; the packed projection is quantised member by member into one
    [3D, K] operand, so no bf16 pack is built for it."""
    st = attn.__dict__["_mx8"]
    if st.sealed is not None:
        return st.sealed[which]
    mods = _modules(attn, which)

    def build():
        with torch.no_grad():
            ws = [m.weight for m in mods]
            if len(ws) == 1:
                return (*ops.quantize_mx8(ws[0]), mods[0].bias)
            n, K = sum(w.shape[0] for w in ws), ws[0].shape[1]
            q = torch.empty((n, K), dtype=ops.E4M3, device=ws[0].device)
            s = torch.empty((n, K // 32), dtype=torch.uint8, device=ws[0].device)
            r = 0
            for w in ws:
                ops.quantize_mx8(w, out=(q[r:r + w.shape[0]], s[r:r + w.shape[0]]))
                r += w.shape[0]
            bias = torch.cat([m.bias for m in mods]) if mods[0].bias is not None else None
            return q, s, bias
    return st.cache.get([m.weight for m in mods] + [m.bias for m in mods], (which,), build)


def seal(attn):
    """keep_bf16=False: hold the quantised weights (and the packed bias) here and free the bf16 weights of the chosen linears."""
    st = attn.__dict__["_mx8"]
    held = {which: weights(attn, which) for which in ("proj", "out") if getattr(st, which)}
    st.sealed = held
    st.cache.clear()
    for which in held:
        for lin in _modules(attn, which):
            lin.weight.data = torch.empty(0, dtype=lin.weight.dtype, device=lin.weight.device)
    attn.invalidate_packed()                     # the bf16 [to_q; to_k; to_v] pack of a freed projection goes with it


def project(attn, x, rowsumsq=None, rowsumsq_cols=0):
    """The quantised q / qkv projection: ``x`` bf16 rows (quantised here) or the (e4m3, scales) pair of
    ``ops.norm_modulate_mx8`` -> bf16 [rows, N], with q's row sums of squares where asked for."""
    wq, ws, bias = weights(attn, "proj")
    xq = x if isinstance(x, tuple) else ops.quantize_mx8(x)
    return ops.gemm_mx8(*xq, wq, ws, bias=bias, rowsumsq=rowsumsq, rowsumsq_cols=rowsumsq_cols,
                        **lora.pair_mx8(attn, "q" if attn.is_cross_attention else "qkv", xq))


def to_out(attn, a2, **kw):
    """quantise(attention output) -> to_out.0; the keywords are ``ops.gemm_mx8``'s (the gate + residual epilogue, ``out``)."""
    wq, ws, bias = weights(attn, "out")
    xq = ops.quantize_mx8(a2)
    return ops.gemm_mx8(*xq, wq, ws, bias=bias, **lora.pair_mx8(attn, "out", xq), **kw)
