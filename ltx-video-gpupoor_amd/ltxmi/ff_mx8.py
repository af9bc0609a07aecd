"""The feed-forward pair of a DiT block in MX-FP8 (ops.quantize_mx8 / ops.gemm_mx8): the per-block state that
``Transformer3DModel.quantize_ff`` sets, and the three launches the block runs when it is set.

A quantised ``FeedForward`` carries ``__dict__["_mx8"]``, an ``FFState``; without it the block's calls are the ones they were
(``BasicTransformerBlock`` tests that one attribute).  ``keep_bf16=True``: the bf16 parameters stay, and the quantised weights
live in a ``derived.DerivedCache`` keyed on the parameters' storage and version, so an in-place edit (a LoRA merge, ``copy_``)
quantises again on the next forward and ``.to()`` is followed.  ``keep_bf16=False``: the quantised weights are held here
(``sealed``) and the bf16 weights are freed; the biases stay."""
import torch

from . import derived, lora, ops


class FFState:
    __slots__ = ("cache", "sealed")

    def __init__(self):
        self.cache, self.sealed = derived.DerivedCache(capacity=1, layout=False), None


def check(ff, what="quantize_ff"):
    """The shapes ``ltxmi_gemm_mx8`` takes: both K (D and the inner width) multiples of 128, both N multiples of 32."""
    w1, w2 = ff.net[0].proj.weight, ff.net[2].weight
    for w, name in ((w1, "ff.net.0.proj"), (w2, "ff.net.2")):
        if w.dim() != 2 or w.shape[1] % 128 or w.shape[0] % 32:
            raise ValueError(f"ltxmi: {what}: {name} is {tuple(w.shape)}; the MX-FP8 GEMM needs in_features % 128 == 0 and "
                             "out_features % 32 == 0")
        if w.dtype != torch.bfloat16 or not w.is_cuda:
            raise TypeError(f"ltxmi: {what}: {name}.weight must be a CUDA bfloat16 tensor, got {w.dtype} on {w.device}")


def weights(ff):
    """((w1q, w1_scales), (w2q, w2_scales)) of a quantised feed-forward."""
    st = ff.__dict__["_mx8"]
    if st.sealed is not None:
        return st.sealed
    w1, w2 = ff.net[0].proj.weight, ff.net[2].weight

    def build():
        with torch.no_grad():
            return ops.quantize_mx8(w1), ops.quantize_mx8(w2)
    return st.cache.get([w1, w2], (), build)


def ff1(ff, norm_h2):
    """quantise(norm_h) -> FF1 with GELU, written as MX-FP8: (q, scales) of [rows, inner]; never bf16."""
    (w1q, w1s), _ = weights(ff)
    xq = ops.quantize_mx8(norm_h2)
    return ops.gemm_mx8(*xq, w1q, w1s, bias=ff.net[0].proj.bias, epilogue=ops.EPI_GELU_TANH, mx_out=True,
                        **lora.pair_mx8(ff, "ff1", xq))


def ff2(ff, h, **kw):
    _, (w2q, w2s) = weights(ff)
    return ops.gemm_mx8(*h, w2q, w2s, bias=ff.net[2].bias, **lora.pair_mx8(ff, "ff2", h), **kw)
