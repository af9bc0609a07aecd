"""fp64 CPU double of ``ops.attention(return_lse=True)`` and ``ops.attention_merge`` -- TEST INFRASTRUCTURE ONLY.

Same argument meaning as the kernels (NHD tensors, lse [B, H, Lq] in natural-log units, a key at or below -1e30 removed, a
row with every key removed reports -inf and an undefined -- here NaN -- output, a partial with lse = -inf skipped by
selection in the merge), computed in float64 so that the ring / hybrid layout code of ltxmi/distributed.py and the merge
algebra can be checked to round-off without a GPU."""
import torch

REMOVED = -1e30


def attention_lse(q, k, v, scale, key_bias=None):
    """q [B, Lq, H, dh], k / v [B, Lk, H, dh] -> (o [B, Lq, H, dh], lse [B, H, Lq]), float64."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    if key_bias is not None:
        kb = key_bias.double()
        s = s + kb[:, None, None, :]
        s = s.masked_fill((kb <= REMOVED)[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])                      # NaN rows where every key is removed: "undefined"
    o = torch.einsum("bhqk,bkhd->bqhd", p, v)
    return o, lse


def attention_merge(outs, lses):
    """The arithmetic of ltxmi_attention_merge_bf16 in float64: returns (o, lse)."""
    L = torch.stack([l.double() for l in lses])            # [n, B, H, Lq]
    m = L.max(dim=0).values
    w = torch.exp(L - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    w = torch.where(torch.isinf(L) & (L < 0), torch.zeros_like(w), w)
    sw = w.sum(0)
    o = torch.zeros_like(outs[0], dtype=torch.float64)
    for wi, oi in zip(w, outs):
        wi = wi.permute(0, 2, 1)[..., None]                # [B, Lq, H, 1]
        o = o + torch.where(wi != 0, wi * oi.double(), torch.zeros_like(o))      # selection: a skipped partial may hold NaN
    o = o / sw.permute(0, 2, 1)[..., None]
    return o, m + torch.log(sw)
