"""LoRA adapters on the linears of the DiT blocks, applied UNMERGED at run time on top of unchanged base weights.

The reference's default 13B setup is a dev checkpoint plus a rank-128 "distilled" LoRA file (inference.py:99,408), handed to
``offload.load_loras_into_model(..., activate_all_loras=True)`` (inference.py:452-455,483-493; ltxv.py:160-161 keeps the file
apart from the model files): every linear the file names then computes ``base(x) + s * up(down(x))``, ``s = weight * alpha / r``.

Here the same formula is two GEMM launches per linear: ``T = bf16(x . down^T)`` on the existing kernel, then the linear's own
call with the second operand pair ``a2 = T, w2 = bf16(s * up)`` (``ops.gemm``, ltxmi_gemm_pair2_bf16), so the adapter arrives
inside the accumulator and every fused epilogue -- GELU, gate + residual, q's row sums of squares -- sees it.  Several adapters
on one linear are one pair: their down matrices stacked along r, their scaled up matrices side by side.  The packed projections
take packed adapters: ``down = [down_q; down_k; down_v]``, one ``T [M, 3R]``, ``up = [up_q; up_k; up_v]`` with member g reading
columns [g R, (g + 1) R) of T (``a2_group_cols = D``); a member without an adapter contributes zero blocks.

State per linear (``LoraSlot``) is rebuilt on attach / detach / weight change, cost O(adapter); with no adapter attached no
slot exists and every call the package makes is the one it makes without this module.

A linear that ``quantize_ff`` / ``quantize_attention`` run in MX-FP8 takes its adapters (``attach_lora(..., mx8=True)``) in MX-FP8
too: a ``LoraSlotMx8`` holds the same stacked operands quantised once, r padded to 128, and the call site's ``pair_mx8`` makes
``T = MX(xq . down_q^T)`` and hands the quantised ups to ``ops.gemm_mx8`` (ltxmi_gemm_mx8_pair2), which continues the linear's K
loop with them.  Which form a slot has follows the linear's state at ``rebuild``.

The other way to run an adapter, for strengths that stay fixed over a generation, is to FUSE it into the weights
(``Transformer3DModel.fuse_lora``; the second half of this file): one launch of the GEMM per linear, exact and reversible, after
which the model runs the kernels of a model without adapters."""
from collections import OrderedDict

import torch

from . import ops

BF16 = torch.bfloat16
RANK_PAD = 64          # include/ltxmi.h: K2 of ltxmi_gemm_pair is a multiple of 64
MX_RANK_PAD = 128      # include/ltxmi_mx_lora.h: K2 of ltxmi_gemm_mx8_pair is a multiple of 128 (a K-tile of the MX-FP8 GEMM)

# the ten linears of a BasicTransformerBlock, by their path below ``transformer_blocks.<i>.``
BLOCK_TARGETS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v",
                 "attn2.to_out.0", "ff.net.0.proj", "ff.net.2")
# linears an adapter file may name that carry no adapter here (attach_lora: strict=True raises, strict=False skips them)
OTHER_LINEARS = ("patchify_proj", "adaln_single.emb.timestep_embedder.linear_1", "adaln_single.emb.timestep_embedder.linear_2",
                 "adaln_single.linear", "caption_projection.linear_1", "caption_projection.linear_2", "proj_out")
# (owner module below the block, slot name, member linears below the owner): a slot with several members is a packed projection
SLOTS = (("attn1", "qkv", ("to_q", "to_k", "to_v")), ("attn1", "out", ("to_out.0",)),
         ("attn2", "q", ("to_q",)), ("attn2", "kv", ("to_k", "to_v")), ("attn2", "out", ("to_out.0",)),
         ("ff", "ff1", ("net.0.proj",)), ("ff", "ff2", ("net.2",)))


class LoraAdapter:
    """``modules``: {module path: (down [r, in], up [out, r], alpha or None)} as loaded (``loading.load_lora``)."""

    def __init__(self, modules):
        self.modules = dict(modules)

    def scale(self, path, weight):
        down, _, alpha = self.modules[path]
        return float(weight) * (float(alpha) / down.shape[0] if alpha is not None else 1.0)


class LoraSlot:
    """down [G R, K], up [N, R] (both bf16, R a multiple of 64) and the group width (0: one group) of one GEMM call."""
    __slots__ = ("down", "up", "group_cols")

    def __init__(self, down, up, group_cols):
        self.down, self.up, self.group_cols = down, up, group_cols


def pair(owner, slot, x2):
    """Keyword arguments of the second operand pair for ``ops.gemm`` at a call site: {} without an adapter on that linear
    (the call is then the one it always was), else ``T = ops.gemm(x2, down)`` -- rounded to bf16 once -- and the scaled ups."""
    slots = owner.__dict__.get("_lora")
    s = slots.get(slot) if slots else None
    if s is None:
        return {}
    return dict(a2=ops.gemm(x2, s.down), w2=s.up, a2_group_cols=s.group_cols)


class LoraSlotMx8:
    """The slot of a linear that runs in MX-FP8 (``attach_lora(mx8=True)``): down [G R, K] and up [N, R] quantised once, each as
    (e4m3, scales) with R a multiple of 128, and the group width (0: one group) of one ``ops.gemm_mx8`` call."""
    __slots__ = ("down", "up", "group_cols")

    def __init__(self, down, up, group_cols):
        self.down, self.up, self.group_cols = down, up, group_cols


def pair_mx8(owner, slot, xq):
    """``pair`` for a call site of ``ops.gemm_mx8``, whose input ``xq`` is an (e4m3, scales) pair: {} without an adapter on that
    linear, else ``T = MX(xq . down_q^T)`` -- quantised straight from the fp32 accumulator -- and the quantised scaled ups
    (include/ltxmi_mx_lora.h)."""
    slots = owner.__dict__.get("_lora")
    s = slots.get(slot) if slots else None
    if s is None:
        return {}
    return dict(a2=ops.gemm_mx8(*xq, *s.down, mx_out=True), w2=s.up, a2_group_cols=s.group_cols)


def runs_mx8(owner, slot):
    """Whether the linear(s) of ``slot`` run in MX-FP8 (ltxmi/ff_mx8.py, ltxmi/attn_mx8.py): their adapters are then MX-FP8 pairs."""
    st = owner.__dict__.get("_mx8")
    if st is None or slot == "kv":
        return False
    if slot in ("ff1", "ff2"):
        return True
    return bool(st.out if slot == "out" else st.proj)


def _held(owner, slot):
    """The quantised weight a ``keep_bf16=False`` model holds for ``slot``, or None."""
    st = owner.__dict__.get("_mx8")
    if st is None or st.sealed is None or not runs_mx8(owner, slot):
        return None
    if slot in ("ff1", "ff2"):
        return st.sealed[0 if slot == "ff1" else 1][0]
    return st.sealed["out" if slot == "out" else "proj"][0]


def member_shapes(owner, slot, members):
    """[(out_features, in_features)] of the member linears of a slot; where ``quantize_*(keep_bf16=False)`` freed the bf16
    weights, from the held quantised operand (the members of a packed projection are equal parts of it)."""
    held = _held(owner, slot)
    if held is None:
        return [tuple(_get(owner, m).weight.shape) for m in members]
    return [(held.shape[0] // len(members), held.shape[1])] * len(members)


def has_slot(owner, slot):
    slots = owner.__dict__.get("_lora")
    return bool(slots) and slot in slots


def epoch(owner):
    """Bumped on every attach / detach / weight change: part of the key of every cache that holds an adapted projection."""
    return owner.__dict__.get("_lora_epoch", 0)


def refuse(model_or_attn, what):
    """The sequence-parallel paths carry no adapters: raise, in the style of ``refuse_fp32_stream``."""
    if model_or_attn.__dict__.get("_lora") or model_or_attn.__dict__.get("_lora_adapters"):
        raise NotImplementedError(f"ltxmi: {what} does not run LoRA adapters; detach_lora() first or use AttnProcessor2_0")


def _get(module, path):
    for p in path.split("."):
        module = module[int(p)] if p.isdigit() else getattr(module, p)
    return module


def _member_state(linear, entries):
    """(down_cat [R, K], up_cat [N, R]) of one linear for ``entries`` = [(down, up, s), ...]; R not yet padded."""
    w = linear.weight
    downs = [d.to(device=w.device, dtype=BF16) for d, _, _ in entries]
    ups = [(u.to(device=w.device, dtype=torch.float32) * s).to(BF16) for _, u, s in entries]
    return torch.cat(downs, 0), torch.cat(ups, 1)


def _pad_to(t, rows=None, cols=None):
    r, c = t.shape
    out = torch.zeros((rows or r, cols or c), dtype=t.dtype, device=t.device)
    out[:r, :c] = t
    return out


def split_targets(adapter, num_blocks):
    """(block entries {(block, target): path}, other linears named) of an adapter; raises on a path that names no module."""
    mine, other = {}, []
    for path in adapter.modules:
        if path in OTHER_LINEARS:
            other.append(path)
            continue
        parts = path.split(".", 2)
        if len(parts) == 3 and parts[0] == "transformer_blocks" and parts[1].isdigit() and parts[2] in BLOCK_TARGETS \
                and int(parts[1]) < num_blocks:
            mine[(int(parts[1]), parts[2])] = path
        else:
            raise KeyError(f"ltxmi.lora: '{path}' names no linear of this model")
    return mine, sorted(other)


def check_shapes(model, adapter, mine):
    for (i, target), path in mine.items():
        block = model.transformer_blocks[i]
        owner = getattr(block, target.split(".")[0], None)
        if owner is None:
            raise KeyError(f"ltxmi.lora: '{path}' names no linear of this model")
        _get(block, target)
        owner_name, slot, members = next(s for s in SLOTS if target in [f"{s[0]}.{m}" for m in s[2]])
        shape = member_shapes(owner, slot, members)[[f"{owner_name}.{m}" for m in members].index(target)]
        down, up, _ = adapter.modules[path]
        if down.shape[1] != shape[1] or up.shape[0] != shape[0]:
            raise ValueError(f"ltxmi.lora: '{path}' is [{up.shape[0]}, r] x [r, {down.shape[1]}] but the linear is "
                             f"{tuple(shape)}")


def rebuild(model):
    """Per-linear state of every block from ``model._lora_adapters`` ({name: [adapter, weight, block entries]}); bumps the epoch."""
    active = model.__dict__.get("_lora_adapters") or OrderedDict()
    ep = model.__dict__.get("_lora_epoch", 0) + 1
    model.__dict__["_lora_epoch"] = ep
    with torch.no_grad():
        for i, block in enumerate(model.transformer_blocks):
            owners = {}
            for owner_name, slot, members in SLOTS:
                owner = getattr(block, owner_name, None)
                if owner is None:
                    continue
                slots = owners.setdefault(owner_name, (owner, {}))[1]
                states = []
                for m in members:
                    target = f"{owner_name}.{m}"
                    entries = []
                    for adapter, weight, mine in active.values():
                        path = mine.get((i, target))
                        if path is not None:
                            down, up, _ = adapter.modules[path]
                            entries.append((down, up, adapter.scale(path, weight)))
                    states.append(_member_state(_get(owner, m), entries) if entries else None)
                if all(s is None for s in states):
                    continue
                mx = runs_mx8(owner, slot)
                pad, group_mult = (MX_RANK_PAD, 256) if mx else (RANK_PAD, 128)
                R = max(s[0].shape[0] for s in states if s is not None)
                R = (R + pad - 1) // pad * pad
                lins = [_get(owner, m) for m in members]
                shapes = member_shapes(owner, slot, members)
                if len(members) > 1 and any(n % group_mult for n, _ in shapes):
                    raise NotImplementedError("ltxmi.lora: a packed projection takes an adapter only with an inner dimension "
                                              f"that is a multiple of {group_mult}")
                downs, ups = [], []
                for lin, (n, k), s in zip(lins, shapes, states):
                    if s is None:
                        downs.append(torch.zeros((R, k), dtype=BF16, device=lin.weight.device))
                        ups.append(torch.zeros((n, R), dtype=BF16, device=lin.weight.device))
                    else:
                        downs.append(_pad_to(s[0], rows=R))
                        ups.append(_pad_to(s[1], cols=R))
                down, up = torch.cat(downs, 0).contiguous(), torch.cat(ups, 0).contiguous()
                group_cols = shapes[0][0] if len(members) > 1 else 0
                if mx:          # the stacked, padded operands quantised as one; zero blocks become scale byte 0, elements 0
                    slots[slot] = LoraSlotMx8(ops.quantize_mx8(down), ops.quantize_mx8(up), group_cols)
                else:
                    slots[slot] = LoraSlot(down, up, group_cols)
            for owner, slots in owners.values():
                owner.__dict__["_lora"] = slots or None
                owner.__dict__["_lora_epoch"] = ep


# ---------------------------------------------------------------------------------------------------- adapters fused into the weights
# ``fuse_lora`` folds an adapter into the weight of every linear it names: W' = bf16(fp32(W + sum_r bf16(s up)[n, r] down[r, k])),
# ONE launch of the GEMM per linear with the base weight as the residual, one rounding for all fused adapters of the linear
# together.  A fused model carries no LoraSlot: every ``pair`` above returns {} and the forward is the one of a model without
# adapters.  The record (``FusedState``) lives in the model's ``__dict__`` under ``_lora_fused``; ``refuse``, ``rebuild``,
# ``epoch`` and ``_lora_adapters`` neither see it nor change.  Staleness: derived.py keys the packs and the text K/V caches on
# address + version counter, and the GEMM writes through a raw pointer, so ``_touch`` moves the counter after every merge.

class FusedState:
    """adapters: {name: [adapter, weight, [paths]]} in insertion order; base: {path: bf16 copy of the weight before any merge}
    for the linears with a fused adapter (and only those); sealed: paths of the linears merged with ``keep_base=False``, whose
    base is gone."""
    __slots__ = ("adapters", "base", "sealed")

    def __init__(self):
        self.adapters, self.base, self.sealed = OrderedDict(), {}, set()


class _Weight:                         # what ``_member_state`` reads of a linear
    __slots__ = ("weight",)

    def __init__(self, weight):
        self.weight = weight


def fused_state(model, create=False):
    st = model.__dict__.get("_lora_fused")
    if st is None and create:
        st = model.__dict__["_lora_fused"] = FusedState()
    return st


def merged_weight(base, entries, out=None, what="the linear"):
    """bf16(fp32(base + sum over ``entries`` = [(down [r, K], up [N, r], s)] of bf16(s up) @ down)) for a bf16 ``base`` [N, K]:
    the fp32 sum includes the base and is rounded once.  The operands are ``_member_state``'s, so a fused and an unmerged
    adapter see the same bf16 values; r is padded with exact zeros to what the GEMM's entry check takes (and K, where it is no
    multiple of 8, in a widened copy).  ``out`` may be ``base`` itself (the residual epilogue reads an element before it writes
    it).  A leading dimension or an address the GEMM refuses raises, naming ``what``."""
    if base.dim() != 2 or base.dtype != BF16 or base.stride(1) != 1:
        raise TypeError(f"ltxmi.lora: '{what}': a merge needs a 2-D bfloat16 weight, got {base.dtype} {tuple(base.shape)}")
    n_out, k_in = base.shape
    for down, up, _ in entries:
        if down.dim() != 2 or up.dim() != 2 or down.shape[1] != k_in or up.shape[0] != n_out or up.shape[1] != down.shape[0]:
            raise ValueError(f"ltxmi.lora: '{what}' is [{up.shape[0]}, r] x [r, {down.shape[1]}] but the linear is {(n_out, k_in)}")
    if out is None:
        out = torch.empty((n_out, k_in), dtype=BF16, device=base.device)
    elif out.shape != base.shape or out.dtype != BF16 or out.device != base.device:
        raise ValueError(f"ltxmi.lora: '{what}': out must be a bfloat16 {(n_out, k_in)} tensor on {base.device}")
    with torch.no_grad():
        down_cat, up_cat = _member_state(_Weight(base), entries)
        if k_in % 8:
            # the GEMM's N is a multiple of 8: merge a copy widened by zero columns, keep the first K (exact zeros change no bit)
            k8 = (k_in + 7) // 8 * 8
            wide = merged_weight(_pad_to(base, cols=k8), [(_pad_to(down_cat, cols=k8), up_cat, 1.0)], what=what)
            out.copy_(wide[:, :k_in])
            return out
        R = (down_cat.shape[0] + RANK_PAD - 1) // RANK_PAD * RANK_PAD
        while True:
            a = _pad_to(up_cat, cols=R)                                   # [N, R]
            w = _pad_to(down_cat, rows=R).t().contiguous()                # [K, R]
            kernel = ops.gemm_kernel_id(a, w, None, out, ops.EPI_GATE_RESIDUAL, base)
            if kernel >= 0 or R >= 2 * RANK_PAD:
                break
            R += RANK_PAD                                                 # a shape refused for a small K: zeros change no bit
        if kernel < 0:
            raise ValueError(f"ltxmi.lora: '{what}' {(n_out, k_in)} (leading dimensions {base.stride(0)}, {out.stride(0)}) cannot "
                             f"be merged: the GEMM refuses it ({kernel}): {ops.lib.ltxmi_last_error().decode()}")
        # no gate table: the kernel's EPI_RESIDUAL, acc + bias + residual in fp32 and one pack_bf16
        ops.gemm(a, w, None, out=out, epilogue=ops.EPI_GATE_RESIDUAL, residual=base)
    return out


def _touch(model, path, weight):
    """The merge wrote ``weight`` through a raw pointer: move its version counter (an in-place op on an empty view of it -- no
    element is written, the parameter and its storage stay).  An inference tensor has no counter: drop what was derived."""
    from .derived import tensor_version
    if tensor_version(weight) >= 0:
        with torch.no_grad():
            weight.narrow(0, 0, 0).zero_()
    else:
        owner = model
        model.invalidate_packed()
        for p in path.split(".")[:-1]:
            owner = owner[int(p)] if p.isdigit() else getattr(owner, p)
            if hasattr(owner, "invalidate_packed"):
                owner.invalidate_packed()
            if "_mx8" in owner.__dict__:                 # a quantised feed-forward (ltxmi/ff_mx8.py): quantise again
                owner.__dict__["_mx8"].cache.clear()


def fuse_paths(model, adapter):
    """The module paths of ``adapter``, all 17 kinds; raises as ``attach_lora`` does on a path that names no linear of this
    model and on a shape that does not fit."""
    mine, other = split_targets(adapter, len(model.transformer_blocks))
    check_shapes(model, adapter, mine)
    for path in other:
        try:
            lin = _get(model, path)
        except AttributeError:
            lin = None
        if lin is None:
            raise KeyError(f"ltxmi.lora: '{path}' names no linear of this model")
        down, up, _ = adapter.modules[path]
        if down.shape[1] != lin.weight.shape[1] or up.shape[0] != lin.weight.shape[0]:
            raise ValueError(f"ltxmi.lora: '{path}' is [{up.shape[0]}, r] x [r, {down.shape[1]}] but the linear is "
                             f"{tuple(lin.weight.shape)}")
    return list(mine.values()) + other


def check_mergeable(model, paths):
    """Raise, naming the linear, where ``merged_weight`` would: asked of the GEMM's entry check for every weight of ``paths``
    before the first one is written (no launch; the operands stand in by shape, the weight by its own address and stride)."""
    stand_in = {}
    for path in paths:
        w = _get(model, path).weight
        if w.dim() != 2 or w.dtype != BF16 or w.stride(1) != 1:
            raise TypeError(f"ltxmi.lora: '{path}': a merge needs a 2-D bfloat16 weight, got {w.dtype} {tuple(w.shape)}")
        n_out, k_in = w.shape
        a = stand_in.setdefault(n_out, torch.empty((n_out, 2 * RANK_PAD), dtype=BF16))
        b = stand_in.setdefault(k_in, torch.empty((k_in, 2 * RANK_PAD), dtype=BF16))
        # (a K that is no multiple of 8 is merged in a widened copy, ``merged_weight``)
        c = w.detach() if k_in % 8 == 0 else torch.empty((n_out, (k_in + 7) // 8 * 8), dtype=BF16)
        if k_in % 8:
            b = torch.empty((c.shape[1], 2 * RANK_PAD), dtype=BF16)
        kernel = ops.gemm_kernel_id(a, b, None, c, ops.EPI_GATE_RESIDUAL, c)
        if kernel < 0:
            raise ValueError(f"ltxmi.lora: '{path}' {(n_out, k_in)} (leading dimension {w.stride(0)}) cannot be merged: the GEMM "
                             f"refuses it ({kernel}): {ops.lib.ltxmi_last_error().decode()}")


def fused_entries(st, path):
    """[(down, up, s)] of every fused adapter that names ``path``, in insertion order."""
    out = []
    for adapter, weight, paths in st.adapters.values():
        if path in adapter.modules and path in paths:
            down, up, _ = adapter.modules[path]
            out.append((down, up, adapter.scale(path, weight)))
    return out


def remerge(model, paths, keep_base=True):
    """Each linear of ``paths`` from its base copy with all fused adapters that name it, in one rounding; a linear no fused
    adapter names any more gets its base bits back and its copy is freed.  ``keep_base=False``: the copy is dropped after the
    merge (in place where none existed) and the linear is sealed."""
    st = fused_state(model)
    with torch.no_grad():
        for path in paths:
            weight = _get(model, path).weight
            entries = fused_entries(st, path)
            base = st.base.get(path)
            if not entries:
                if base is not None:
                    weight.copy_(base)
                    del st.base[path]
                continue
            if base is None:
                if keep_base:
                    base = st.base[path] = weight.detach().clone()
                else:
                    base = weight.detach()
            merged_weight(base, entries, out=weight.detach(), what=path)
            _touch(model, path, weight)
            if not keep_base:
                st.base.pop(path, None)
                st.sealed.add(path)
