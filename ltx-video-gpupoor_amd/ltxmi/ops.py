"""Tensor-level wrappers over the C ABI (one function per entry point of include/ltxmi.h).

PyTorch is plumbing only here: it owns the device allocations and the stream; every
FLOP of the hot path runs in libltxmi.so.  All wrappers launch on
``torch.cuda.current_stream()`` and never synchronise.
"""
import ctypes
import math

import torch

from . import _lib, _lib_mx, _lib_mxa, _lib_mxl, _lib_mxt, derived
from ._lib import lib, check

BF16 = torch.bfloat16


def _header(*names):
    """The values of include/ltxmi.h's enum constants and defines LTXMI_<name>: no number of the header is restated here."""
    return tuple(_lib.CONSTANTS["LTXMI_" + n] for n in names)


EPI_NONE, EPI_GELU_TANH, EPI_SILU, EPI_GATE_RESIDUAL = _header("EPI_NONE", "EPI_GELU_TANH", "EPI_SILU", "EPI_GATE_RESIDUAL")
NORM_RMS, NORM_LAYER = _header("NORM_RMS", "NORM_LAYER")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- optional per-launch timing (bench.py): HIP events recorded on the launch stream around
# the launches whose key is being watched; nothing is recorded (or allocated) otherwise.
_watch = None
_events = {}


def watch_launches(keys):
    """keys: iterable of ("gemm", M, N, K, epilogue) / ("attention", B, H, Lq, Lk, dh) /
    ("conv3d", output positions, Cin, Cout, d2s[, "plain" | "add" | "post_norm" | "second_output"]) tuples, or None."""
    global _watch
    _watch = set(keys) if keys else None
    _events.clear()


_redo_counter = None


def count_attention_redos(counter):
    """Diagnostic: an int32 CUDA tensor of one element that EVERY attention launch from now on bumps once per (batch, head,
    query tile) item it had to redo in the exact form (``ops.attention(redo_counter=)``); None switches it off.  bench.py
    keeps it on through the timed steps: the count is part of the bench line."""
    global _redo_counter
    _redo_counter = counter


def launch_times_ms():
    """{key: [ms, ...]} for the watched launches (call after a stream/device synchronize)."""
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in _events.items()}


def _prof_begin(key, key2=None):
    if _watch is None:
        return None
    if key not in _watch:
        if key2 is None or key2 not in _watch:
            return None
        key = key2
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    return key, e0, e1


def _prof_end(tok):
    if tok is not None:
        tok[2].record()
        _events.setdefault(tok[0], []).append((tok[1], tok[2]))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _chk_bf16(*ts):
    for t in ts:
        if t is None:
            continue
        if t.dtype != BF16 or not t.is_cuda:
            raise TypeError(f"ltxmi: expected a CUDA bfloat16 tensor, got {t.dtype} on {t.device}")


def _rows(t):
    """View [..., K] with contiguous last dim as (rows, ld)."""
    if t.stride(-1) != 1:
        raise ValueError("ltxmi: innermost dimension must be contiguous")
    t2 = t.reshape(-1, t.shape[-1]) if t.is_contiguous() else t
    if t2.dim() != 2:
        raise ValueError("ltxmi: expected a 2-D tensor or a contiguous N-D tensor")
    return t2, t2.shape[0], t2.stride(0)


# alias kept for tools: the cache keys of packed weights and derived tensors live in ltxmi/derived.py, whose docstring says
# what they cannot see and when to call ``invalidate_packed()`` (``Attention``, ``CausalConv3d``, the upsampler's
# ``_ConvParams``, the T5 attention / feed-forward modules, ``T5EncoderModel``, ``Transformer3DModel``)
tensor_version = derived.tensor_version


def _chk_bf16_any_device(*ts):
    for t in ts:
        if t is not None and t.dtype != BF16:
            raise TypeError(f"ltxmi: expected a bfloat16 tensor, got {t.dtype}")


def _gemm_args(a, w, bias, out, epilogue, residual, gate_table, gate_temb, rows_per_group, algo, rowsumsq, rowsumsq_cols,
               a_kblock, a_kblock_stride, allocate_out):
    """The ltxmi_gemm_args of a ``gemm`` / ``gemm_kernel_id`` call -> (args, out, M, N, K).  ``out is None``: allocated
    (allocate_out), or stood in for by what a fresh allocation always is -- contiguous and 16-byte aligned."""
    a2, M, lda = _rows(a)
    N, K = w.shape
    if a_kblock:
        # ``a`` is block 0 of a K-blocked operand: [M, a_kblock] rows; block j lies j * a_kblock_stride elements further
        if a2.shape[1] != a_kblock or K % a_kblock:
            raise ValueError(f"ltxmi.gemm: K-blocked a must be [M, {a_kblock}] with K={K} a multiple of the block")
    elif a2.shape[1] != K:
        raise ValueError(f"ltxmi.gemm: a is [{M},{a2.shape[1]}] but w is [{N},{K}]")
    args = _lib.GemmArgs()
    if out is None and not allocate_out:
        args.C, args.ldc = 256, N
    else:
        if out is None:
            out = torch.empty((M, N), dtype=BF16, device=a.device)
        o2, Mo, ldc = _rows(out)
        if Mo != M or o2.shape[1] != N:
            raise ValueError("ltxmi.gemm: bad out shape")
        args.C, args.ldc = o2.data_ptr(), ldc
    args.A, args.lda = a2.data_ptr(), lda
    args.W, args.ldw = w.data_ptr(), w.stride(0)
    args.bias = bias.data_ptr() if bias is not None else None
    args.M, args.N, args.K = M, N, K
    args.epilogue = epilogue
    if residual is not None:
        r2, Mr, ldr = _rows(residual)
        args.residual, args.ldr = r2.data_ptr(), ldr
    if gate_table is not None:
        args.gate_table = gate_table.data_ptr()
        args.gate_temb = gate_temb.data_ptr()
        args.gate_ld = gate_temb.stride(0) if gate_temb.dim() == 2 else 0
    args.rows_per_group = rows_per_group
    args.algo = algo               # 0 = kernel chosen by shape; 128 / 256: diagnostics (include/ltxmi.h)
    args.a_kblock, args.a_kblock_stride = a_kblock, a_kblock_stride
    if rowsumsq is not None:
        # fp32 [M, rowsumsq_cols/64]: per-64-column sums of squares of the bf16 outputs, columns < rowsumsq_cols
        if rowsumsq.dtype != torch.float32 or rowsumsq.dim() != 2 or rowsumsq.shape[0] != M or rowsumsq.stride(1) != 1 \
                or rowsumsq.shape[1] * 64 < rowsumsq_cols:
            raise ValueError("ltxmi.gemm: rowsumsq must be fp32 [M, >= rowsumsq_cols/64]")
        args.rowsumsq, args.rowsumsq_cols, args.rowsumsq_ld = rowsumsq.data_ptr(), rowsumsq_cols, rowsumsq.stride(0)
    return args, out, M, N, K


def _gemm_pair(M, N, a2, w2, a2_group_cols):
    """The ltxmi_gemm_pair of a second operand pair: a2 [M, groups * K2] (a row-strided view is fine), w2 [N, K2]."""
    if w2 is None:
        raise ValueError("ltxmi.gemm: a2 given without w2")
    t2, M2, lda2 = _rows(a2)
    if w2.dim() != 2 or w2.stride(1) != 1:
        raise ValueError("ltxmi.gemm: w2 must be 2-D with a contiguous innermost dimension")
    K2 = w2.shape[1]
    groups = N // a2_group_cols if a2_group_cols > 0 else 1
    if M2 != M or w2.shape[0] != N or t2.shape[1] != groups * K2:
        raise ValueError(f"ltxmi.gemm: a2 is [{M2},{t2.shape[1]}], w2 is [{w2.shape[0]},{K2}]: expected [{M},{groups}*K2], [{N},K2]")
    pair = _lib.GemmPair()
    pair.A2, pair.lda2 = t2.data_ptr(), lda2
    pair.W2, pair.ldw2 = w2.data_ptr(), w2.stride(0)
    pair.K2, pair.group_cols = K2, a2_group_cols
    return pair


def gemm(a, w, bias=None, out=None, epilogue=EPI_NONE, residual=None, gate_table=None, gate_temb=None,
         rows_per_group=1, algo=0, rowsumsq=None, rowsumsq_cols=0, a_kblock=0, a_kblock_stride=0,
         a2=None, w2=None, a2_group_cols=0):
    """out[M,N] = epi(a[M,K] @ w[N,K]^T + bias).  ``a``/``out``/``residual`` may be row-strided 2-D views.
    gate_temb: 2-D view [groups, N] (row stride = gate_ld).
    ``a2`` [M, groups * K2], ``w2`` [N, K2]: a second operand pair that continues the K loop (an adapter applied unmerged,
    ltxmi_gemm_pair2_bf16): out = epi(a @ w^T + a2[:, g K2:(g + 1) K2] @ w2^T + bias) with g = n // a2_group_cols (0: one
    group).  Without ``a2`` the call is ltxmi_gemm_bf16's."""
    _chk_bf16(a, w, bias, out, residual, gate_table, gate_temb, a2, w2)
    if a2 is None and w2 is not None:
        raise ValueError("ltxmi.gemm: w2 given without a2")
    if a2 is not None:
        # checked before anything is allocated or launched: a refused call leaves ``out`` as it was
        M, N = _rows(a)[1], w.shape[0]
        pair = _gemm_pair(M, N, a2, w2, a2_group_cols)
    args, out, M, N, K = _gemm_args(a, w, bias, out, epilogue, residual, gate_table, gate_temb, rows_per_group, algo,
                                    rowsumsq, rowsumsq_cols, a_kblock, a_kblock_stride, True)
    if a2 is None:
        tok = _prof_begin(("gemm", M, N, K, epilogue))
        check(lib.ltxmi_gemm_bf16(ctypes.byref(args), _stream()), "ltxmi_gemm_bf16")
    else:
        tok = _prof_begin(("gemm_pair2", M, N, K, epilogue))
        check(lib.ltxmi_gemm_pair2_bf16(ctypes.byref(args), ctypes.byref(pair), _stream()), "ltxmi_gemm_pair2_bf16")
    _prof_end(tok)
    return out


# ltxmi_gemm_kernel: what ltxmi_gemm_kernel_id and ltxmi_gemm_pair2_kernel_id answer
GEMM_TILE128, GEMM_TILE256, GEMM_PERSISTENT256 = _header("GEMM_TILE128", "GEMM_TILE256", "GEMM_PERSISTENT256")
GEMM_PAIR2_TILE128, GEMM_PAIR2_TILE256 = _header("GEMM_PAIR2_TILE128", "GEMM_PAIR2_TILE256")


def gemm_kernel_id(a, w, bias=None, out=None, epilogue=EPI_NONE, residual=None, gate_table=None, gate_temb=None,
                   rows_per_group=1, algo=0, rowsumsq=None, rowsumsq_cols=0, a_kblock=0, a_kblock_stride=0,
                   a2=None, w2=None, a2_group_cols=0):
    """Which kernel ``gemm`` runs for the same arguments (0 the 128x128 tile kernel, 1 the non-persistent 256x256 one,
    2 the persistent 256x256 one; with a second pair 3 the 128x128 two-pair kernel, 4 the 256x256 one), or the negative
    status ``gemm`` would raise on.  Built from the same struct as the
    launch and decided by the same code; nothing is launched or read, so the tensors may live on any device (only their
    shapes, strides and addresses count)."""
    _chk_bf16_any_device(a, w, bias, out, residual, gate_table, gate_temb, a2, w2)
    args = _gemm_args(a, w, bias, out, epilogue, residual, gate_table, gate_temb, rows_per_group, algo,
                      rowsumsq, rowsumsq_cols, a_kblock, a_kblock_stride, False)[0]
    if a2 is None:
        return int(lib.ltxmi_gemm_kernel_id(ctypes.byref(args)))
    pair = _gemm_pair(args.M, args.N, a2, w2, a2_group_cols)
    return int(lib.ltxmi_gemm_pair2_kernel_id(ctypes.byref(args), ctypes.byref(pair)))


def _chk_f32(t, what):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"ltxmi.{what}: expected a CUDA float32 tensor, got {t.dtype} on {t.device}")


def _norm_modulate(what, f32in, x, out, eps, kind, scale_table, scale_temb, shift_table, shift_temb, rows_per_group):
    """The one body of ``norm_modulate`` and ``norm_modulate_f32in``: x's dtype and the entry point are what differs."""
    if f32in:
        _chk_f32(x, what)
    _chk_bf16(None if f32in else x, out, scale_table, scale_temb, shift_table, shift_temb)
    x2, rows, ldx = _rows(x)
    o2, orows, ldy = _rows(out)
    D = x2.shape[1]
    if f32in and (orows != rows or o2.shape[1] != D):     # (the bf16 entry has never tested out's shape: left as it was)
        raise ValueError(f"ltxmi.{what}: out must have x's rows and channels")
    if scale_temb.stride(0) != shift_temb.stride(0):
        raise ValueError(f"ltxmi.{what}: scale/shift tables must share a row stride")
    entry = lib.ltxmi_norm_modulate_f32in_bf16 if f32in else lib.ltxmi_norm_modulate_bf16
    check(entry(_ptr(x2), ldx, _ptr(o2), ldy, rows, D, eps, kind, _ptr(scale_table), _ptr(scale_temb), _ptr(shift_table),
                _ptr(shift_temb), scale_temb.stride(0), rows_per_group, _stream()),
          "ltxmi_norm_modulate_f32in_bf16" if f32in else "ltxmi_norm_modulate_bf16")
    return out


def norm_modulate(x, out, eps, kind, scale_table, scale_temb, shift_table, shift_temb, rows_per_group):
    """out = norm(x) * (1 + scale_table + scale_temb[g]) + shift_table + shift_temb[g].
    scale_temb/shift_temb: 2-D views [groups, D] sharing one row stride."""
    return _norm_modulate("norm_modulate", False, x, out, eps, kind, scale_table, scale_temb, shift_table, shift_temb,
                          rows_per_group)


def norm_modulate_f32in(x, out, eps, kind, scale_table, scale_temb, shift_table, shift_temb, rows_per_group):
    """``norm_modulate`` for the fp32 residual stream (mixed precision): x fp32 rows, out bf16 rows, the statistics and the
    modulation in fp32 from the unrounded stream, one rounding at the store (include/ltxmi.h)."""
    return _norm_modulate("norm_modulate_f32in", True, x, out, eps, kind, scale_table, scale_temb, shift_table, shift_temb,
                          rows_per_group)


def gate_residual_f32_(h, y, gate_table=None, gate_temb=None, rows_per_group=1, round_product=0, h_bf16=None):
    """In place on the fp32 stream: h += (gate_table + gate_temb[group]) * y, y bf16 rows; gate_table None: h += y.
    gate_temb: 2-D view [groups, D].  round_product=1 rounds the product to bf16 before the add (the reference's in-place
    ``attn_output *= gate_msa``), 0 keeps it fp32 (its FF gate).  h_bf16 (bf16 rows): also receives bf16(h) of the result."""
    _chk_f32(h, "gate_residual_f32_")
    _chk_bf16(y, gate_table, gate_temb, h_bf16)
    h2, rows, ldh = _rows(h)
    y2, yrows, ldy = _rows(y)
    D = h2.shape[1]
    if yrows != rows or y2.shape[1] != D:
        raise ValueError("ltxmi.gate_residual_f32_: y must have h's rows and channels")
    if (gate_table is None) != (gate_temb is None):
        raise ValueError("ltxmi.gate_residual_f32_: gate_table and gate_temb go together")
    gate_ld = 0
    if gate_temb is not None:
        gate_ld = gate_temb.stride(0) if gate_temb.dim() == 2 else 0
    b2, ldb = None, 0
    if h_bf16 is not None:
        b2, brows, ldb = _rows(h_bf16)
        if brows != rows or b2.shape[1] != D:
            raise ValueError("ltxmi.gate_residual_f32_: h_bf16 must have h's rows and channels")
    check(lib.ltxmi_gate_residual_f32(_ptr(h2), ldh, _ptr(y2), ldy, rows, D, _ptr(gate_table), _ptr(gate_temb), gate_ld,
                                      rows_per_group, int(round_product), _ptr(b2), ldb, _stream()),
          "ltxmi_gate_residual_f32")
    return h


def rmsnorm_rope_(x, weight, eps, cos=None, sin=None, rope_period=0, rstd_of=None):
    """In place: x = rope(rmsnorm(x) * weight).  x: 2-D row-strided view [rows, D];
    cos/sin: [period, D] tables (row r uses row r % period) or None.
    rstd_of = (rowsumsq fp32 [rows, blocks], norm_dim, eps, out fp32 [rows]): riding on the launch, out[r] =
    rsqrt(sum(rowsumsq[r]) / norm_dim + eps) -- q's RMSNorm factor from the projection GEMM's partial sums."""
    _chk_bf16(x, weight, cos, sin)
    x2, rows, ldx = _rows(x)
    D = x2.shape[1]
    ld_tab = 0
    if cos is not None:
        if cos.dim() != 2 or cos.shape != sin.shape or cos.stride(0) != sin.stride(0):
            raise ValueError("ltxmi.rmsnorm_rope_: cos/sin must be matching 2-D tables")
        ld_tab = cos.stride(0)
        rope_period = rope_period or cos.shape[0]
    if rstd_of is not None:
        ss, norm_dim, norm_eps, out = rstd_of
        if ss.dtype != torch.float32 or out.dtype != torch.float32 or ss.dim() != 2 or ss.shape[0] != rows or \
                ss.stride(1) != 1 or out.shape != (rows,) or not out.is_contiguous():
            raise ValueError("ltxmi.rmsnorm_rope_: rstd_of needs fp32 sums [rows, blocks] and a contiguous fp32 out [rows]")
        check(lib.ltxmi_rmsnorm_rope_rstd_bf16(_ptr(x2), ldx, rows, D, _ptr(weight), eps, _ptr(cos), _ptr(sin), ld_tab,
                                               rope_period, _ptr(ss), ss.stride(0), ss.shape[1], norm_dim, norm_eps,
                                               _ptr(out), _stream()), "ltxmi_rmsnorm_rope_rstd_bf16")
        return x
    check(lib.ltxmi_rmsnorm_rope_bf16(_ptr(x2), ldx, rows, D, _ptr(weight), eps, _ptr(cos), _ptr(sin), ld_tab,
                                      rope_period, _stream()), "ltxmi_rmsnorm_rope_bf16")
    return x


def rowsumsq_rstd(ss, norm_dim, eps, out=None):
    """fp32 [rows, blocks] partial sums of squares -> fp32 [rows] RMSNorm factors rsqrt(sum / norm_dim + eps)."""
    if ss.dtype != torch.float32 or ss.dim() != 2 or ss.stride(1) != 1 or not ss.is_cuda:
        raise ValueError("ltxmi.rowsumsq_rstd: expected CUDA fp32 sums [rows, blocks]")
    rows = ss.shape[0]
    out = torch.empty((rows,), dtype=torch.float32, device=ss.device) if out is None else out
    check(lib.ltxmi_rowsumsq_rstd_f32(_ptr(ss), ss.stride(0), ss.shape[1], rows, norm_dim, eps, _ptr(out), _stream()),
          "ltxmi_rowsumsq_rstd_f32")
    return out


def attention_fuses_qnorm(B, H, Lq, Lk, dh, has_key_bias=False):
    """Whether ``attention(..., q_norm=...)`` is available for this shape (every shape ``attention`` accepts)."""
    return bool(lib.ltxmi_attention_fuses_qnorm(B, H, Lq, Lk, dh, int(has_key_bias)))


def attention_kernel_id(B, H, Lq, Lk, dh, has_key_bias=False, k_stride_l=None, v_stride_l=None):
    """Which kernel instance ``attention`` runs for a shape: equal ids = the same arithmetic per (batch, head, row).
    k_stride_l / v_stride_l: the token strides of k and v in elements (default: slices of the packed [.., 3 H dh]
    projection, what AttnProcessor2_0 passes)."""
    ks = 3 * H * dh if k_stride_l is None else k_stride_l
    vs = ks if v_stride_l is None else v_stride_l
    return int(lib.ltxmi_attention_kernel_id(B, H, Lq, Lk, dh, int(has_key_bias), ks, vs))


def _attn_shared(a, what, cuda_bias, dims, q, k, v, out, key_bias, softmax_scale):
    """The twenty leading fields that ltxmi_attn_args and ltxmi_attn_relbias_args have in common (the second is a prefix of
    the first by design), after ``_chk_attn_qkv``.  ``out`` has been tested by the caller: its shape is where the two
    contracts differ (``attention``'s out_segments), and so do the error texts."""
    B, H, Lq, Lk, dh = dims
    a.q, a.q_stride_b, a.q_stride_l = q.data_ptr(), q.stride(0), q.stride(1)
    a.k, a.k_stride_b, a.k_stride_l = k.data_ptr(), k.stride(0), k.stride(1)
    a.v, a.v_stride_b, a.v_stride_l = v.data_ptr(), v.stride(0), v.stride(1)
    a.o, a.o_stride_b, a.o_stride_l = out.data_ptr(), out.stride(0), out.stride(1)
    if key_bias is not None:
        if key_bias.dtype != torch.float32 or key_bias.shape != (B, Lk) or key_bias.stride(1) != 1 \
                or (cuda_bias and not key_bias.is_cuda):
            raise ValueError(f"ltxmi.{what}: key_bias must be {'a CUDA ' if cuda_bias else ''}fp32 [B, Lk]")
        a.key_bias, a.bias_stride_b = key_bias.data_ptr(), key_bias.stride(0)
    a.B, a.H, a.Lq, a.Lk, a.head_dim = B, H, Lq, Lk, dh
    a.softmax_scale = softmax_scale


def _chk_attn_qkv(what, q, k, v, out):
    """The tests ``attention`` and ``attention_relbias`` make before anything else -> (B, H, Lq, Lk, dh)."""
    _chk_bf16(q, k, v, out)
    B, Lq, H, dh = q.shape
    for t in (q, k, v):
        if t.stride(3) != 1 or t.stride(2) != dh:
            raise ValueError(f"ltxmi.{what}: (heads, head_dim) must be contiguous")
    return B, H, Lq, k.shape[1], dh


def attention(q, k, v, out=None, key_bias=None, softmax_scale=None, q_norm=None, rope=None, out_segments=None,
              redo_counter=None, force_exact=False, return_lse=False, lse=None):
    """q [B,Lq,H,dh], k/v [B,Lk,H,dh] (NHD; batch and token strides free, (H,dh) contiguous).
    key_bias: fp32 [B,Lk] additive (broadcast over heads and queries).  Any finite value and -inf are accepted; a value at
    or below -1e30 (-inf, ``torch.finfo(...).min``) means "key removed": its weight is exactly 0.  A batch row with every key
    removed is undefined, as in torch's SDPA.
    q_norm = (rowsumsq fp32 [B*Lq, H*dh/64] from ``gemm(..., rowsumsq=)`` OR the finalised factor fp32 [B*Lq] from
    ``rmsnorm_rope_(..., rstd_of=)``, weight bf16 [H*dh], eps): q is the raw projection output and is RMS-normalised over
    all heads (+ rotated with rope = (cos [period, H*dh], sin, period)) while the kernel loads it.
    out_segments = (tokens per segment, elements between segments): ``out`` is segment 0's [B, segment, H, dh] view of a
    buffer whose token axis is cut into such segments (the Ulysses return all-to-all's send buffer).
    redo_counter (diagnostic): int32 device tensor of one element, incremented once per (batch, head, query tile) item the
    pipelined kernels had to run again in the exact online-softmax form; force_exact: every item in that form.
    return_lse: return ``(out, lse)`` with lse fp32 [B, H, Lq] = ln sum_j exp(scale q.k_j + key_bias_j), the normaliser
    ``out`` was divided by (-inf for a row with every key removed) -- allocated here or written into ``lse=`` (which
    implies return_lse); ``attention_merge`` combines such pairs over disjoint key sets.  ``out`` and the kernel chosen do
    not depend on it."""
    B, H, Lq, Lk, dh = dims = _chk_attn_qkv("attention", q, k, v, out)
    if out is None:
        if out_segments is not None:
            raise ValueError("ltxmi.attention: out_segments needs an explicit out")
        out = torch.empty((B, Lq, H, dh), dtype=BF16, device=q.device)
    if out.dim() != 4 or out.stride(3) != 1 or out.stride(2) != dh:
        raise ValueError("ltxmi.attention: out must be 4-D with (heads, head_dim) contiguous")
    a = _lib.AttnArgs()
    if out_segments is not None:
        seg_len, seg_stride = out_segments
        if seg_len <= 0 or Lq % seg_len != 0 or tuple(out.shape) != (B, seg_len, H, dh):
            raise ValueError(f"ltxmi.attention: out_segments=({seg_len}, {seg_stride}) needs Lq={Lq} to be a multiple of the "
                             f"segment and out to be segment 0's [B, segment, H, dh] view, got {tuple(out.shape)}")
        a.o_segment_len, a.o_stride_segment = seg_len, seg_stride
    elif tuple(out.shape) != (B, Lq, H, dh):
        raise ValueError(f"ltxmi.attention: out must be [B, Lq, H, dh] = {(B, Lq, H, dh)}, got {tuple(out.shape)}")
    _attn_shared(a, "attention", False, dims, q, k, v, out, key_bias,
                 softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(dh))
    if q_norm is not None:
        ss, w, eps = q_norm
        nb = H * dh // 64
        _chk_bf16(w)
        if ss.dim() == 1:                                    # one finalised factor per row
            if ss.dtype != torch.float32 or ss.shape != (B * Lq,) or ss.stride(0) != 1 or not ss.is_cuda:
                raise ValueError("ltxmi.attention: q_norm row factors must be a contiguous fp32 [B*Lq]")
            a.q_rstd, a.q_rstd_stride_b, a.q_rstd_stride_l = ss.data_ptr(), Lq, 1
        else:
            if ss.dtype != torch.float32 or ss.dim() != 2 or ss.shape != (B * Lq, nb) or ss.stride(1) != 1:
                raise ValueError("ltxmi.attention: q_norm row sums must be fp32 [B*Lq, H*dh/64]")
            a.q_rowsumsq, a.q_rowsumsq_stride_b, a.q_rowsumsq_stride_l = ss.data_ptr(), Lq * ss.stride(0), ss.stride(0)
            a.q_rowsumsq_blocks = nb
        a.q_norm_weight, a.q_norm_eps = w.data_ptr(), eps
        if rope is not None:
            cos, sin, period = rope
            _chk_bf16(cos, sin)
            if period not in (Lq, B * Lq) or cos.stride(0) != sin.stride(0) or cos.stride(1) != 1:
                raise ValueError("ltxmi.attention: rope tables must be [Lq or B*Lq, H*dh] with one row stride")
            a.rope_cos, a.rope_sin = cos.data_ptr(), sin.data_ptr()
            a.rope_stride_l = cos.stride(0)
            a.rope_stride_b = 0 if period == Lq else Lq * cos.stride(0)
    elif rope is not None:
        raise ValueError("ltxmi.attention: rope needs q_norm")
    if redo_counter is None:
        redo_counter = _redo_counter
    if redo_counter is not None:
        if redo_counter.dtype != torch.int32 or redo_counter.numel() != 1 or not redo_counter.is_cuda:
            raise ValueError("ltxmi.attention: redo_counter must be a CUDA int32 tensor of one element")
        a.redo_counter = redo_counter.data_ptr()
    a.force_exact = int(bool(force_exact))
    if return_lse or lse is not None:
        if lse is None:
            lse = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
        _chk_lse(lse, B, H, Lq, "ltxmi.attention: lse")
        a.lse, a.lse_stride_b, a.lse_stride_h = lse.data_ptr(), lse.stride(0), lse.stride(1)
    tok = _prof_begin(("attention", B, H, Lq, Lk, dh))
    check(lib.ltxmi_attention_fwd_bf16(ctypes.byref(a), _stream()), "ltxmi_attention_fwd_bf16")
    _prof_end(tok)
    return (out, lse) if lse is not None else out


def _chk_lse(lse, B, H, Lq, what):
    if lse.dtype != torch.float32 or not lse.is_cuda or tuple(lse.shape) != (B, H, Lq) or lse.stride(2) != 1:
        raise ValueError(f"{what} must be a CUDA fp32 [B, H, Lq] = {(B, H, Lq)} tensor with contiguous tokens")


def attention_merge(outs, lses, out=None, return_lse=False, lse=None):
    """Merge 2 .. 8 partial attention results over disjoint key sets for the same queries in one launch
    (``ltxmi_attention_merge_bf16``): outs[i] bf16 [B, Lq, H, dh] and lses[i] fp32 [B, H, Lq] as ``attention(...,
    return_lse=True)`` returns them.  fp32: w_i = exp(lse_i - max lse), out = sum w_i outs[i] / sum w_i, rounded to bf16
    once; a partial with lse_i = -inf is skipped (its out may hold anything).  Returns out, or (out, merged lse) with
    return_lse / ``lse=``.  ``out`` may be one of the partials."""
    n = len(outs)
    if n != len(lses) or not 2 <= n <= _lib.ATTN_MERGE_MAX:
        raise ValueError(f"ltxmi.attention_merge: {n} outputs / {len(lses)} lse tensors, need 2 .. {_lib.ATTN_MERGE_MAX} of each")
    _chk_bf16(*outs, out)
    B, Lq, H, dh = outs[0].shape
    if out is None:
        out = torch.empty((B, Lq, H, dh), dtype=BF16, device=outs[0].device)
    a = _lib.AttnMergeArgs()
    a.n = n
    for i, (o, l) in enumerate(zip(outs, lses)):
        if tuple(o.shape) != (B, Lq, H, dh) or o.stride(3) != 1 or o.stride(2) != dh:
            raise ValueError("ltxmi.attention_merge: partial outputs must be [B, Lq, H, dh] with (heads, head_dim) contiguous")
        _chk_lse(l, B, H, Lq, f"ltxmi.attention_merge: lses[{i}]")
        a.o_part[i], a.o_part_stride_b[i], a.o_part_stride_l[i] = o.data_ptr(), o.stride(0), o.stride(1)
        a.lse_part[i], a.lse_part_stride_b[i], a.lse_part_stride_h[i] = l.data_ptr(), l.stride(0), l.stride(1)
    if tuple(out.shape) != (B, Lq, H, dh) or out.stride(3) != 1 or out.stride(2) != dh:
        raise ValueError("ltxmi.attention_merge: out must be [B, Lq, H, dh] with (heads, head_dim) contiguous")
    a.o, a.o_stride_b, a.o_stride_l = out.data_ptr(), out.stride(0), out.stride(1)
    if return_lse or lse is not None:
        if lse is None:
            lse = torch.empty((B, H, Lq), dtype=torch.float32, device=out.device)
        _chk_lse(lse, B, H, Lq, "ltxmi.attention_merge: lse")
        a.lse, a.lse_stride_b, a.lse_stride_h = lse.data_ptr(), lse.stride(0), lse.stride(1)
    a.B, a.H, a.Lq, a.head_dim = B, H, Lq, dh
    check(lib.ltxmi_attention_merge_bf16(ctypes.byref(a), _stream()), "ltxmi_attention_merge_bf16")
    return (out, lse) if lse is not None else out


def qkv_norm_rope_pack(qkv, B, Nl, D, P, q_weight, k_weight, eps, cos=None, sin=None, rope_period=0, out=None):
    """qkv [B*Nl, 3D] (row-strided) -> the Ulysses send buffer [P, Nl, B, 3, D/P]: q/k RMS-normalised over all D
    channels (+ weight) and rotated, v copied, each channel in its destination rank's chunk (include/ltxmi.h)."""
    _chk_bf16(qkv, q_weight, k_weight, cos, sin, out)
    x2, rows, ld = _rows(qkv)
    if rows != B * Nl or x2.shape[1] != 3 * D:
        raise ValueError("ltxmi.qkv_norm_rope_pack: qkv must be [B*Nl, 3D]")
    if out is None:
        out = torch.empty((P, Nl, B, 3, D // P), dtype=BF16, device=qkv.device)
    if not out.is_contiguous() or out.numel() != rows * 3 * D:
        raise ValueError("ltxmi.qkv_norm_rope_pack: out must be a contiguous [P, Nl, B, 3, D/P] buffer")
    ld_tab = cos.stride(0) if cos is not None else 0
    check(lib.ltxmi_qkv_norm_rope_pack_bf16(_ptr(x2), ld, B, Nl, D, P, _ptr(q_weight), _ptr(k_weight), eps, _ptr(cos),
                                            _ptr(sin), ld_tab, rope_period, _ptr(out), _stream()),
          "ltxmi_qkv_norm_rope_pack_bf16")
    return out


def stg_blend_grouped_(a, v, m_f32):
    """a [G, B, L, Dg] contiguous (the K-blocked layout: channel block g of every row), v [B, L, >= G*Dg] with channels
    contiguous: a[g] = a[g] * m + v[..., g*Dg:(g+1)*Dg] * (1 - m), one launch."""
    _chk_bf16(a, v)
    G, B, L, Dg = a.shape
    if not a.is_contiguous() or v.dim() != 3 or v.shape[0] != B or v.shape[1] != L or v.shape[2] < G * Dg or v.stride(2) != 1:
        raise ValueError("ltxmi.stg_blend_grouped_: a must be contiguous [G,B,L,Dg], v [B,L,>=G*Dg] with unit channel stride")
    check(lib.ltxmi_stg_blend_grouped_bf16(_ptr(a), _ptr(v), Dg, v.stride(0), v.stride(1), _ptr(m_f32), G, B, L, Dg, _stream()),
          "ltxmi_stg_blend_grouped_bf16")
    return a


def silu(x, out=None):
    _chk_bf16(x, out)
    if not x.is_contiguous() or (out is not None and (not out.is_contiguous() or out.shape != x.shape)):
        raise ValueError("ltxmi.silu: x / out must be contiguous and equally shaped")
    out = torch.empty_like(x) if out is None else out
    check(lib.ltxmi_silu_bf16(_ptr(x), _ptr(out), x.numel(), _stream()), "ltxmi_silu_bf16")
    return out


def add(a, b, out=None):
    _chk_bf16(a, b, out)
    if not a.is_contiguous() or not b.is_contiguous() or b.shape != a.shape or \
            (out is not None and (not out.is_contiguous() or out.shape != a.shape)):
        raise ValueError("ltxmi.add: a / b / out must be contiguous and equally shaped")
    out = torch.empty_like(a) if out is None else out
    check(lib.ltxmi_add_bf16(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()), "ltxmi_add_bf16")
    return out


def timestep_embedding(t_f32, dim=256):
    """t_f32: fp32 [n] (already multiplied by timestep_scale_multiplier) -> bf16 [n, dim]."""
    if t_f32.dtype != torch.float32 or not t_f32.is_cuda or not t_f32.is_contiguous():
        raise TypeError("ltxmi.timestep_embedding: expected a contiguous CUDA fp32 vector")
    out = torch.empty((t_f32.numel(), dim), dtype=BF16, device=t_f32.device)
    check(lib.ltxmi_timestep_embedding_bf16(_ptr(t_f32), _ptr(out), t_f32.numel(), dim, _stream()),
          "ltxmi_timestep_embedding_bf16")
    return out


def stg_blend_(a, v, m_f32):
    """a [B,L,D] (rows contiguous over (B,L)), v row-strided view with the same rows; a = a*m + v*(1-m)."""
    _chk_bf16(a, v)
    B, L, D = a.shape
    a2, _, lda = _rows(a)
    v2 = v.reshape(B * L, D) if v.is_contiguous() else v
    if v2.dim() == 3:
        if v2.stride(0) != L * v2.stride(1):
            raise ValueError("ltxmi.stg_blend_: v batch stride must equal L * row stride")
        ldv = v2.stride(1)
    else:
        ldv = v2.stride(0)
    check(lib.ltxmi_stg_blend_bf16(_ptr(a2), lda, _ptr(v2), ldv, _ptr(m_f32), B, L, D, _stream()),
          "ltxmi_stg_blend_bf16")
    return a


# Convolution implementation: 0 = chosen by shape (the product setting), 1 = implicit GEMM, 2 = direct convolution.
# The parity tests run a decode both ways to check the two implementations against each other.
CONV_ALGO = 0


# conv3d(post_norm=...): let the convolution apply the PixelNorm -> AdaLN -> SiLU in its epilogue where it can (False: always
# the second launch; the A/B switch of tools/vae_time.py --ab-post-norm and of the parity tests)
CONV_POST_NORM_FUSE = True
# conv3d(post_norm=..., keep_raw=True): the consumer's norm as a second output of the producing convolution where it can
# (False: always the second launch; tools/vae_time.py --ab-second-output)
CONV_SECOND_OUTPUT_FUSE = True
# conv3d: give the library the workspace it asks for (ltxmi_conv3d_workspace_bytes), i.e. let the wide, short layers run split over
# their input channels (False: never; tools/vae_time.py --ab-split)
CONV_SPLIT = True
_conv_workspace = {}


# conv3d(pad_replicate=...): the spatial padding mode, ltxmi_conv3d_args.pad_replicate (False / True are the first two)
PAD_ZEROS, PAD_REPLICATE, PAD_REFLECT = _header("PAD_ZEROS", "PAD_REPLICATE", "PAD_REFLECT")


def _conv3d_args(x, w_packed, bias, causal, pad_replicate, d2s, residual, add, out, stride, tpad, out_T, kernel_t,
                 time_pad_zeros, algo, post_norm, keep_raw, workspace, out_norm, launch):
    """The ltxmi_conv3d_args of a ``conv3d`` / ``conv3d_route`` call -> (args, out, out_norm, second_launch, key).  ``launch``
    False (the route query): nothing is allocated -- a missing ``out`` / second output / workspace is stood in for by what a
    fresh allocation always is, 16-byte aligned and large enough -- and the tensors may live on any device."""
    (_chk_bf16 if launch else _chk_bf16_any_device)(x, w_packed, bias, residual, add, out, out_norm)
    B, T, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    if not x.is_contiguous() or not w_packed.is_contiguous():
        raise ValueError("ltxmi.conv3d: x and w must be contiguous")
    st, sh, sw = stride
    if sh != sw:
        raise ValueError("ltxmi.conv3d: height and width strides must be equal")
    front = tpad if tpad > 0 else (2 if causal else 1)
    back = 0 if (tpad > 0 or causal) else 1
    oT = out_T if out_T > 0 else (T + front + back - 3) // st + 1
    if kernel_t == 1:
        oT = T
    if w_packed.shape[1] != 9 * kernel_t * Cin:
        raise ValueError(f"ltxmi.conv3d: packed weight has K={w_packed.shape[1]}, expected {9 * kernel_t * Cin}")
    oH, oW = (H - 1) // sh + 1, (W - 1) // sh + 1
    out_shape = (B, 2 * T - 1, 2 * H, 2 * W, Cout // 8) if d2s else (B, oT, oH, oW, Cout)
    if out is None and launch:
        out = torch.empty(out_shape, dtype=BF16, device=x.device)
    a = _lib.Conv3dArgs()
    a.x, a.w, a.bias = x.data_ptr(), w_packed.data_ptr(), (bias.data_ptr() if bias is not None else None)
    a.y = out.data_ptr() if out is not None else 256
    a.B, a.T, a.H, a.W, a.Cin, a.Cout = B, T, H, W, Cin, Cout
    a.causal, a.pad_replicate, a.d2s = int(causal), int(pad_replicate), int(d2s)
    a.stride_t, a.stride_hw, a.tpad, a.out_T = st, sh, tpad, out_T
    a.kernel_t, a.time_pad_zeros = kernel_t, int(time_pad_zeros)
    a.algo = CONV_ALGO if algo is None else algo
    if residual is not None:
        a.residual, a.res_channels = residual.data_ptr(), residual.shape[-1]
    if add is not None:
        if not add.is_contiguous() or add.shape != (B, oT, oH, oW, Cout):
            raise ValueError("ltxmi.conv3d: `add` must be a contiguous [B,T,H,W,Cout] tensor")
        a.add = add.data_ptr()
    if out_norm is not None and (not keep_raw or not out_norm.is_contiguous() or out_norm.shape != out_shape):
        raise ValueError("ltxmi.conv3d: out_norm is the second output of keep_raw, contiguous and of the output's shape")
    if keep_raw and post_norm is None:
        raise ValueError("ltxmi.conv3d: keep_raw is for post_norm")
    if post_norm is not None:
        scale, shift, eps = post_norm
        if (scale is None) != (shift is None) or ((d2s or add is not None) and not keep_raw):
            raise ValueError("ltxmi.conv3d: post_norm needs scale and shift together, and (without keep_raw) the plain store "
                             "without `add`")
        c_norm = Cout // 8 if d2s else Cout
        for t in (scale, shift):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape != (B, c_norm)
                                  or (launch and not t.is_cuda)):
                raise ValueError("ltxmi.conv3d: post_norm scale / shift must be contiguous fp32 [B, C] device tensors")
        if keep_raw and launch and out_norm is None:
            out_norm = torch.empty(out_shape, dtype=BF16, device=x.device)
        if CONV_SECOND_OUTPUT_FUSE if keep_raw else CONV_POST_NORM_FUSE:
            a.post_norm, a.post_scale, a.post_shift, a.post_eps = 1, _ptr(scale), _ptr(shift), eps
            if keep_raw:
                a.y_norm = out_norm.data_ptr() if out_norm is not None else 512
    # Scratch for the channel-split form of the wide, short layers (ltxmi_conv3d_args.workspace): one buffer per (device, stream),
    # grown on demand, shared by every call on that stream (stream-ordered: the next call's writes follow this call's reads).  Asked
    # with the norm request in place (at 512 input channels the split pays only when the norm rides along), as the launch sees it.
    # ``workspace`` (a uint8 tensor): the caller's own scratch instead, handed to the library as it is, whatever its size.
    if workspace is not None:
        if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or (launch and not workspace.is_cuda):
            raise ValueError("ltxmi.conv3d: workspace must be a contiguous uint8 device tensor")
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    elif CONV_SPLIT:
        want = int(lib.ltxmi_conv3d_workspace_bytes(ctypes.byref(a)))
        if want > 0 and not launch:
            a.workspace, a.workspace_bytes = 256, want
        elif want > 0:
            key = (x.device, torch.cuda.current_stream().cuda_stream)
            ws = _conv_workspace.get(key)
            if ws is None or ws.numel() < want:
                if ws is None and len(_conv_workspace) >= 8:          # streams come and go: do not keep their buffers for ever
                    _conv_workspace.clear()
                ws = _conv_workspace[key] = torch.empty(want, dtype=torch.uint8, device=x.device)
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    if a.post_norm and not lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)):
        a.post_norm, a.post_scale, a.post_shift, a.post_eps, a.y_norm = 0, None, None, 0.0, None
    second_launch = post_norm if post_norm is not None and not a.post_norm else None
    # (watched either by shape alone or by shape + epilogue: "plain" / "add" / "post_norm" / "second_output")
    kind = ("second_output" if a.y_norm else "post_norm") if a.post_norm else ("add" if add is not None else "plain")
    key = ("conv3d", B * oT * oH * oW, Cin, Cout, int(d2s))
    return a, out, out_norm, second_launch, (key, key + (kind,))


def conv3d(x, w_packed, bias, causal, pad_replicate, d2s=False, residual=None, add=None, out=None,
           stride=(1, 1, 1), tpad=0, out_T=0, kernel_t=3, time_pad_zeros=False, algo=None, post_norm=None, keep_raw=False,
           workspace=None, out_norm=None):
    """x [B,T,H,W,Cin] NDHWC; w_packed [Cout, 27*Cin] (tap-major; (p1p2p3, c')-major rows when d2s).
    stride = (st, s, s) with st, s in {1, 2}; tpad / out_T: front time padding and output frames
    when they differ from CausalConv3d's (0 = default); kernel_t = 1: per-frame 3x3 Conv2d
    (w_packed [Cout, 9*Cin]); time_pad_zeros: nn.Conv3d zero padding in time.  See include/ltxmi.h.
    post_norm = (scale fp32 [B,Cout] or None, shift, eps): the result goes through PixelNorm -> (1+scale) x + shift -> SiLU
    (``pixelnorm_ada_silu``) -- in the convolution's epilogue where the kernel can (ltxmi_conv3d_fuses_post_norm), as a
    second launch on the result otherwise.
    keep_raw (with post_norm): return (raw, activated) -- the raw result too, for the skip path of the block that consumes the
    activated one (the NEXT block's norm1 -> AdaLN -> SiLU riding on this convolution: ltxmi_conv3d_args.y_norm); allowed
    with `add` and with d2s.
    workspace: a uint8 device tensor to use as ltxmi_conv3d_args.workspace instead of the module's own buffer; out_norm: where
    keep_raw's activated output goes (allocated if None).
    pad_replicate: the spatial padding mode -- PAD_ZEROS / PAD_REPLICATE / PAD_REFLECT (0 / 1 / 2; False / True mean the first
    two).  Reflect is torch's (index -1 reads index 1, the edge is not repeated) and needs H, W >= 2; the time axis is never
    mirrored."""
    a, out, out_norm, second_launch, keys = _conv3d_args(x, w_packed, bias, causal, pad_replicate, d2s, residual, add, out, stride,
                                                         tpad, out_T, kernel_t, time_pad_zeros, algo, post_norm, keep_raw,
                                                         workspace, out_norm, True)
    tok = _prof_begin(*keys)
    check(lib.ltxmi_conv3d_ndhwc_bf16(ctypes.byref(a), _stream()), "ltxmi_conv3d_ndhwc_bf16")
    _prof_end(tok)
    if second_launch is not None:
        pixelnorm_ada_silu(out, second_launch[0], second_launch[1], True, second_launch[2], out=out_norm if keep_raw else out)
    return (out, out_norm) if keep_raw else out


# ltxmi_conv_route: ltxmi_conv3d_route_info.route
CONV_GEMM128, CONV_GEMM256, CONV_DIRECT8, CONV_DIRECT4 = _header("CONV_GEMM128", "CONV_GEMM256", "CONV_DIRECT8", "CONV_DIRECT4")


def conv3d_route(x, w_packed, bias, causal, pad_replicate, d2s=False, residual=None, add=None, out=None,
                 stride=(1, 1, 1), tpad=0, out_T=0, kernel_t=3, time_pad_zeros=False, algo=None, post_norm=None, keep_raw=False,
                 workspace=None, out_norm=None):
    """How ``conv3d`` runs the same arguments: dict(route, epilogue, ksplit, swap_hw, finalize_blocks, second_launch) of
    ltxmi_conv3d_route_info (include/ltxmi.h) for the convolution launch ``conv3d`` makes -- ``second_launch``: the norm
    follows as a launch of its own -- or the negative status ``conv3d`` would raise on.  Built from the same struct as the launch
    and decided by the same code; nothing is launched or read, so the tensors may live on any device (only their shapes and
    addresses count)."""
    a, _, _, second_launch, _ = _conv3d_args(x, w_packed, bias, causal, pad_replicate, d2s, residual, add, out, stride, tpad,
                                             out_T, kernel_t, time_pad_zeros, algo, post_norm, keep_raw, workspace, out_norm,
                                             False)
    info = _lib.Conv3dRouteInfo()
    rc = int(lib.ltxmi_conv3d_route(ctypes.byref(a), ctypes.byref(info)))
    if rc != 0:
        return rc
    return dict(route=info.route, epilogue=info.epilogue, ksplit=info.ksplit, swap_hw=info.swap_hw,
                finalize_blocks=info.finalize_blocks, second_launch=second_launch is not None)


def pixelnorm_ada_silu(x, scale=None, shift=None, apply_silu=True, eps=1e-8, out=None):
    """x NDHWC [B,T,H,W,C]; scale/shift fp32 [B,C] or None."""
    _chk_bf16(x, out)
    B, C = x.shape[0], x.shape[-1]
    rows = x.numel() // C
    out = torch.empty_like(x) if out is None else out
    check(lib.ltxmi_pixelnorm_ada_silu_bf16(_ptr(x), _ptr(out), rows, C, rows // B, _ptr(scale), _ptr(shift),
                                            int(apply_silu), eps, _stream()), "ltxmi_pixelnorm_ada_silu_bf16")
    return out


def layernorm_affine(x, gamma, beta, eps, out=None):
    _chk_bf16(x, gamma, beta, out)
    C = x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    check(lib.ltxmi_layernorm_affine_bf16(_ptr(x), _ptr(out), x.numel() // C, C, _ptr(gamma), _ptr(beta), eps,
                                          _stream()), "ltxmi_layernorm_affine_bf16")
    return out


def ncdhw_to_ndhwc(z, std=None, mean=None):
    _chk_bf16(z)
    B, C, T, H, W = z.shape
    out = torch.empty((B, T, H, W, C), dtype=BF16, device=z.device)
    check(lib.ltxmi_ncdhw_to_ndhwc_bf16(_ptr(z.contiguous()), _ptr(out), B, C, T, H, W, _ptr(std), _ptr(mean),
                                        _stream()), "ltxmi_ncdhw_to_ndhwc_bf16")
    return out


def unpatchify_to_ncdhw(x, c_out, patch):
    _chk_bf16(x)
    B, T, H, W, Cp = x.shape
    if not x.is_contiguous() or Cp != c_out * patch * patch:
        raise ValueError(f"ltxmi.unpatchify_to_ncdhw: x must be contiguous with {c_out * patch * patch} channels")
    out = torch.empty((B, c_out, T, H * patch, W * patch), dtype=BF16, device=x.device)
    check(lib.ltxmi_unpatchify_to_ncdhw_bf16(_ptr(x), _ptr(out), B, T, H, W, c_out, patch, _stream()),
          "ltxmi_unpatchify_to_ncdhw_bf16")
    return out


def patchify_to_ndhwc(x, patch, c_pad):
    """pixels [B,C,T,H,W] -> NDHWC [B,T,H/p,W/p,c_pad] (zero channels beyond C*p*p)."""
    _chk_bf16(x)
    B, C, T, H, W = x.shape
    out = torch.empty((B, T, H // patch, W // patch, c_pad), dtype=BF16, device=x.device)
    check(lib.ltxmi_patchify_to_ndhwc_bf16(_ptr(x.contiguous()), _ptr(out), B, C, T, H, W, patch, c_pad, _stream()),
          "ltxmi_patchify_to_ndhwc_bf16")
    return out


def space_to_depth_skip(conv, x, stride):
    """conv [B,T',H,W,Cc] (T' = T+1 when stride[0] == 2), x [B,T,H,W,Cin] -> [B,T'/st,H/s,W/s,Cc*st*s*s]."""
    _chk_bf16(conv, x)
    B, T, H, W, Cin = x.shape
    Cc = conv.shape[-1]
    st, s, _ = stride
    Tc = T + 1 if st == 2 else T
    if tuple(conv.shape) != (B, Tc, H, W, Cc) or not conv.is_contiguous() or not x.is_contiguous() or Cin % Cc:
        raise ValueError(f"ltxmi.space_to_depth_skip: conv {tuple(conv.shape)} does not match x {tuple(x.shape)}")
    out = torch.empty((B, Tc // st, H // s, W // s, Cc * st * s * s), dtype=BF16, device=x.device)
    check(lib.ltxmi_space_to_depth_skip_bf16(_ptr(conv), _ptr(x), _ptr(out), B, T, H, W, Cin, Cc, st, s, Cin // Cc,
                                             _stream()), "ltxmi_space_to_depth_skip_bf16")
    return out


def ndhwc_to_ncdhw(x, c0, C, std=None, mean=None):
    """channels c0..c0+C of NDHWC x -> NCDHW [B,C,T,H,W], optionally (v - mean) / std per channel."""
    _chk_bf16(x)
    B, T, H, W, ld = x.shape
    if not x.is_contiguous():
        raise ValueError("ltxmi.ndhwc_to_ncdhw: x must be contiguous")
    out = torch.empty((B, C, T, H, W), dtype=BF16, device=x.device)
    check(lib.ltxmi_ndhwc_to_ncdhw_bf16(_ptr(x), ld, c0, _ptr(out), B, C, T, H, W, _ptr(std), _ptr(mean), _stream()),
          "ltxmi_ndhwc_to_ncdhw_bf16")
    return out


# Loop-invariant reuse across denoise steps (caption projection, text keys/values): exact, on by default;
# bench.py switches it off for its headline number so that every step of the timed region does all the work
# the reference's step does.
STEP_INVARIANT_CACHING = True
# Without that cache every step projects the prompt through every layer's to_k / to_v (the reference's own schedule:
# attention.py:1042-1048 once per block and step).  768 text rows make a skinny GEMM per layer (192 workgroups of 128 x 128 on 256
# CUs, 11 % matrix-pipe busy); Transformer3DModel.forward therefore runs ALL layers' projections as one GEMM against the
# stacked weights before the block loop (same kernels' arithmetic, bit-identical values) and hands each block its slice.
STACKED_TEXT_KV = True


def set_step_invariant_caching(enabled: bool):
    global STEP_INVARIANT_CACHING
    STEP_INVARIANT_CACHING = bool(enabled)


GUIDANCE_WORKSPACE_FLOATS, = _header("GUIDANCE_WORKSPACE_FLOATS")


def _chk_guidance(what, noise_pred, latents, workspace, cond_mask, batched):
    """The tests ``guidance_step_`` (one video: b = 1 whatever latents' leading dimension) and ``guidance_step_batched_``
    share -> (b, num_conds, n, C, is_bf16)."""
    _chk_bf16(noise_pred)
    is_bf16 = latents.dtype == BF16
    if not is_bf16 and latents.dtype != torch.float32:
        raise TypeError(f"ltxmi.{what}: latents must be fp32 or bf16")
    b = latents.shape[0] if batched else 1
    if batched and (latents.dim() != 3 or noise_pred.dim() != 3 or not noise_pred.is_contiguous() or noise_pred.shape[0] % b != 0):
        raise ValueError(f"ltxmi.{what}: noise_pred must be contiguous [num_conds * b, N, C] for latents [b, N, C]")
    n = noise_pred[0].numel()
    if not latents.is_contiguous() or latents.numel() != b * n:
        raise ValueError(f"ltxmi.{what}: latents must be contiguous and match one chunk of noise_pred")
    if workspace.dtype != torch.float32 or workspace.numel() < b * GUIDANCE_WORKSPACE_FLOATS:
        raise ValueError(f"ltxmi.{what}: workspace must hold {f'{b} x ' if batched else ''}{GUIDANCE_WORKSPACE_FLOATS} fp32 values")
    C = noise_pred.shape[-1]
    if cond_mask is not None and (cond_mask.dtype != torch.float32 or not cond_mask.is_contiguous()
                                  or cond_mask.numel() * C != b * n):
        raise ValueError(f"ltxmi.{what}: cond_mask must be contiguous fp32 with one value per token")
    return b, noise_pred.shape[0] // b, n, C, is_bf16


def guidance_step_(noise_pred, latents, dt, guidance_scale, stg_scale, rescaling_scale, do_cfg, do_stg, do_rescale,
                   workspace, cond_mask=None, t=0.0):
    """noise_pred bf16 [num_conds, N, C] (one sample); latents fp32/bf16 [1, N, C], updated in place.
    cond_mask fp32 [1, N] (or None): only tokens with t - 1e-6 < 1 - cond_mask are advanced."""
    _, num_conds, n, C, is_bf16 = _chk_guidance("guidance_step_", noise_pred, latents, workspace, cond_mask, False)
    if cond_mask is None:
        check(lib.ltxmi_guidance_step_bf16(_ptr(noise_pred), n, num_conds, guidance_scale, stg_scale, rescaling_scale,
                                           int(do_cfg), int(do_stg), int(do_rescale), _ptr(latents), int(is_bf16),
                                           float(dt), _ptr(workspace), _stream()), "ltxmi_guidance_step_bf16")
        return latents
    check(lib.ltxmi_guidance_step_masked_bf16(_ptr(noise_pred), n, num_conds, guidance_scale, stg_scale,
                                              rescaling_scale, int(do_cfg), int(do_stg), int(do_rescale),
                                              _ptr(latents), int(is_bf16), float(dt), _ptr(cond_mask), C, float(t),
                                              _ptr(workspace), _stream()), "ltxmi_guidance_step_masked_bf16")
    return latents


def guidance_step_batched_(noise_pred, latents, dt, guidance_scale, stg_scale, rescaling_scale, do_cfg, do_stg, do_rescale,
                           workspace, cond_mask=None, t=0.0):
    """The step for b videos of one call: noise_pred bf16 [num_conds * b, N, C] in chunk order (uncond x b, text x b,
    perturbed x b); latents fp32/bf16 [b, N, C], updated in place; cond_mask fp32 [b, N] (or None); workspace fp32 of at
    least b * GUIDANCE_WORKSPACE_FLOATS values.  Video j gets the bits ``guidance_step_`` gives for noise_pred[j::b],
    latents[j:j + 1], cond_mask[j:j + 1]: every sum of the guidance is per video."""
    b, num_conds, n, C, is_bf16 = _chk_guidance("guidance_step_batched_", noise_pred, latents, workspace, cond_mask, True)
    check(lib.ltxmi_guidance_step_batched_bf16(_ptr(noise_pred), b, n, num_conds, guidance_scale, stg_scale,
                                               rescaling_scale, int(do_cfg), int(do_stg), int(do_rescale),
                                               _ptr(latents), int(is_bf16), float(dt),
                                               None if cond_mask is None else _ptr(cond_mask), C, float(t),
                                               _ptr(workspace), workspace.numel(), _stream()),
          "ltxmi_guidance_step_batched_bf16")
    return latents


def image_cond_noise_(latents, init_latents, noise, cond_mask, noise_scale, t):
    """latents/init_latents/noise [b, N, C] (all fp32 or all bf16), cond_mask fp32 [b, N]; in place."""
    is_bf16 = latents.dtype == BF16
    for x in (latents, init_latents, noise):
        if x.dtype != latents.dtype or x.shape != latents.shape or not x.is_contiguous():
            raise ValueError("ltxmi.image_cond_noise_: latents, init_latents and noise must match and be contiguous")
    if latents.dtype not in (BF16, torch.float32) or cond_mask.dtype != torch.float32 or not cond_mask.is_contiguous():
        raise TypeError("ltxmi.image_cond_noise_: fp32/bf16 latents and a contiguous fp32 mask expected")
    C = latents.shape[-1]
    tokens = latents.numel() // C
    if cond_mask.numel() != tokens:
        raise ValueError("ltxmi.image_cond_noise_: one mask value per token expected")
    check(lib.ltxmi_image_cond_noise(_ptr(latents), _ptr(init_latents), _ptr(noise), int(is_bf16), _ptr(cond_mask),
                                     tokens, C, float(noise_scale), float(t), _stream()), "ltxmi_image_cond_noise")
    return latents


def groupnorm_silu(x, gamma, beta, groups, eps, residual=None, samples=None, out=None):
    """x channels-last [..., C]; statistics per sample over everything but the leading ``samples``
    rows-groups (samples = B for 5-D NDHWC input by default; pass B*T for per-frame GroupNorm)."""
    _chk_bf16(x, gamma, beta, residual, out)
    if not x.is_contiguous() or (residual is not None and (not residual.is_contiguous() or residual.shape != x.shape)):
        raise ValueError("ltxmi.groupnorm_silu: x / residual must be contiguous and equally shaped")
    C = x.shape[-1]
    samples = x.shape[0] if samples is None else samples
    S = x.numel() // C // samples
    out = torch.empty_like(x) if out is None else out
    # per-block partial sums [samples][max(1, 2048 // samples)][C][2] + the statistics [samples][groups][2] (include/ltxmi.h)
    ws = torch.empty(samples * (max(1, 2048 // samples) * 2 * C + 2 * groups), dtype=torch.float32, device=x.device)
    check(lib.ltxmi_groupnorm_silu_bf16(_ptr(x), _ptr(out), _ptr(residual), samples, S, C, groups, _ptr(gamma),
                                        _ptr(beta), eps, _ptr(ws), _stream()), "ltxmi_groupnorm_silu_bf16")
    return out


def pixel_shuffle2d(x):
    """x NDHWC [B,T,H,W,4C] (channel (p1 p2 c)) -> [B,T,2H,2W,C]."""
    _chk_bf16(x)
    B, T, H, W, C4 = x.shape
    if not x.is_contiguous() or C4 % 32:
        raise ValueError("ltxmi.pixel_shuffle2d: contiguous input with 4*C channels (C % 8 == 0) expected")
    out = torch.empty((B, T, 2 * H, 2 * W, C4 // 4), dtype=BF16, device=x.device)
    check(lib.ltxmi_pixel_shuffle2d_ndhwc_bf16(_ptr(x), _ptr(out), B * T, H, W, C4 // 4, _stream()),
          "ltxmi_pixel_shuffle2d_ndhwc_bf16")
    return out


def pixel_shuffle_nd(x, pt, ps, drop_first=False, out=None):
    """x NDHWC [B,T,H,W,pt*ps*ps*C] (channel (p1 p2 p3 c)) -> [B, pt*T - drop_first, ps*H, ps*W, C]: PixelShuffleND over
    time (pt = 2) and / or space (ps = 2), and with drop_first the temporal upsampler's ``x[:, :, 1:]`` in the same pass.
    ``out``: a contiguous tensor of that shape to write into."""
    _chk_bf16(x, out)
    if pt not in (1, 2) or ps not in (1, 2) or pt * ps == 1 or (drop_first and pt == 1):
        raise ValueError("ltxmi.pixel_shuffle_nd: pt, ps in {1, 2}, not both 1; drop_first needs pt = 2")
    B, T, H, W, Cp = x.shape
    f = pt * ps * ps
    if not x.is_contiguous() or Cp % (8 * f):
        raise ValueError(f"ltxmi.pixel_shuffle_nd: contiguous input with {f}*C channels (C % 8 == 0) expected")
    drop = int(bool(drop_first))
    shape = (B, pt * T - drop, ps * H, ps * W, Cp // f)
    if out is None:
        out = torch.empty(shape, dtype=BF16, device=x.device)
    elif tuple(out.shape) != shape or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"ltxmi.pixel_shuffle_nd: `out` must be a contiguous {list(shape)} tensor on x's device")
    check(lib.ltxmi_pixel_shuffle_nd_ndhwc_bf16(_ptr(x), _ptr(out), B, T, H, W, Cp // f, pt, ps, drop, _stream()),
          "ltxmi_pixel_shuffle_nd_ndhwc_bf16")
    return out


def adain_filter(latents, reference, factor=1.0):
    """latents [B,C,...], reference [B,C,...] (NCDHW, fp32 or bf16): per-(b,c) statistics transfer."""
    if latents.dtype != reference.dtype or latents.dtype not in (BF16, torch.float32):
        raise TypeError("ltxmi.adain_filter: fp32 or bf16 latents and reference of the same dtype expected")
    if latents.shape[:2] != reference.shape[:2]:
        raise ValueError("ltxmi.adain_filter: batch/channel sizes differ")
    latents, reference = latents.contiguous(), reference.contiguous()
    planes = latents.shape[0] * latents.shape[1]
    out = torch.empty_like(latents)
    check(lib.ltxmi_adain_filter(_ptr(latents), _ptr(reference), _ptr(out), int(latents.dtype == BF16), planes,
                                 latents.numel() // planes, reference.numel() // planes, float(factor), _stream()),
          "ltxmi_adain_filter")
    return out


BLEND_F32, BLEND_BF16, BLEND_F16 = _header("BLEND_F32", "BLEND_BF16", "BLEND_F16")      # ltxmi_blend_dtype


def tile_blend_(a, b, extent, dim):
    """In place in ``b``: the first ``extent`` slices of ``b`` along ``dim`` cross-faded with the last ``extent`` of ``a``
    (blend_z / blend_v / blend_h, vae.py:193-221).  a, b: contiguous, same dtype (fp32 or bf16), equal sizes on every
    other axis."""
    codes = {torch.float32: BLEND_F32, BF16: BLEND_BF16, torch.float16: BLEND_F16}
    if a.dtype != b.dtype or b.dtype not in codes:
        raise TypeError("ltxmi.tile_blend_: fp32, bf16 or fp16 tensors of the same dtype expected")
    if not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("ltxmi.tile_blend_: contiguous tensors expected")
    sa, sb = list(a.shape), list(b.shape)
    if len(sa) != len(sb) or sa[:dim] + sa[dim + 1:] != sb[:dim] + sb[dim + 1:]:
        raise ValueError("ltxmi.tile_blend_: shapes differ off the blended axis")
    extent = min(sa[dim], sb[dim], int(extent))
    if extent <= 0:
        return b
    outer = 1
    for n in sb[:dim]:
        outer *= n
    inner = 1
    for n in sb[dim + 1:]:
        inner *= n
    check(lib.ltxmi_tile_blend(_ptr(a), _ptr(b), codes[b.dtype], outer, sa[dim], sb[dim], inner, extent, _stream()),
          "ltxmi_tile_blend")
    return b


# ---- T5 text encoder (ltxmi/t5.py) ------------------------------------------------------------------------------------
def attention_relbias(q, k, v, rel_bias=None, rel_center=0, key_bias=None, softmax_scale=1.0, out=None):
    """softmax(softmax_scale q k^T + rel_bias[h, j - i] + key_bias[b, j]) v -- T5's attention (ltxmi_attention_relbias_bf16).
    q [B, Lq, H, 64], k / v [B, Lk, H, 64] as ``attention`` takes them (slices of one packed projection are fine).
    rel_bias: fp32 [H, >= rel_center + Lk], the value for head h and offset d = key - query at ``rel_bias[h, rel_center +
    d]``, rel_center >= Lq - 1; None: no relative bias, the call is ``attention``'s.  key_bias: fp32 [B, Lk] with the
    contract of ``attention`` (at or below -1e30 removes the key).  T5 does not scale its scores: softmax_scale = 1."""
    B, H, Lq, Lk, dh = dims = _chk_attn_qkv("attention_relbias", q, k, v, out)
    if out is None:
        out = torch.empty((B, Lq, H, dh), dtype=BF16, device=q.device)
    if tuple(out.shape) != (B, Lq, H, dh) or out.stride(3) != 1 or out.stride(2) != dh:
        raise ValueError(f"ltxmi.attention_relbias: out must be [B, Lq, H, dh] = {(B, Lq, H, dh)} with (heads, head_dim) contiguous")
    a = _lib.AttnRelBiasArgs()
    _attn_shared(a, "attention_relbias", True, dims, q, k, v, out, key_bias, float(softmax_scale))
    if rel_bias is not None:
        if rel_bias.dtype != torch.float32 or rel_bias.dim() != 2 or rel_bias.shape[0] != H or rel_bias.stride(1) != 1 \
                or not rel_bias.is_cuda or rel_bias.shape[1] < rel_center + Lk:
            raise ValueError("ltxmi.attention_relbias: rel_bias must be a CUDA fp32 [H, >= rel_center + Lk]")
        a.rel_bias, a.rel_stride_h, a.rel_center = rel_bias.data_ptr(), rel_bias.stride(0), rel_center
    tok = _prof_begin(("attention_relbias", B, H, Lq, Lk, dh))
    check(lib.ltxmi_attention_relbias_bf16(ctypes.byref(a), _stream()), "ltxmi_attention_relbias_bf16")
    _prof_end(tok)
    return out


def rmsnorm_weight(x, weight, eps, out=None):
    """T5LayerNorm, out of place: bf16(bf16(x * rsqrt(mean(x^2) + eps)) * weight).  x: [..., D] rows (row-strided 2-D views
    are fine); ``out`` must not overlap x."""
    _chk_bf16(x, weight, out)
    x2, rows, ldx = _rows(x)
    D = x2.shape[1]
    if weight.shape != (D,) or weight.stride(0) != 1:
        raise ValueError(f"ltxmi.rmsnorm_weight: weight must be a contiguous [{D}]")
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    o2, orows, ldy = _rows(out)
    if orows != rows or o2.shape[1] != D:
        raise ValueError("ltxmi.rmsnorm_weight: out must have x's rows and channels")
    tok = _prof_begin(("rmsnorm_weight", rows, D))
    check(lib.ltxmi_rmsnorm_weight_bf16(_ptr(x2), ldx, _ptr(o2), ldy, rows, D, _ptr(weight), float(eps), _stream()),
          "ltxmi_rmsnorm_weight_bf16")
    _prof_end(tok)
    return out


def gated_gelu(h, out=None):
    """h [rows, 2F] (the output of one GEMM against the stacked [wi_0; wi_1]) -> [rows, F]:
    bf16(bf16(gelu_tanh(h[:, :F])) * h[:, F:])."""
    _chk_bf16(h, out)
    h2, rows, ldh = _rows(h)
    if h2.shape[1] % 2:
        raise ValueError("ltxmi.gated_gelu: h must be [rows, 2F]")
    F = h2.shape[1] // 2
    if out is None:
        out = torch.empty((*h.shape[:-1], F), dtype=BF16, device=h.device)
    o2, orows, ldy = _rows(out)
    if orows != rows or o2.shape[1] != F:
        raise ValueError("ltxmi.gated_gelu: out must be [rows, F]")
    tok = _prof_begin(("gated_gelu", rows, F))
    check(lib.ltxmi_gated_gelu_bf16(_ptr(h2), ldh, _ptr(o2), ldy, rows, F, _stream()), "ltxmi_gated_gelu_bf16")
    _prof_end(tok)
    return out


def embedding(ids, table, out=None):
    """table[ids]: ids int64 on the device (any shape), table bf16 [vocab, D] -> [*ids.shape, D].  A row whose id is
    outside [0, vocab) comes back as zeros."""
    _chk_bf16(table, out)
    if ids.dtype != torch.int64 or not ids.is_cuda:
        raise TypeError(f"ltxmi.embedding: ids must be a CUDA int64 tensor, got {ids.dtype} on {ids.device}")
    if table.dim() != 2 or table.stride(1) != 1:
        raise ValueError("ltxmi.embedding: table must be [vocab, D] with a contiguous innermost dimension")
    flat = ids.reshape(-1).contiguous()
    vocab, D = table.shape
    if out is None:
        out = torch.empty((*ids.shape, D), dtype=BF16, device=table.device)
    o2, orows, ldo = _rows(out)
    if orows != flat.numel() or o2.shape[1] != D:
        raise ValueError("ltxmi.embedding: out must be [*ids.shape, D]")
    tok = _prof_begin(("embedding", flat.numel(), D))
    check(lib.ltxmi_embedding_bf16(_ptr(flat), _ptr(table), table.stride(0), vocab, _ptr(o2), ldo, flat.numel(), D, _stream()),
          "ltxmi_embedding_bf16")
    _prof_end(tok)
    return out


# ---- MX-FP8 (include/ltxmi_mx.h, bound by ltxmi/_lib_mx.py): e4m3 elements, one E8M0 scale byte per 32 elements of a row
E4M3 = torch.float8_e4m3fn


def _chk_mx8(what, q, scales, K):
    """q [rows, K] float8_e4m3fn (or uint8) and scales [rows, K / 32] uint8 on the device -> their 2-D row views."""
    if q.dtype not in (E4M3, torch.uint8) or scales.dtype != torch.uint8 or not q.is_cuda or not scales.is_cuda:
        raise TypeError(f"ltxmi.{what}: expected CUDA float8_e4m3fn elements and uint8 scales, got {q.dtype} / {scales.dtype} on "
                        f"{q.device} / {scales.device}")
    q2, rows, ldq = _rows(q)
    s2, srows, lds = _rows(scales)
    if q2.shape[1] != K or srows != rows or s2.shape[1] * 32 != K:
        raise ValueError(f"ltxmi.{what}: elements {tuple(q.shape)} and scales {tuple(scales.shape)} do not belong to K={K}")
    return q2, ldq, s2, lds, rows


def quantize_mx8(x, out=None):
    """x [..., K] bf16 (row-strided 2-D views are fine), K % 32 == 0 -> (q [..., K] float8_e4m3fn, scales [..., K / 32] uint8).
    ``out``: a (q, scales) pair to write into."""
    _chk_bf16(x)
    x2, rows, ldx = _rows(x)
    K = x2.shape[1]
    if K % 32:
        raise ValueError(f"ltxmi.quantize_mx8: K={K} must be a multiple of 32")
    if out is None:
        out = (torch.empty(x.shape, dtype=E4M3, device=x.device),
               torch.empty((*x.shape[:-1], K // 32), dtype=torch.uint8, device=x.device))
    q, scales = out
    q2, ldq, s2, lds, orows = _chk_mx8("quantize_mx8", q, scales, K)
    if orows != rows:
        raise ValueError("ltxmi.quantize_mx8: out must have x's rows")
    tok = _prof_begin(("quantize_mx8", rows, K))
    check(_lib_mx.lib.ltxmi_quantize_mx8_bf16(_ptr(x2), ldx, _ptr(q2), ldq, _ptr(s2), lds, rows, K, _stream()), "ltxmi_quantize_mx8_bf16")
    _prof_end(tok)
    return q, scales


def _gemm_mx8_pair(a, N, a2, w2, a2_group_cols):
    """The ltxmi_gemm_mx8_pair of a second operand pair, or None without one: a2 = (q [M, groups * K2], scales) (row-strided views
    are fine), w2 = (q [N, K2], scales)."""
    if a2 is None and w2 is None:
        return None
    if a2 is None or w2 is None:
        raise ValueError("ltxmi.gemm_mx8: a2 and w2 go together")
    K2 = w2[0].shape[-1]
    if a2_group_cols < 0 or (a2_group_cols > 0 and N % a2_group_cols):
        raise ValueError(f"ltxmi.gemm_mx8: a2_group_cols={a2_group_cols} must be 0 or divide N={N}")
    groups = N // a2_group_cols if a2_group_cols > 0 else 1
    t2, lda2, ts2, lda2_s, M2 = _chk_mx8("gemm_mx8", a2[0], a2[1], groups * K2)
    u2, ldw2, us2, ldw2_s, N2 = _chk_mx8("gemm_mx8", w2[0], w2[1], K2)
    if M2 != _rows(a)[1] or N2 != N:
        raise ValueError(f"ltxmi.gemm_mx8: a2 has {M2} rows, w2 has {N2}: expected {_rows(a)[1]}, {N}")
    pair = _lib_mxl.GemmMx8Pair()
    pair.A2q, pair.lda2, pair.A2_scales, pair.lda2_s = t2.data_ptr(), lda2, ts2.data_ptr(), lda2_s
    pair.W2q, pair.ldw2, pair.W2_scales, pair.ldw2_s = u2.data_ptr(), ldw2, us2.data_ptr(), ldw2_s
    pair.K2, pair.group_cols = K2, a2_group_cols
    return pair


def gemm_mx8(a, a_scales, w, w_scales, bias=None, out=None, epilogue=EPI_NONE, residual=None, gate_table=None, gate_temb=None,
             rows_per_group=1, mx_out=False, rowsumsq=None, rowsumsq_cols=0, a2=None, w2=None, a2_group_cols=0):
    """epi((a 2^a_scales)[M,K] @ (w 2^w_scales)[N,K]^T + bias) on the block-scaled MFMA; K % 128 == 0, N % 32 == 0.  The
    keywords are ``gemm``'s.  ``mx_out=False``: a bf16 [M,N] (``out``: the tensor to write).  ``mx_out=True``: the result is
    quantised from its fp32 value and returned as (q, scales) (``out``: such a pair); epilogue NONE or GELU_TANH.
    ``rowsumsq`` (fp32 [M, >= rowsumsq_cols / 64], epilogue NONE, bf16 output): also receives the per-64-column sums of squares
    of the bf16 outputs for the columns < rowsumsq_cols, as ``gemm``'s (include/ltxmi_mx_attn.h).
    ``a2`` = (q [M, groups * K2], scales), ``w2`` = (q [N, K2], scales): a second MX-FP8 operand pair accumulated behind the
    first, ``gemm``'s ``a2`` / ``w2`` / ``a2_group_cols`` in MX-FP8 (include/ltxmi_mx_lora.h); K2 % 128 == 0."""
    N, K = w.shape
    pair = _gemm_mx8_pair(a, N, a2, w2, a2_group_cols)
    aq, lda, aqs, lda_s, M = _chk_mx8("gemm_mx8", a, a_scales, K)
    wq, ldw, wqs, ldw_s, _ = _chk_mx8("gemm_mx8", w, w_scales, K)
    _chk_bf16(bias, residual, gate_table, gate_temb)
    args = _lib_mx.GemmMx8Args()
    if mx_out:
        if out is None:
            out = (torch.empty((M, N), dtype=E4M3, device=a.device), torch.empty((M, N // 32), dtype=torch.uint8, device=a.device))
        c2, ldcq, cs2, ldc_s, Mo = _chk_mx8("gemm_mx8", out[0], out[1], N)
        if Mo != M:
            raise ValueError("ltxmi.gemm_mx8: bad out shape")
        args.Cq, args.ldcq, args.C_scales, args.ldc_s = c2.data_ptr(), ldcq, cs2.data_ptr(), ldc_s
    else:
        if out is None:
            out = torch.empty((M, N), dtype=BF16, device=a.device)
        _chk_bf16(out)
        o2, Mo, ldc = _rows(out)
        if Mo != M or o2.shape[1] != N:
            raise ValueError("ltxmi.gemm_mx8: bad out shape")
        args.C, args.ldc = o2.data_ptr(), ldc
    args.Aq, args.lda, args.A_scales, args.lda_s = aq.data_ptr(), lda, aqs.data_ptr(), lda_s
    args.Wq, args.ldw, args.W_scales, args.ldw_s = wq.data_ptr(), ldw, wqs.data_ptr(), ldw_s
    args.bias = bias.data_ptr() if bias is not None else None
    args.M, args.N, args.K = M, N, K
    args.epilogue = epilogue
    if residual is not None:
        r2, Mr, ldr = _rows(residual)
        if Mr != M or r2.shape[1] != N:
            raise ValueError(f"ltxmi.gemm_mx8: residual is [{Mr},{r2.shape[1]}], expected [{M},{N}]")
        args.residual, args.ldr = r2.data_ptr(), ldr
    if (gate_table is None) != (gate_temb is None):
        raise ValueError("ltxmi.gemm_mx8: gate_table and gate_temb go together")
    if gate_table is not None:
        if gate_table.shape != (N,) or gate_temb.shape[-1] != N or gate_temb.stride(-1) != 1:
            raise ValueError(f"ltxmi.gemm_mx8: gate_table must be [{N}] and gate_temb [groups, {N}] with a contiguous last dimension")
        args.gate_table = gate_table.data_ptr()
        args.gate_temb = gate_temb.data_ptr()
        args.gate_ld = gate_temb.stride(0) if gate_temb.dim() == 2 else 0
    args.rows_per_group = rows_per_group
    if rowsumsq is not None:
        if rowsumsq.dtype != torch.float32 or not rowsumsq.is_cuda or rowsumsq.dim() != 2 or rowsumsq.shape[0] != M \
                or rowsumsq.stride(1) != 1 or rowsumsq.shape[1] * 64 < rowsumsq_cols:
            raise ValueError("ltxmi.gemm_mx8: rowsumsq must be a CUDA fp32 [M, >= rowsumsq_cols/64]")
    tok = _prof_begin(("gemm_mx8", M, N, K, epilogue))
    if pair is not None:
        rss = (None, 0, 0) if rowsumsq is None else (_ptr(rowsumsq), rowsumsq_cols, rowsumsq.stride(0))
        check(_lib_mxl.lib.ltxmi_gemm_mx8_pair2(ctypes.byref(args), ctypes.byref(pair), *rss, _stream()), "ltxmi_gemm_mx8_pair2")
    elif rowsumsq is None:
        check(_lib_mx.lib.ltxmi_gemm_mx8(ctypes.byref(args), _stream()), "ltxmi_gemm_mx8")
    else:
        check(_lib_mxa.lib.ltxmi_gemm_mx8_rowsumsq(ctypes.byref(args), _ptr(rowsumsq), rowsumsq_cols, rowsumsq.stride(0), _stream()),
              "ltxmi_gemm_mx8_rowsumsq")
    _prof_end(tok)
    return out


def norm_modulate_mx8(x, eps, kind, scale_table, scale_temb, shift_table, shift_temb, rows_per_group, out=None):
    """``quantize_mx8(norm_modulate(x, ...))`` in one row pass, bit for bit, without the bf16 tensor in between: x [..., D] bf16,
    D % 32 == 0 -> (q [..., D] float8_e4m3fn, scales [..., D / 32] uint8).  ``out``: a (q, scales) pair to write into."""
    _chk_bf16(x, scale_table, scale_temb, shift_table, shift_temb)
    x2, rows, ldx = _rows(x)
    D = x2.shape[1]
    if D % 32:
        raise ValueError(f"ltxmi.norm_modulate_mx8: D={D} must be a multiple of 32")
    if scale_temb.stride(0) != shift_temb.stride(0):
        raise ValueError("ltxmi.norm_modulate_mx8: scale/shift tables must share a row stride")
    if out is None:
        out = (torch.empty(x.shape, dtype=E4M3, device=x.device),
               torch.empty((*x.shape[:-1], D // 32), dtype=torch.uint8, device=x.device))
    q, scales = out
    q2, ldq, s2, lds, orows = _chk_mx8("norm_modulate_mx8", q, scales, D)
    if orows != rows:
        raise ValueError("ltxmi.norm_modulate_mx8: out must have x's rows")
    tok = _prof_begin(("norm_modulate_mx8", rows, D))
    check(_lib_mxa.lib.ltxmi_norm_modulate_mx8(_ptr(x2), ldx, _ptr(q2), ldq, _ptr(s2), lds, rows, D, eps, kind, _ptr(scale_table),
                                               _ptr(scale_temb), _ptr(shift_table), _ptr(shift_temb), scale_temb.stride(0),
                                               rows_per_group, _stream()), "ltxmi_norm_modulate_mx8")
    _prof_end(tok)
    return q, scales


# ---- the MX-FP8 T5 encoder (include/ltxmi_mx_t5.h, bound by ltxmi/_lib_mxt.py; ltxmi/t5_mx8.py)
MXT_FORMS, MXT_STAGES, MXT_MAX_ROWS = _lib_mxt.FORMS, _lib_mxt.STAGES, _lib_mxt.MAX_ROWS


def _gemm_mx8_skinny_args(a, a_scales, w, w_scales, bias, out, epilogue, residual):
    """The ``ltxmi_gemm_mx8_args`` of a bf16-output call and the tensor it writes."""
    N, K = w.shape
    a2, lda, as2, lda_s, M = _chk_mx8("gemm_mx8_skinny", a, a_scales, K)
    w2, ldw, ws2, ldw_s, _ = _chk_mx8("gemm_mx8_skinny", w, w_scales, K)
    _chk_bf16(bias, residual)
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
    _chk_bf16(out)
    o2, Mo, ldc = _rows(out)
    if Mo != M or o2.shape[1] != N:
        raise ValueError("ltxmi.gemm_mx8_skinny: bad out shape")
    args = _lib_mx.GemmMx8Args()
    args.C, args.ldc = o2.data_ptr(), ldc
    args.Aq, args.lda, args.A_scales, args.lda_s = a2.data_ptr(), lda, as2.data_ptr(), lda_s
    args.Wq, args.ldw, args.W_scales, args.ldw_s = w2.data_ptr(), ldw, ws2.data_ptr(), ldw_s
    args.bias = bias.data_ptr() if bias is not None else None
    args.M, args.N, args.K = M, N, K
    args.epilogue = epilogue
    args.rows_per_group = 1
    if residual is not None:
        r2, Mr, ldr = _rows(residual)
        if Mr != M or r2.shape[1] != N:
            raise ValueError(f"ltxmi.gemm_mx8_skinny: residual is [{Mr},{r2.shape[1]}], expected [{M},{N}]")
        args.residual, args.ldr = r2.data_ptr(), ldr
    return args, out


def gemm_mx8_skinny(a, a_scales, w, w_scales, bias=None, out=None, epilogue=EPI_NONE, residual=None, form=0):
    """``gemm_mx8`` for M <= MXT_MAX_ROWS rows, bf16 output, epilogue NONE or GATE_RESIDUAL without a gate (the residual may be
    ``out``): small output tiles that each walk all of K through a ring of LDS stages, bit-identical to ``gemm_mx8``
    (ltxmi_gemm_mx8_skinny).  ``form``: 0 chooses the tile form by shape, one of ``MXT_FORMS`` forces it."""
    args, out = _gemm_mx8_skinny_args(a, a_scales, w, w_scales, bias, out, epilogue, residual)
    tok = _prof_begin(("gemm_mx8_skinny", args.M, args.N, args.K, epilogue))
    check(_lib_mxt.lib.ltxmi_gemm_mx8_skinny(ctypes.byref(args), form, _stream()), "ltxmi_gemm_mx8_skinny")
    _prof_end(tok)
    return out


def gemm_mx8_skinny_form(a, a_scales, w, w_scales, bias=None, out=None, epilogue=EPI_NONE, residual=None, form=0):
    """The tile form ``gemm_mx8_skinny`` would run for these arguments (the launch's own check and plan; nothing is launched)."""
    args, _ = _gemm_mx8_skinny_args(a, a_scales, w, w_scales, bias, out, epilogue, residual)
    chosen = _lib_mxt.lib.ltxmi_gemm_mx8_skinny_form(ctypes.byref(args), form)
    check(min(chosen, 0), "ltxmi_gemm_mx8_skinny_form")
    return chosen


def _mx8_out(what, x, K, out):
    """The (q, scales) pair a fused row pass writes for the rows of ``x`` and K output channels -> its row views."""
    if out is None:
        out = (torch.empty((*x.shape[:-1], K), dtype=E4M3, device=x.device),
               torch.empty((*x.shape[:-1], K // 32), dtype=torch.uint8, device=x.device))
    q2, ldq, s2, lds, orows = _chk_mx8(what, out[0], out[1], K)
    return out, q2, ldq, s2, lds, orows


def rmsnorm_weight_mx8(x, weight, eps, out=None):
    """``quantize_mx8(rmsnorm_weight(x, weight, eps))`` in one row pass, bit for bit, without the bf16 tensor in between:
    x [..., D] bf16, D % 32 == 0 -> (q [..., D] float8_e4m3fn, scales [..., D / 32] uint8).  ``out``: such a pair to write into."""
    _chk_bf16(x, weight)
    x2, rows, ldx = _rows(x)
    D = x2.shape[1]
    if D % 32:
        raise ValueError(f"ltxmi.rmsnorm_weight_mx8: D={D} must be a multiple of 32")
    if weight.shape != (D,) or weight.stride(0) != 1:
        raise ValueError(f"ltxmi.rmsnorm_weight_mx8: weight must be a contiguous [{D}]")
    out, q2, ldq, s2, lds, orows = _mx8_out("rmsnorm_weight_mx8", x, D, out)
    if orows != rows:
        raise ValueError("ltxmi.rmsnorm_weight_mx8: out must have x's rows")
    tok = _prof_begin(("rmsnorm_weight_mx8", rows, D))
    check(_lib_mxt.lib.ltxmi_rmsnorm_weight_mx8(_ptr(x2), ldx, _ptr(q2), ldq, _ptr(s2), lds, rows, D, _ptr(weight), float(eps),
                                                _stream()), "ltxmi_rmsnorm_weight_mx8")
    _prof_end(tok)
    return out


def gated_gelu_mx8(h, out=None):
    """``quantize_mx8(gated_gelu(h))`` in one pass, bit for bit: h [rows, 2F] bf16, F % 32 == 0 -> (q [rows, F] float8_e4m3fn,
    scales [rows, F / 32] uint8).  ``out``: such a pair to write into."""
    _chk_bf16(h)
    h2, rows, ldh = _rows(h)
    if h2.shape[1] % 64:
        raise ValueError(f"ltxmi.gated_gelu_mx8: h must be [rows, 2F] with F a multiple of 32, got {tuple(h.shape)}")
    F = h2.shape[1] // 2
    out, q2, ldq, s2, lds, orows = _mx8_out("gated_gelu_mx8", h, F, out)
    if orows != rows:
        raise ValueError("ltxmi.gated_gelu_mx8: out must have h's rows")
    tok = _prof_begin(("gated_gelu_mx8", rows, F))
    check(_lib_mxt.lib.ltxmi_gated_gelu_mx8(_ptr(h2), ldh, _ptr(q2), ldq, _ptr(s2), lds, rows, F, _stream()), "ltxmi_gated_gelu_mx8")
    _prof_end(tok)
    return out
