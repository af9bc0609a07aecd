"""CPU checks of the log-sum-exp output, the merge entry point and the ring / hybrid sequence parallelism: the ABI (header,
ctypes mirror, argument validation before any launch), the merge algebra on the fp64 double (tests/attn_lse_double.py) and
gloo runs at world sizes 2, 3 and 4 of ``ring_attn_forward`` / ``usp_attn_forward(ring_degree=2)`` with that double as the
attention and merge functions."""
import ctypes
import os
import re
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attn_lse_double as dbl  # noqa: E402
from test_abi import ATTN_KERNEL_IDS, HEADER  # noqa: E402

EPS = torch.finfo(torch.float64).eps


# ------------------------------------------------------------------ 1. ABI
def test_merge_entry_point_is_exported_and_declared():
    from ltxmi import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+ltxmi_attention_merge_bf16\s*\(\s*const\s+ltxmi_attn_merge_args\s*\*", text)
    assert hasattr(_lib.lib, "ltxmi_attention_merge_bf16") and "ltxmi_attention_merge_bf16" in _lib.SIGNATURES
    assert _lib.SIGNATURES["ltxmi_attention_merge_bf16"] == (ctypes.c_int32, [ctypes.POINTER(_lib.AttnMergeArgs), ctypes.c_void_p])


def test_ctypes_mirrors_match_the_header():
    """The classes are read from the header (tests/test_abi_binding.py holds every field's offset and size against the
    compiler's): what is left to say here is where the lse fields sit."""
    from ltxmi import _lib
    attn = [f[0] for f in _lib.AttnArgs._fields_]
    assert attn[-3:] == ["lse", "lse_stride_b", "lse_stride_h"]                     # appended at the tail
    assert attn[-5:-3] == ["redo_counter", "force_exact"]
    assert _lib.AttnArgs.lse_stride_h.offset + 8 == ctypes.sizeof(_lib.AttnArgs)     # ... of the struct itself, no padding behind
    assert [f[0] for f in _lib.AttnMergeArgs._fields_][:7] == ["n", "o_part", "o_part_stride_b", "o_part_stride_l", "lse_part",
                                                               "lse_part_stride_b", "lse_part_stride_h"]
    assert _lib.AttnArgs.lse.size == 8 and _lib.AttnArgs.lse_stride_b.size == 8 and _lib.AttnArgs.lse_stride_h.size == 8
    assert _lib.AttnMergeArgs.o_part.size == _lib.AttnMergeArgs.lse_part_stride_h.size == 8 * _lib.ATTN_MERGE_MAX
    assert _lib.ATTN_MERGE_MAX == _lib.CONSTANTS["LTXMI_ATTN_MERGE_MAX"] == 8


@pytest.mark.parametrize("case", ATTN_KERNEL_IDS, ids=lambda c: "x".join(map(str, c[:-1])))
def test_kernel_id_table_is_unchanged(case):
    from ltxmi import _lib
    *shape, want = case
    assert _lib.lib.ltxmi_attention_kernel_id(*shape) == want


# ------------------------------------------------------------------ 2. validation, no GPU
def _aligned(nbytes=1 << 16):
    buf = ctypes.create_string_buffer(nbytes + 64)
    return buf, (ctypes.addressof(buf) + 63) & ~63


def test_attention_rejects_a_bad_lse_before_any_launch():
    from ltxmi import _lib
    lib = _lib.lib
    keep, base = _aligned()
    at = _lib.AttnArgs()
    at.q = at.k = at.v = at.o = base
    at.B, at.H, at.Lq, at.Lk, at.head_dim = 2, 2, 8, 8, 64
    for f in ("q", "k", "v", "o"):
        setattr(at, f + "_stride_b", 8 * 128)
        setattr(at, f + "_stride_l", 128)
    at.softmax_scale = 0.125
    at.lse, at.lse_stride_b, at.lse_stride_h = base + 2, 16, 8                       # misaligned
    assert lib.ltxmi_attention_fwd_bf16(ctypes.byref(at), None) == -1
    assert b"lse" in lib.ltxmi_last_error()
    at.lse = base
    at.lse_stride_h = 4                                                              # rows of a head overlap
    assert lib.ltxmi_attention_fwd_bf16(ctypes.byref(at), None) == -1
    at.lse_stride_h, at.lse_stride_b = 8, 8                                          # batch rows overlap
    assert lib.ltxmi_attention_fwd_bf16(ctypes.byref(at), None) == -1
    at.lse_stride_h, at.lse_stride_b = 8, -16
    assert lib.ltxmi_attention_fwd_bf16(ctypes.byref(at), None) == -1


def _merge_args(base, n):
    from ltxmi import _lib
    a = _lib.AttnMergeArgs()
    a.n = n
    a.B, a.H, a.Lq, a.head_dim = 1, 2, 8, 64
    for i in range(min(max(n, 0), 8)):
        a.o_part[i], a.o_part_stride_b[i], a.o_part_stride_l[i] = base, 8 * 128, 128
        a.lse_part[i], a.lse_part_stride_b[i], a.lse_part_stride_h[i] = base, 16, 8
    a.o, a.o_stride_b, a.o_stride_l = base, 8 * 128, 128
    return a


def test_merge_rejects_bad_arguments_before_any_launch():
    from ltxmi import _lib
    lib = _lib.lib
    keep, base = _aligned()
    assert lib.ltxmi_attention_merge_bf16(None, None) == -1
    for n in (-1, 0, 1, 9, 100):
        assert lib.ltxmi_attention_merge_bf16(ctypes.byref(_merge_args(base, n)), None) == -1, n
        assert b"partials" in lib.ltxmi_last_error()
    a = _merge_args(base, 3)
    a.o_part[2] = None
    assert lib.ltxmi_attention_merge_bf16(ctypes.byref(a), None) == -1
    assert b"NULL" in lib.ltxmi_last_error()
    a = _merge_args(base, 3)
    a.lse_part[1] = None
    assert lib.ltxmi_attention_merge_bf16(ctypes.byref(a), None) == -1
    a = _merge_args(base, 2)
    a.lse_part[1] = base + 1                                                          # misaligned partial lse
    assert lib.ltxmi_attention_merge_bf16(ctypes.byref(a), None) == -1
    assert b"lse" in lib.ltxmi_last_error()
    a = _merge_args(base, 2)
    a.lse, a.lse_stride_b, a.lse_stride_h = base + 2, 16, 8                           # misaligned merged lse
    assert lib.ltxmi_attention_merge_bf16(ctypes.byref(a), None) == -1
    a = _merge_args(base, 2)
    a.o = None
    assert lib.ltxmi_attention_merge_bf16(ctypes.byref(a), None) == -1


def test_host_wrappers_refuse_cpu_tensors_and_bad_counts():
    from ltxmi import ops
    o = torch.zeros(1, 8, 2, 64, dtype=torch.bfloat16)
    l = torch.zeros(1, 2, 8)
    with pytest.raises(TypeError):
        ops.attention_merge([o, o], [l, l])
    with pytest.raises(ValueError):
        ops.attention_merge([o], [l])
    with pytest.raises(ValueError):
        ops.attention_merge([o] * 9, [l] * 9)
    with pytest.raises(TypeError):
        ops.attention(o, o, o, return_lse=True)


# ------------------------------------------------------------------ 4. merge algebra on the double
def _rand(B, L, H, dh, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, H, dh, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("cuts", [(5,), (1, 30), (7, 8, 40), (3, 3, 3, 3, 3), (2, 9, 11, 20, 21, 50, 60), (1, 2, 3, 4, 5, 6, 7)])
def test_split_keys_and_merge_reproduces_the_unsplit_softmax(cuts):
    B, Lq, Lk, H, dh = 2, 9, 64, 3, 16
    q, k, v = _rand(B, Lq, H, dh, 1), _rand(B, Lk, H, dh, 2) * 3, _rand(B, Lk, H, dh, 3)
    g = torch.Generator().manual_seed(4)
    bias = torch.randn(B, Lk, generator=g, dtype=torch.float64) * 4
    ref_o, ref_l = dbl.attention_lse(q, k, v, 0.25, bias)
    edges = [0, *cuts, Lk]
    assert 2 <= len(edges) - 1 <= 8
    parts = [dbl.attention_lse(q, k[:, a:b], v[:, a:b], 0.25, bias[:, a:b]) for a, b in zip(edges[:-1], edges[1:])]
    o, l = dbl.attention_merge([p[0] for p in parts], [p[1] for p in parts])
    # fp64 round-off: each softmax weight carries a few eps, sums over Lk keys
    bound = 16 * EPS * Lk
    assert (o - ref_o).abs().max() <= bound * ref_o.abs().max()
    assert (l - ref_l).abs().max() <= bound * ref_l.abs().max().clamp(min=1)


def test_a_chunk_with_every_key_removed_is_ignored():
    B, Lq, Lk, H, dh = 2, 5, 48, 2, 8
    q, k, v = _rand(B, Lq, H, dh, 5), _rand(B, Lk, H, dh, 6), _rand(B, Lk, H, dh, 7)
    bias = torch.zeros(B, Lk, dtype=torch.float64)
    bias[:, 16:32] = float("-inf")                          # the middle chunk: every key removed
    bias[0, 40:] = torch.finfo(torch.float32).min           # and a dtype-min tail in the last one
    ref_o, ref_l = dbl.attention_lse(q, k, v, 0.3, bias)
    parts = [dbl.attention_lse(q, k[:, a:b], v[:, a:b], 0.3, bias[:, a:b]) for a, b in ((0, 16), (16, 32), (32, 48))]
    assert torch.isinf(parts[1][1]).all() and (parts[1][1] < 0).all()
    parts[1] = (torch.full_like(parts[1][0], float("nan")), parts[1][1])
    o, l = dbl.attention_merge([p[0] for p in parts], [p[1] for p in parts])
    assert torch.isfinite(o).all() and torch.isfinite(l).all()
    assert (o - ref_o).abs().max() <= 16 * EPS * Lk * ref_o.abs().max()
    assert (l - ref_l).abs().max() <= 16 * EPS * Lk * ref_l.abs().max().clamp(min=1)
    # every partial empty: lse = -inf
    none = [(torch.full_like(parts[1][0], float("nan")), parts[1][1])] * 2
    assert (dbl.attention_merge([p[0] for p in none], [p[1] for p in none])[1] == float("-inf")).all()


# ------------------------------------------------------------------ 3. gloo: ring and hybrid against full attention
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, fn_name, q):
    for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        globals()[fn_name](rank, world)
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _run(fn_name, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, fn_name, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=30)
    for rank, res in results:
        assert res == "ok", f"rank {rank}:\n{res}"


def _global_qkv(B, N, H, dh):
    g = torch.Generator().manual_seed(11)
    return torch.randn(B, N, 3, H, dh, generator=g, dtype=torch.float64)


def _double_fns(calls):
    def attn_fn(q, k, v, scale):
        calls.append(k.shape[1])
        return dbl.attention_lse(q, k, v, scale)

    def merge_fn(outs, lses):
        return dbl.attention_merge(outs, lses)[0]
    return attn_fn, merge_fn


def _check(out, ref, n_keys):
    # fp64 round-off of a softmax over n_keys keys, as a multiple of eps x keys
    assert out.shape == ref.shape
    assert (out - ref).abs().max() <= 16 * EPS * n_keys * ref.abs().max()


def _case_ring(rank, world):
    from ltxmi import distributed as sp
    H = 4                                                  # world 3: 4 heads do not divide the ranks
    qkv = _global_qkv(2, 12 * world, H, 16)
    ref = dbl.attention_lse(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 0.25)[0]
    calls = []
    attn_fn, merge_fn = _double_fns(calls)
    local = sp.shard_tokens(qkv, rank, world).contiguous()
    out = sp.ring_attn_forward(local, 0.25, attn_fn=attn_fn, merge_fn=merge_fn)
    assert calls == [12] * world                           # one partial per shard, every shard once
    _check(out, sp.shard_tokens(ref, rank, world), qkv.shape[1])
    if H % world != 0:
        with pytest.raises(ValueError):
            sp.usp_attn_forward(local, 0.25, attn_fn=lambda q, k, v, s: q)      # the Ulysses mode cannot take this


def _case_hybrid(rank, world):
    from ltxmi import distributed as sp
    assert world == 4
    qkv = _global_qkv(2, 8 * world, 6, 16)                 # 6 heads: divisible by the Ulysses degree 2, not by the world 4
    ref = dbl.attention_lse(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 0.25)[0]
    calls = []
    attn_fn, merge_fn = _double_fns(calls)
    local = sp.shard_tokens(qkv, rank, world).contiguous()
    out = sp.usp_attn_forward(local, 0.25, attn_fn=attn_fn, ring_degree=2, merge_fn=merge_fn)
    assert calls == [16, 16]                               # two ring steps over blocks of U x N/P = 16 keys
    _check(out, sp.shard_tokens(ref, rank, world), qkv.shape[1])
    ug, rg = sp.hybrid_groups(2)
    assert dist.get_process_group_ranks(ug) == [rank // 2 * 2, rank // 2 * 2 + 1]
    assert dist.get_process_group_ranks(rg) == [rank % 2, rank % 2 + 2]
    # ring_degree = 1 is the plain Ulysses path: 6 heads on 4 ranks are refused there
    with pytest.raises(ValueError):
        sp.usp_attn_forward(local, 0.25, attn_fn=lambda q, k, v, s: q)
    with pytest.raises(ValueError):
        sp.hybrid_groups(3)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_ring_attention_equals_full_attention(world):
    _run("_case_ring", world)


def test_hybrid_ulysses_ring_equals_full_attention_at_world_4():
    _run("_case_hybrid", 4)
