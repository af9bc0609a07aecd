"""Argument validation of the four T5 entry points with no device: every refused call returns the status include/ltxmi.h
documents, before anything is launched (no GPU is visible to a CPU run, so a launch would come back as LTXMI_ERR_LAUNCH)."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -2
BASE = 1 << 30                                      # fake, 64-byte aligned addresses: nothing is dereferenced


def _attn(**over):
    from ltxmi import _lib
    a = _lib.AttnRelBiasArgs()
    a.q, a.k, a.v, a.o = BASE, BASE + 128, BASE + 256, BASE + (1 << 20)
    for n in ("q", "k", "v"):
        setattr(a, n + "_stride_b", 24 * 384)
        setattr(a, n + "_stride_l", 384)
    a.o_stride_b, a.o_stride_l = 24 * 128, 128
    a.B, a.H, a.Lq, a.Lk, a.head_dim = 2, 2, 24, 24, 64
    a.softmax_scale = 1.0
    a.rel_bias, a.rel_stride_h, a.rel_center = BASE + (2 << 20), 47, 23
    a.key_bias, a.bias_stride_b = BASE + (3 << 20), 24
    for k, v in over.items():
        setattr(a, k, v)
    return a


ATTN_REFUSED = [
    ("q NULL", dict(q=None), INVALID, "NULL"), ("o NULL", dict(o=None), INVALID, "NULL"),
    ("B 0", dict(B=0), INVALID, "non-positive"), ("H -1", dict(H=-1), INVALID, "non-positive"),
    ("Lq 0", dict(Lq=0), INVALID, "non-positive"), ("Lk 0", dict(Lk=0), INVALID, "non-positive"),
    ("head_dim 128", dict(head_dim=128), UNSUPPORTED, "head_dim"), ("head_dim 32", dict(head_dim=32), UNSUPPORTED, "head_dim"),
    ("Lq 513", dict(Lq=513, rel_center=512, rel_stride_h=600), UNSUPPORTED, "at most 512"),
    ("Lk 513", dict(Lk=513, rel_stride_h=600), UNSUPPORTED, "at most 512"),
    ("Lk 513, no rel_bias", dict(Lk=513, rel_bias=None), UNSUPPORTED, "at most 512"),
    ("center < Lq - 1", dict(rel_center=22), INVALID, "rel_center"),
    ("stride_h < center + Lk", dict(rel_stride_h=46), INVALID, "rel_stride_h"),
    ("q stride % 8", dict(q_stride_l=388), UNSUPPORTED, "multiples of 8"), ("o stride % 8", dict(o_stride_b=3076), UNSUPPORTED, "multiples of 8"),
    ("k + 8 bytes", dict(k=BASE + 8), UNSUPPORTED, "16-byte"), ("o + 2 bytes", dict(o=BASE + 2), UNSUPPORTED, "16-byte"),
    ("rel_bias + 2 bytes", dict(rel_bias=BASE + 2), UNSUPPORTED, "4-byte"), ("key_bias + 1 byte", dict(key_bias=BASE + 1), UNSUPPORTED, "4-byte"),
]


@pytest.mark.parametrize("case", ATTN_REFUSED, ids=lambda c: c[0])
def test_attention_relbias_refuses(case):
    from ltxmi import _lib
    what, over, status, word = case
    assert _lib.lib.ltxmi_attention_relbias_bf16(ctypes.byref(_attn(**over)), None) == status, _lib.lib.ltxmi_last_error()
    assert word.encode() in _lib.lib.ltxmi_last_error()


def test_attention_relbias_null_struct():
    from ltxmi import _lib
    assert _lib.lib.ltxmi_attention_relbias_bf16(None, None) == INVALID
    assert b"NULL" in _lib.lib.ltxmi_last_error()


ROWS = [
    # entry, arguments (without the stream), status, word of the message
    ("ltxmi_rmsnorm_weight_bf16", (None, 128, BASE, 128, 4, 128, BASE, 1e-6), INVALID, "NULL"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 128, None, 128, 4, 128, BASE, 1e-6), INVALID, "NULL"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 128, BASE + 4096, 128, 4, 128, None, 1e-6), INVALID, "NULL"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 128, BASE + 4096, 128, 0, 128, BASE, 1e-6), INVALID, "non-positive"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 128, BASE + 4096, 128, 4, -8, BASE, 1e-6), INVALID, "non-positive"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 128, BASE + 4096, 128, 4, 100, BASE, 1e-6), UNSUPPORTED, "multiple of 8"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 8200, BASE + 4096, 8200, 4, 8200, BASE, 1e-6), UNSUPPORTED, "8192"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 132, BASE + 4096, 128, 4, 128, BASE, 1e-6), UNSUPPORTED, "strides"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 64, BASE + 4096, 128, 4, 128, BASE, 1e-6), UNSUPPORTED, "strides"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE + 8, 128, BASE + 4096, 128, 4, 128, BASE, 1e-6), UNSUPPORTED, "16-byte"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 128, BASE + 4096, 128, 4, 128, BASE + 2, 1e-6), UNSUPPORTED, "16-byte"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 128, BASE + 4096, 128, 4 * (2 ** 24 - 1) + 1, 128, BASE, 1e-6), UNSUPPORTED, "at most"),
    ("ltxmi_rmsnorm_weight_bf16", (BASE, 128, BASE + 4096, 128, 2 ** 31 - 1, 128, BASE, 1e-6), UNSUPPORTED, "at most"),
    ("ltxmi_gated_gelu_bf16", (None, 512, BASE, 256, 4, 256), INVALID, "NULL"),
    ("ltxmi_gated_gelu_bf16", (BASE, 512, None, 256, 4, 256), INVALID, "NULL"),
    ("ltxmi_gated_gelu_bf16", (BASE, 512, BASE + 8192, 256, 0, 256), INVALID, "non-positive"),
    ("ltxmi_gated_gelu_bf16", (BASE, 512, BASE + 8192, 256, 4, 0), INVALID, "non-positive"),
    ("ltxmi_gated_gelu_bf16", (BASE, 512, BASE + 8192, 256, 4, 252), UNSUPPORTED, "multiple of 8"),
    ("ltxmi_gated_gelu_bf16", (BASE, 504, BASE + 8192, 256, 4, 256), UNSUPPORTED, "ldh"),
    ("ltxmi_gated_gelu_bf16", (BASE, 512, BASE + 8192, 248, 4, 256), UNSUPPORTED, "ldy"),
    ("ltxmi_gated_gelu_bf16", (BASE + 8, 512, BASE + 8192, 256, 4, 256), UNSUPPORTED, "16-byte"),
    ("ltxmi_embedding_bf16", (None, BASE, 128, 64, BASE + 65536, 128, 4, 128), INVALID, "NULL"),
    ("ltxmi_embedding_bf16", (BASE, None, 128, 64, BASE + 65536, 128, 4, 128), INVALID, "NULL"),
    ("ltxmi_embedding_bf16", (BASE, BASE, 128, 64, None, 128, 4, 128), INVALID, "NULL"),
    ("ltxmi_embedding_bf16", (BASE, BASE, 128, 0, BASE + 65536, 128, 4, 128), INVALID, "non-positive"),
    ("ltxmi_embedding_bf16", (BASE, BASE, 128, 64, BASE + 65536, 128, -1, 128), INVALID, "non-positive"),
    ("ltxmi_embedding_bf16", (BASE, BASE, 128, 64, BASE + 65536, 128, 4, 124), UNSUPPORTED, "multiple of 8"),
    ("ltxmi_embedding_bf16", (BASE, BASE, 120, 64, BASE + 65536, 128, 4, 128), UNSUPPORTED, "strides"),
    ("ltxmi_embedding_bf16", (BASE, BASE + 8, 128, 64, BASE + 65536, 128, 4, 128), UNSUPPORTED, "aligned"),
    ("ltxmi_embedding_bf16", (BASE + 4, BASE, 128, 64, BASE + 65536, 128, 4, 128), UNSUPPORTED, "aligned"),
    ("ltxmi_embedding_bf16", (BASE, BASE, 128, 64, BASE + 65536, 128, 2 ** 24, 128), UNSUPPORTED, "at most"),
]


@pytest.mark.parametrize("case", ROWS, ids=lambda c: f"{c[0]}-{c[3]}-{c[2]}")
def test_row_entries_refuse(case):
    from ltxmi import _lib
    name, args, status, word = case
    assert getattr(_lib.lib, name)(*args, None) == status, _lib.lib.ltxmi_last_error()
    assert word.encode() in _lib.lib.ltxmi_last_error()


def test_relbias_args_begin_as_attn_args_do():
    """ltxmi_attn_relbias_args is a prefix of ltxmi_attn_args by design (ops._attn_shared fills both): the same twenty
    fields, types and offsets, then its own three."""
    from ltxmi import _lib
    rel, attn = _lib.AttnRelBiasArgs, _lib.AttnArgs
    assert rel._fields_[:20] == attn._fields_[:20] and rel._fields_[19][0] == "softmax_scale"
    assert [getattr(rel, n).offset for n, _ in rel._fields_[:20]] == [getattr(attn, n).offset for n, _ in attn._fields_[:20]]
    assert [n for n, _ in rel._fields_[20:]] == ["rel_bias", "rel_stride_h", "rel_center"]
    assert _lib.SIGNATURES["ltxmi_attention_relbias_bf16"] == (ctypes.c_int32, [ctypes.POINTER(rel), ctypes.c_void_p])


def test_header_names_the_pipeline_lines_the_entries_serve():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ltxmi.h")).read()
    tail = text[text.index("T5-v1.1 text encoder"):]
    for entry in ("ltxmi_attention_relbias_bf16", "ltxmi_rmsnorm_weight_bf16", "ltxmi_gated_gelu_bf16", "ltxmi_embedding_bf16"):
        assert entry in tail
    assert tail.count("pipeline_ltx_video.py:405-417") >= 4 and "ltxv.py:200-209" in tail
