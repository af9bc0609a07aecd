"""CPU-side checks of the drop-in boundary: libltxmi.so loads, exports every symbol that
include/ltxmi.h declares, and rejects bad arguments before touching a GPU (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ltxmi.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ltxmi_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from ltxmi import _lib
    names = declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} is declared in include/ltxmi.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in ltxmi/_lib.py"
    assert set(_lib.SIGNATURES) == set(names)
    assert _lib.lib.ltxmi_arch() == b"gfx950"
    assert b"ltxmi" in _lib.lib.ltxmi_version()


def test_header_cites_the_reference_for_every_entry_point():
    text = open(HEADER).read()
    for needle in ("attention.py:", "transformer3d.py:", "wan/modules/attention.py:", "causal_conv3d.py:",
                   "causal_video_autoencoder.py:", "pipeline_ltx_video.py:", "rf.py:"):
        assert needle in text, needle


def test_argument_validation_without_gpu():
    from ltxmi import _lib
    lib = _lib.lib
    # NULL struct
    assert lib.ltxmi_gemm_bf16(None, None) == -1
    assert b"NULL" in lib.ltxmi_last_error()
    a = _lib.GemmArgs()
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) & ~63
    a.A = a.W = a.C = base
    a.M, a.N, a.K = 16, 16, 100            # K not a multiple of 64
    a.lda = a.ldw = 128
    a.ldc = 16
    assert lib.ltxmi_gemm_bf16(ctypes.byref(a), None) == -2
    assert b"multiple of 64" in lib.ltxmi_last_error()
    at = _lib.AttnArgs()
    at.q = at.k = at.v = at.o = base
    at.B, at.H, at.Lq, at.Lk, at.head_dim = 1, 1, 8, 8, 48
    assert lib.ltxmi_attention_fwd_bf16(ctypes.byref(at), None) == -2
    assert b"head_dim" in lib.ltxmi_last_error()
    at.head_dim = 64
    at.Lk = 0
    assert lib.ltxmi_attention_fwd_bf16(ctypes.byref(at), None) == -1
    c = _lib.Conv3dArgs()
    c.x = c.w = c.y = base
    c.B, c.T, c.H, c.W, c.Cin, c.Cout = 1, 1, 2, 2, 32, 64     # Cin % 64 != 0
    assert lib.ltxmi_conv3d_ndhwc_bf16(ctypes.byref(c), None) == -2
    assert lib.ltxmi_silu_bf16(None, None, 8, None) == -1
    assert lib.ltxmi_rmsnorm_rope_bf16(base, 64, 4, 60, base, 1e-5, None, None, 0, 0, None) == -2


# ltxmi_attention_kernel_id over the product's shapes and every threshold of the selection: (B, H, Lq, Lk, head_dim,
# has_key_bias, k_stride_l, v_stride_l, id).  Ids: 0 / 1 / 2 attention.hip head_dim 64 (key bias / 64 rows per wave),
# 3 pipelined, 4 / 5 attention.hip head_dim 128 (key bias), 6 pipelined head_dim 128, 7 short keys; -1 not taken.
ATTN_KERNEL_IDS = [
    (3, 32, 4992, 4992, 64, 0, 6144, 6144, 3),
    (3, 4, 4992, 4992, 64, 0, 768, 768, 3),
    (3, 8, 4992, 4992, 64, 0, 1536, 1536, 3),
    (3, 32, 4992, 128, 64, 0, 4096, 4096, 7),
    (3, 32, 4992, 256, 64, 0, 4096, 4096, 7),
    (3, 32, 4992, 257, 64, 0, 4096, 4096, 3),
    (3, 32, 1023, 256, 64, 0, 4096, 4096, 3),
    (3, 32, 1024, 256, 64, 0, 4096, 4096, 7),
    (1, 191, 256, 512, 64, 0, 12224, 12224, 0),
    (1, 192, 256, 512, 64, 0, 12288, 12288, 3),
    (1, 511, 256, 512, 64, 0, 32704, 32704, 3),
    (1, 511, 256, 512, 64, 0, 5000000, 32704, 0),
    (1, 512, 256, 512, 64, 0, 32768, 32768, 3),
    (1, 512, 256, 512, 64, 0, 5000000, 32768, 2),
    (1, 12, 32760, 1023, 128, 0, 1536, 1536, 4),
    (1, 12, 32760, 1024, 128, 0, 1536, 1536, 6),
    (1, 127, 256, 1024, 128, 0, 16256, 16256, 4),
    (1, 128, 256, 1024, 128, 0, 16384, 16384, 6),
    (1, 12, 32760, 32760, 128, 0, 4608, 4608, 6),
    (1, 12, 32760, 512, 128, 0, 1536, 1536, 4),
    (3, 32, 4992, 4992, 64, 0, 204600, 6144, 3),
    (3, 32, 4992, 4992, 64, 0, 6144, 204600, 3),
    (3, 32, 4992, 4992, 64, 0, 204601, 6144, 2),
    (3, 32, 4992, 4992, 64, 0, 6144, 204601, 2),
    (1, 12, 32760, 32760, 128, 0, 32521, 4608, 6),
    (1, 12, 32760, 32760, 128, 0, 32522, 4608, 4),
    (3, 32, 4992, 4992, 64, 1, 6144, 6144, 1),
    (3, 4, 4992, 4992, 64, 1, 768, 768, 1),
    (3, 8, 4992, 4992, 64, 1, 1536, 1536, 1),
    (3, 32, 4992, 128, 64, 1, 4096, 4096, 7),
    (3, 32, 4992, 256, 64, 1, 4096, 4096, 7),
    (3, 32, 4992, 257, 64, 1, 4096, 4096, 1),
    (3, 32, 1023, 256, 64, 1, 4096, 4096, 1),
    (3, 32, 1024, 256, 64, 1, 4096, 4096, 7),
    (1, 191, 256, 512, 64, 1, 12224, 12224, 1),
    (1, 192, 256, 512, 64, 1, 12288, 12288, 1),
    (1, 511, 256, 512, 64, 1, 32704, 32704, 1),
    (1, 511, 256, 512, 64, 1, 5000000, 32704, 1),
    (1, 512, 256, 512, 64, 1, 32768, 32768, 1),
    (1, 512, 256, 512, 64, 1, 5000000, 32768, 1),
    (1, 12, 32760, 1023, 128, 1, 1536, 1536, 5),
    (1, 12, 32760, 1024, 128, 1, 1536, 1536, 5),
    (1, 127, 256, 1024, 128, 1, 16256, 16256, 5),
    (1, 128, 256, 1024, 128, 1, 16384, 16384, 5),
    (1, 12, 32760, 32760, 128, 1, 4608, 4608, 5),
    (1, 12, 32760, 512, 128, 1, 1536, 1536, 5),
    (3, 32, 4992, 4992, 64, 1, 204600, 6144, 1),
    (3, 32, 4992, 4992, 64, 1, 6144, 204600, 1),
    (3, 32, 4992, 4992, 64, 1, 204601, 6144, 1),
    (3, 32, 4992, 4992, 64, 1, 6144, 204601, 1),
    (1, 12, 32760, 32760, 128, 1, 32521, 4608, 5),
    (1, 12, 32760, 32760, 128, 1, 32522, 4608, 5),
    (0, 32, 4992, 4992, 64, 0, 6144, 6144, -1),
    (3, 0, 4992, 4992, 64, 0, 6144, 6144, -1),
    (3, 32, 0, 4992, 64, 0, 6144, 6144, -1),
    (3, 32, 4992, 0, 64, 0, 6144, 6144, -1),
    (3, 32, 4992, 4992, 96, 0, 6144, 6144, -1),
    (3, 32, 4992, 4992, 32, 0, 6144, 6144, -1),
    (3, 32, 4992, 4992, 64, 0, 0, 6144, -1),
    (3, 32, 4992, 4992, 64, 0, 6144, -8, -1),
    (-1, 32, 4992, 4992, 64, 0, 6144, 6144, -1),
]


@pytest.mark.parametrize("case", ATTN_KERNEL_IDS, ids=lambda c: "x".join(map(str, c[:-1])))
def test_attention_kernel_id_table(case):
    from ltxmi import _lib
    *shape, want = case
    assert _lib.lib.ltxmi_attention_kernel_id(*shape) == want


def test_host_ops_refuse_cpu_tensors():
    """The product path has no CPU fallback: CPU tensors are an error, not a slow path."""
    import torch
    from ltxmi import ops
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.gemm(x, w)
    with pytest.raises(TypeError):
        ops.gemm(x.float(), w.float())


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "ltx-video-gpupoor_amd", "ltxmi")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("the oracle", ""), f"{fn} mentions the oracle package"
            assert "/root/reference" not in src
