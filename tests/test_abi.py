"""CPU-side checks of the drop-in boundary: libltxmi.so loads, exports every symbol that
include/ltxmi.h declares, and rejects bad arguments before touching a GPU (no compute calls)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ltxmi.h")


def test_library_exports_every_declared_symbol():
    """The declared symbols are the binding's own parse of the header (ltxmi/_abi.py; tests/test_abi_binding.py holds that
    parse against the compiler); it reads every declaration or raises, so none is left out."""
    from ltxmi import _abi, _lib
    names = sorted(_abi.parse(open(HEADER).read(), _lib.STRUCT_NAMES).signatures)
    assert len(names) >= 47
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} is declared in include/ltxmi.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in ltxmi/_lib.py"
        fn, (res, args) = getattr(_lib.lib, n), _lib.SIGNATURES[n]
        assert fn.restype is res and list(fn.argtypes) == list(args), n
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


# ltxmi_gemm_kernel_id over the product's shapes and one row on each side of every threshold of the selection.  Each row is
# (what, M, N, K, overrides of the struct built by _gemm_geometry, id).  Ids: 0 the 128x128 tile kernel, 1 the non-persistent
# 256x256 one, 2 the persistent 256x256 one; negative = the ltxmi_status the launch would return.  The ids are worked out
# by hand from include/ltxmi.h (tiles = ceil(M/256) * ceil(N/256)), not read off the library.
GEMM_KERNEL_IDS = [
    # M >= 768 (3 x 43 = 129 tiles either side)
    ("M767", 767, 11008, 128, {}, 0),
    ("M768", 768, 11008, 128, {}, 2),
    # N >= 256 (128 tiles either side)
    ("N248", 32768, 248, 128, {}, 0),
    ("N256", 32768, 256, 128, {}, 2),
    # >= 128 tiles: 8 x 15 = 120, 8 x 16 = 128 (the last N tile 8 columns wide), 8 x 16 exactly; 127 x 1 and 128 x 1
    ("tiles120", 2048, 3840, 128, {}, 0),
    ("tiles128_ragged", 2048, 3848, 128, {}, 2),
    ("tiles128", 2048, 4096, 128, {}, 2),
    ("tiles127", 32512, 256, 128, {}, 0),
    ("tiles128_tall", 32513, 256, 128, {}, 2),
    # K >= 128 at a persistent-sized shape
    ("K64", 4097, 2056, 64, {}, 1),
    ("K128", 4097, 2056, 128, {}, 2),
    # the residual the persistent kernel reads 16 bytes at a time
    ("ldr_mod8_0", 4097, 2056, 128, dict(epilogue=3, residual=0, ldr=2064), 2),
    ("ldr_mod8_4", 4097, 2056, 128, dict(epilogue=3, residual=0, ldr=2060), 1),
    ("res_plus8", 4097, 2056, 128, dict(epilogue=3, residual=8, ldr=2064), 1),
    ("res_plus16", 4097, 2056, 128, dict(epilogue=3, residual=16, ldr=2064), 2),
    ("res_span_2p32", 1048576, 256, 128, dict(epilogue=3, residual=0, ldr=2048, ldc=256), 1),
    ("res_span_under", 1048576, 256, 128, dict(epilogue=3, residual=0, ldr=2040, ldc=256), 2),
    # 32-bit byte offsets: M * ldc * 2 < 2^32, 256 * lda * 2 < 2^31, 256 * ldw * 2 < 2^31
    ("c_span_under", 1048576, 256, 128, dict(ldc=2044), 2),
    ("c_span_2p32", 1048576, 256, 128, dict(ldc=2048), 1),
    ("lda_under", 2048, 4096, 128, dict(lda=(1 << 22) - 8), 2),
    ("lda_2p31", 2048, 4096, 128, dict(lda=1 << 22), 1),
    ("ldw_under", 2048, 4096, 128, dict(ldw=(1 << 22) - 8), 2),
    ("ldw_2p31", 2048, 4096, 128, dict(ldw=1 << 22), 1),
    # C only 8-byte aligned with ldc % 8 == 4: accepted, and no reason to leave the persistent kernel
    ("c_plus8_ldc4", 4097, 2056, 128, dict(C=8, ldc=2060), 2),
    ("c_plus8_ldc4_small", 129, 136, 64, dict(C=8, ldc=140), 0),
    # algo (diagnostics): 128 / 256 hold for every accepted shape
    ("small", 16, 16, 64, {}, 0),
    ("small_algo128", 16, 16, 64, dict(algo=128), 0),
    ("small_algo256", 16, 16, 64, dict(algo=256), 1),
    ("one_row_algo256", 1, 8, 64, dict(algo=256), 1),
    ("mid_algo256", 2048, 2048, 2048, dict(algo=256), 1),
    ("mid_algo0", 2048, 2048, 2048, {}, 0),
    ("large_algo128", 2048, 4096, 128, dict(algo=128), 0),
    ("large_algo256", 2048, 4096, 128, dict(algo=256), 1),
    ("algo7", 2048, 4096, 128, dict(algo=7), -1),
    # refused arguments
    ("K100", 16, 16, 100, dict(lda=128, ldw=128), -2),
    ("N12", 16, 12, 64, {}, -2),
    ("M0", 0, 16, 64, {}, -1),
    ("ldc_mod4", 16, 16, 64, dict(ldc=18), -2),
    ("ldc_below_N", 16, 16, 64, dict(ldc=8), -2),
    ("lda_mod8", 16, 16, 64, dict(lda=68), -2),
    ("c_plus4", 16, 16, 64, dict(C=4), -2),
    ("a_plus8", 16, 16, 64, dict(A=8), -2),
    ("bias_plus4", 16, 16, 64, dict(bias=4), -2),
    ("epilogue99", 16, 16, 64, dict(epilogue=99), -1),
    ("gate_without_residual", 16, 16, 64, dict(epilogue=3), -1),
    ("gate_table_without_temb", 16, 16, 64, dict(epilogue=3, residual=0, ldr=16, gate_table=0), -1),
    ("ldr_mod4", 16, 16, 64, dict(epilogue=3, residual=0, ldr=18), -1),
    ("ldr_below_N", 16, 16, 64, dict(epilogue=3, residual=0, ldr=8), -1),
    ("gate_ld_mod4", 16, 16, 64, dict(epilogue=3, residual=0, ldr=16, gate_table=0, gate_temb=0, gate_ld=18), -1),
    # the epilogue reads the residual and the gate rows 8 bytes per lane
    ("res_plus4", 16, 16, 64, dict(epilogue=3, residual=4, ldr=16), -2),
    ("res_plus8_small", 16, 16, 64, dict(epilogue=3, residual=8, ldr=16), 0),
    ("gate_table_plus4", 16, 16, 64, dict(epilogue=3, residual=0, ldr=16, gate_table=4, gate_temb=0, gate_ld=16), -2),
    ("gate_temb_plus4", 16, 16, 64, dict(epilogue=3, residual=0, ldr=16, gate_table=0, gate_temb=4, gate_ld=16), -2),
    ("gate_temb_plus8", 16, 16, 64, dict(epilogue=3, residual=0, ldr=16, gate_table=8, gate_temb=8, gate_ld=16), 0),
    ("rowsumsq_with_gelu", 2048, 4096, 128, dict(epilogue=1, rowsumsq=0, rowsumsq_cols=64, rowsumsq_ld=1), -2),
    ("rowsumsq_cols_mod64", 2048, 4096, 128, dict(rowsumsq=0, rowsumsq_cols=96, rowsumsq_ld=2), -1),
    ("rowsumsq_192", 2048, 4096, 128, dict(rowsumsq=0, rowsumsq_cols=192, rowsumsq_ld=6), 2),
    ("a_kblock_not_dividing", 2048, 4096, 256, dict(a_kblock=192, a_kblock_stride=2048 * 192, lda=192), -1),
    # the product's own launches (14976 = 3 x 4992 tokens): QKV, FF1, FF2, to_out on the K-blocked receive buffer of the
    # Ulysses return exchange (2 and 8 ranks), and the stacked text K/V projection (3 x 256 text rows, 28 layers' [to_k; to_v])
    ("qkv", 14976, 6144, 2048, {}, 2),
    ("ff1", 14976, 8192, 2048, dict(epilogue=1), 2),
    ("ff2", 14976, 2048, 8192, dict(epilogue=3, residual=0, ldr=2048, gate_table=0, gate_temb=0, gate_ld=12288,
                                    rows_per_group=4992), 2),
    ("to_out_kblocked_2", 14976, 2048, 2048, dict(epilogue=3, residual=0, ldr=2048, gate_table=0, gate_temb=0, gate_ld=12288,
                                                  rows_per_group=4992, lda=1024, a_kblock=1024,
                                                  a_kblock_stride=14976 * 1024), 2),
    ("to_out_kblocked_8", 1872, 2048, 2048, dict(epilogue=3, residual=0, ldr=2048, lda=256, a_kblock=256,
                                                 a_kblock_stride=1872 * 256), 0),
    ("text_kv_stacked", 768, 114688, 2048, {}, 2),
    ("text_kv_one_prompt", 256, 114688, 2048, {}, 0),
    ("adaln_table", 3, 12288, 2048, {}, 0),
]


def _gemm_geometry(M, N, K, over):
    """A ltxmi_gemm_args of that geometry on fake addresses (nothing is dereferenced): pointer-valued overrides are byte
    offsets from a 64-byte aligned base."""
    from ltxmi import _lib
    a = _lib.GemmArgs()
    base = 1 << 30
    a.A = a.W = a.C = base
    a.M, a.N, a.K = M, N, K
    a.lda = a.ldw = K
    a.ldc = N
    a.rows_per_group = 1
    for k, v in over.items():
        setattr(a, k, base + v if k in ("A", "W", "C", "bias", "residual", "gate_table", "gate_temb", "rowsumsq") else v)
    return a


@pytest.mark.parametrize("case", GEMM_KERNEL_IDS, ids=lambda c: c[0])
def test_gemm_kernel_id_table(case):
    from ltxmi import _lib
    what, M, N, K, over, want = case
    a = _gemm_geometry(M, N, K, over)
    got = _lib.lib.ltxmi_gemm_kernel_id(ctypes.byref(a))
    assert got == want, (what, got, _lib.lib.ltxmi_last_error())
    if want < 0:
        assert _lib.lib.ltxmi_last_error()
        # the launch refuses the same arguments with the same status, before it needs a device
        assert _lib.lib.ltxmi_gemm_bf16(ctypes.byref(a), None) == want


def test_gemm_kernel_id_through_ops_needs_no_device():
    """ops.gemm_kernel_id builds the struct ops.gemm builds: host tensors give the geometry (never touched)."""
    import torch
    from ltxmi import ops
    a, w = torch.empty(5000, 192, dtype=torch.bfloat16), torch.empty(4104, 192, dtype=torch.bfloat16)
    assert ops.gemm_kernel_id(a, w) == ops.GEMM_PERSISTENT256 == 2
    assert ops.gemm_kernel_id(a, w, algo=256) == ops.GEMM_TILE256 == 1
    assert ops.gemm_kernel_id(a, w, algo=128) == ops.GEMM_TILE128 == 0
    assert ops.gemm_kernel_id(a[:767], w) == 0
    res = torch.empty(5000, 4108, dtype=torch.bfloat16)
    assert ops.gemm_kernel_id(a, w, epilogue=ops.EPI_GATE_RESIDUAL, residual=res[:, :4104]) == 1
    out = torch.empty(5000, 4112, dtype=torch.bfloat16)
    assert ops.gemm_kernel_id(a, w, out=out[:, :4104], epilogue=ops.EPI_GATE_RESIDUAL, residual=out[:, :4104]) == 2
    blocked = torch.empty(3, 5000, 64, dtype=torch.bfloat16)
    assert ops.gemm_kernel_id(blocked[0], w, a_kblock=64, a_kblock_stride=5000 * 64) == 2
    assert ops.gemm_kernel_id(a, w, algo=7) == -1
    with pytest.raises(TypeError):
        ops.gemm_kernel_id(a.float(), w)


# ltxmi_conv3d_route: (what, overrides of the struct built by _conv_geometry, status or (route, epilogue, ksplit, swap_hw,
# finalize_blocks)).  Routes: 0 / 1 the implicit GEMM with 128 / 256 tiles, 2 / 3 the eight- / four-wave direct convolution.
# Worked out by hand from include/ltxmi.h and conv3d_plan's comments (direct tiles are 2 x 8 x 16 positions x 128 channels).
CONV_ROUTES = [
    ("24576 x 256: 192 direct tiles -> eight waves", {}, (2, 0, 1, 0, 0)),
    ("... + add", dict(add=True), (2, 1, 1, 0, 0)),
    ("algo 1: 96 tiles of 256 -> the 128 tile", dict(algo=1), (0, 0, 1, 0, 0)),
    ("algo 3: four waves whatever the grid", dict(algo=3), (3, 0, 1, 0, 0)),
    ("algo 3, Cout 264: not whole 128-blocks -> eight waves", dict(algo=3, Cout=264), (2, 0, 1, 0, 0)),
    ("T 24: 768 tiles -> four waves by shape", dict(T=24), (3, 0, 1, 0, 0)),
    ("T 24, algo 4", dict(T=24, algo=4), (2, 0, 1, 0, 0)),
    ("T 3: 128 tiles -> still eight waves", dict(T=3), (2, 0, 1, 0, 0)),
    ("T 2: 64 tiles -> the implicit GEMM", dict(T=2), (0, 0, 1, 0, 0)),
    ("M 49149 x 264, algo 1: 384 tiles of 256", dict(T=3, H=129, W=127, Cout=264, algo=1), (1, 0, 1, 0, 0)),
    ("M 48896 x 264, algo 1: 382 tiles of 256", dict(T=2, H=191, W=128, Cout=264, algo=1), (0, 0, 1, 0, 0)),
    ("strided: never direct", dict(stride_t=2, stride_hw=2), (0, 0, 1, 0, 0)),
    ("strided, algo 2: refused", dict(stride_hw=2, algo=2), -2),
    ("kernel_t 1", dict(kernel_t=1), (0, 0, 1, 0, 0)),
    ("no bias: never direct", dict(bias=False), (0, 0, 1, 0, 0)),
    ("depth-to-space off 1024 channels", dict(d2s=True, Cout=320), (0, 2, 1, 0, 0)),
    ("depth-to-space at 1024 channels", dict(d2s=True, Cout=1024, residual=True), (3, 2, 1, 0, 0)),
    ("depth-to-space + add", dict(d2s=True, Cout=1024, add=True), -1),
    ("post_norm, Cout 128, four waves", dict(T=48, Cout=128, post_norm=1), (3, 3, 1, 0, 0)),
    ("post_norm where no wave holds a position", dict(post_norm=1), -2),
    ("y_norm + add, Cout 128", dict(T=48, Cout=128, post_norm=1, add=True, y_norm=True), (3, 4, 1, 0, 0)),
    ("y_norm without post_norm", dict(y_norm=True), -1),
    ("1024 -> 1024 at 13 x 16 x 24 with a workspace: three ranges, rows along H",
     dict(T=13, H=16, W=24, Cin=1024, Cout=1024, workspace=3 * 4992 * 1024 * 4), (3, 6, 3, 1, 4)),
    ("... a workspace 16 bytes short: unsplit", dict(T=13, H=16, W=24, Cin=1024, Cout=1024, workspace=3 * 4992 * 1024 * 4 - 16),
     (2, 0, 1, 0, 0)),
    ("... workspace_bytes without a workspace", dict(workspace_bytes_only=64), -1),
    ("Cin 96", dict(Cin=96), -2), ("Cout 12", dict(Cout=12), -2), ("algo 5", dict(algo=5), -1), ("stride 3", dict(stride_t=3), -2),
    ("misaligned x", dict(x_off=8), -2), ("NULL y", dict(y=False), -1), ("T 0", dict(T=0), -1),
]


def _conv_geometry(over):
    from ltxmi import _lib
    over = dict(over)
    a = _lib.Conv3dArgs()
    a.x, a.w, a.y, a.bias = 4096 + over.pop("x_off", 0), 8192, (12288 if over.pop("y", True) else None), \
        (16384 if over.pop("bias", True) else None)
    a.B, a.T, a.H, a.W, a.Cin, a.Cout, a.causal, a.pad_replicate = 1, 6, 64, 64, 64, 256, 1, 1
    for k in ("add", "y_norm", "residual"):
        if over.pop(k, False):
            setattr(a, k, 20480)
    if a.residual:
        a.res_channels = 64
    if "workspace" in over:
        a.workspace, a.workspace_bytes = 24576, over.pop("workspace")
    a.workspace_bytes = over.pop("workspace_bytes_only", a.workspace_bytes)
    for k, v in over.items():
        setattr(a, k, int(v))
    return a


@pytest.mark.parametrize("case", CONV_ROUTES, ids=lambda c: c[0])
def test_conv3d_route_table(case):
    """The route query reports the launch's own decision, and refuses what the launch refuses with the same status -- both
    before anything needs a device."""
    from ltxmi import _lib
    what, over, want = case
    a = _conv_geometry(over)
    info = _lib.Conv3dRouteInfo(9, 9, 9, 9, 9)
    got = _lib.lib.ltxmi_conv3d_route(ctypes.byref(a), ctypes.byref(info))
    fields = (info.route, info.epilogue, info.ksplit, info.swap_hw, info.finalize_blocks)
    if isinstance(want, int):
        assert got == want and fields == (-1, 0, 0, 0, 0), (what, got, fields, _lib.lib.ltxmi_last_error())
        assert _lib.lib.ltxmi_last_error()
        assert _lib.lib.ltxmi_conv3d_ndhwc_bf16(ctypes.byref(a), None) == want
    else:
        assert got == 0 and fields == want, (what, got, fields, _lib.lib.ltxmi_last_error())
    assert _lib.lib.ltxmi_conv3d_route(ctypes.byref(a), None) == -1


def test_conv3d_route_through_ops_needs_no_device():
    """ops.conv3d_route builds the struct ops.conv3d builds: host tensors give the geometry (never touched)."""
    import torch
    from ltxmi import ops
    bf = torch.bfloat16
    x, w, b = torch.empty(1, 13, 16, 24, 1024, dtype=bf), torch.empty(1024, 27 * 1024, dtype=bf), torch.empty(1024, dtype=bf)
    split = dict(route=ops.CONV_DIRECT4, epilogue=6, ksplit=3, swap_hw=1, finalize_blocks=4, second_launch=False)
    assert ops.conv3d_route(x, w, b, True, True) == split                      # with the workspace ops.conv3d would hand over
    assert ops.conv3d_route(x, w, b, True, True, post_norm=(None, None, 1e-8)) == split
    none = torch.empty(0, dtype=torch.uint8)
    assert ops.conv3d_route(x, w, b, True, True, workspace=none) == dict(split, route=ops.CONV_DIRECT8, epilogue=0, ksplit=1,
                                                                        swap_hw=0, finalize_blocks=0)
    # unsplit, no kernel takes the norm along at this width: ops.conv3d launches it after the convolution
    assert ops.conv3d_route(x, w, b, True, True, workspace=none, post_norm=(None, None, 1e-8))["second_launch"]
    assert ops.conv3d_route(x, w, b, True, True, algo=1)["route"] == ops.CONV_GEMM128
    assert ops.conv3d_route(x, w, b, True, True, stride=(2, 2, 2), algo=2) == -2
    with pytest.raises(TypeError):
        ops.conv3d_route(x.float(), w, b, True, True)


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
