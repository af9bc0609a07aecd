"""The second extension header include/ltxmi_mx_attn.h on the CPU: both declarations are exported with the signatures
ltxmi/_lib_mxa.py parsed, the base ABI and the first extension are untouched, and every refusal the header documents comes back
before anything is launched (no device is visible to a CPU run; the addresses are fake and never dereferenced)."""
import ctypes

import pytest

from test_mx8_abi import BASE, GATE, INVALID, UNSUPPORTED, _gemm

RSS = BASE + (8 << 20)


def test_every_declaration_is_exported_with_the_parsed_signature():
    from ltxmi import _abi, _lib, _lib_mx, _lib_mxa
    abi = _abi.parse(open(_lib_mxa.HEADER_PATH).read(), _lib_mxa.STRUCT_NAMES, _lib_mxa.KNOWN_STRUCTS)
    assert sorted(abi.signatures) == ["ltxmi_gemm_mx8_rowsumsq", "ltxmi_norm_modulate_mx8"] == sorted(_lib_mxa.SIGNATURES)
    for n, (res, args) in abi.signatures.items():
        fn = getattr(_lib.lib, n)
        assert fn.restype is res and [a.__name__ for a in fn.argtypes] == [a.__name__ for a in args], n
    assert not abi.structs and not abi.constants
    # the struct is the first extension's own class, not a copy
    assert _lib_mxa.SIGNATURES["ltxmi_gemm_mx8_rowsumsq"][1][0]._type_ is _lib_mx.GemmMx8Args
    assert len(_lib_mxa.SIGNATURES["ltxmi_gemm_mx8_rowsumsq"][1]) == 5 and len(_lib_mxa.SIGNATURES["ltxmi_norm_modulate_mx8"][1]) == 17
    assert _lib_mxa.MXA_VERSION == "1" and _lib_mx.MX_VERSION == "1"
    assert not set(_lib_mxa.SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib_mx.SIGNATURES))
    assert _lib.lib.ltxmi_version().decode() == "ltxmi " + _lib.ABI.strings["LTXMI_VERSION"]


def test_a_struct_pointer_the_parser_was_not_told_about_is_refused():
    from ltxmi import _abi, _lib_mxa
    with pytest.raises(_abi.HeaderError, match="ltxmi_gemm_mx8_args"):
        _abi.parse(open(_lib_mxa.HEADER_PATH).read(), {})


# (what, struct overrides, (rowsumsq, cols, ld), status, a word of the message): first what ltxmi_gemm_mx8 refuses for the struct
OK3 = (RSS, 64, 1)
RSS_REFUSED = [
    ("Aq NULL", dict(Aq=None), OK3, INVALID, "NULL"), ("W_scales NULL", dict(W_scales=None), OK3, INVALID, "NULL"),
    ("no output", dict(C=None), OK3, INVALID, "exactly one"), ("M 0", dict(M=0), OK3, INVALID, "non-positive"),
    ("SILU", dict(epilogue=2), OK3, INVALID, "bad epilogue"),
    ("GATE_RESIDUAL without a residual", dict(GATE, residual=None), OK3, INVALID, "residual"),
    ("K 192", dict(K=192), OK3, UNSUPPORTED, "multiple of 128"), ("N 264", dict(N=264), OK3, UNSUPPORTED, "multiple of 32"),
    ("lda % 16", dict(lda=264), OK3, UNSUPPORTED, "16-byte"), ("lda 2^24", dict(lda=1 << 24), OK3, UNSUPPORTED, "2^31"),
    ("A_scales + 2", dict(A_scales=BASE + 2), OK3, UNSUPPORTED, "4-byte"), ("bias + 4", dict(bias=BASE + 4), OK3, UNSUPPORTED, "bias"),
    ("ldc < N", dict(ldc=256), OK3, UNSUPPORTED, "8-byte"), ("C of 2^32 bytes", dict(M=4096, ldc=1 << 19), OK3, UNSUPPORTED, "2^32"),
    # then its own
    ("rowsumsq NULL", {}, (None, 64, 1), INVALID, "NULL rowsumsq"),
    ("GELU", dict(epilogue=1), OK3, INVALID, "epilogue NONE"), ("GATE_RESIDUAL", dict(GATE), OK3, INVALID, "epilogue NONE"),
    ("Cq set", dict(C=None, Cq=BASE + (5 << 20), ldcq=288, C_scales=BASE + (6 << 20), ldc_s=9), OK3, INVALID, "Cq set"),
    ("cols 0", {}, (RSS, 0, 1), INVALID, "rowsumsq_cols"), ("cols -64", {}, (RSS, -64, 1), INVALID, "rowsumsq_cols"),
    ("cols % 64", {}, (RSS, 96, 2), INVALID, "rowsumsq_cols"), ("cols > N", {}, (RSS, 320, 5), INVALID, "rowsumsq_cols"),
    ("ld < cols / 64", {}, (RSS, 256, 3), INVALID, "rowsumsq_ld"),
    ("rowsumsq + 2", {}, (RSS + 2, 64, 1), UNSUPPORTED, "4-byte aligned"),
    ("sums of 2^32 bytes", {}, (RSS, 64, 1 << 22), UNSUPPORTED, "2^32"),
]


@pytest.mark.parametrize("case", RSS_REFUSED, ids=lambda c: c[0])
def test_gemm_mx8_rowsumsq_refuses(case):
    from ltxmi import _lib
    what, over, (rss, cols, ld), status, word = case
    assert _lib.lib.ltxmi_gemm_mx8_rowsumsq(ctypes.byref(_gemm(False, **over)), rss, cols, ld, None) == status, _lib.lib.ltxmi_last_error()
    assert word.encode() in _lib.lib.ltxmi_last_error()


def _norm(**over):
    a = dict(x=BASE, ldx=64, q=BASE + (1 << 20), ldq=64, scales=BASE + (2 << 20), lds=2, rows=4, D=64, eps=1e-6, kind=0,
             scale_table=BASE + (3 << 20), scale_temb=BASE + (4 << 20), shift_table=BASE + (5 << 20), shift_temb=BASE + (6 << 20),
             temb_ld=384, rows_per_group=1)
    a.update(over)
    return tuple(a.values())


NORM_REFUSED = [
    # what ltxmi_norm_modulate_bf16 refuses for the shared arguments
    ("x NULL", dict(x=None), INVALID, "NULL"), ("scale_table NULL", dict(scale_table=None), INVALID, "NULL"),
    ("scale_temb NULL", dict(scale_temb=None), INVALID, "NULL"), ("shift_table NULL", dict(shift_table=None), INVALID, "NULL"),
    ("shift_temb NULL", dict(shift_temb=None), INVALID, "NULL"),
    ("rows 0", dict(rows=0), INVALID, "non-positive"), ("D -32", dict(D=-32), INVALID, "non-positive"),
    ("rows_per_group 0", dict(rows_per_group=0), INVALID, "non-positive"),
    ("kind 2", dict(kind=2), INVALID, "bad kind"), ("kind -1", dict(kind=-1), INVALID, "bad kind"),
    ("D 8", dict(D=8), UNSUPPORTED, "multiple of 32"), ("ldx % 8", dict(ldx=68), UNSUPPORTED, "stride"),
    ("temb_ld % 8", dict(temb_ld=388), UNSUPPORTED, "stride"),
    # what ltxmi_quantize_mx8_bf16 refuses
    ("q NULL", dict(q=None), INVALID, "NULL"), ("scales NULL", dict(scales=None), INVALID, "NULL"),
    ("D 48", dict(D=48), UNSUPPORTED, "multiple of 32"), ("ldx < D", dict(ldx=56), UNSUPPORTED, "stride"),
    ("ldq % 16", dict(ldq=72), UNSUPPORTED, "stride"), ("ldq < D", dict(ldq=48), UNSUPPORTED, "stride"),
    ("lds < D / 32", dict(lds=1), UNSUPPORTED, "stride"),
    ("x + 8", dict(x=BASE + 8), UNSUPPORTED, "16-byte"), ("q + 8", dict(q=BASE + 8), UNSUPPORTED, "16-byte"),
    # its own
    ("D 8224", dict(D=8224, ldx=8224, ldq=8224, lds=257), UNSUPPORTED, "<= 8192"),
]


@pytest.mark.parametrize("case", NORM_REFUSED, ids=lambda c: c[0])
def test_norm_modulate_mx8_refuses(case):
    from ltxmi import _lib
    what, over, status, word = case
    assert _lib.lib.ltxmi_norm_modulate_mx8(*_norm(**over), None) == status, _lib.lib.ltxmi_last_error()
    assert word.encode() in _lib.lib.ltxmi_last_error()


def test_null_struct_and_accepted_calls_reach_the_launch():
    from ltxmi import _lib
    import torch
    assert _lib.lib.ltxmi_gemm_mx8_rowsumsq(None, RSS, 64, 1, None) == INVALID and b"NULL" in _lib.lib.ltxmi_last_error()
    if not torch.cuda.is_available():              # accepted arguments get as far as the launch, which has no device
        for over, rss in ((dict(), OK3), (dict(M=1), OK3), (dict(bias=None), (RSS, 192, 8)), (dict(), (RSS, 256, 4)),
                          (dict(N=256, ldc=256), (RSS, 256, 4))):                       # the last: rowsumsq_cols == N
            assert _lib.lib.ltxmi_gemm_mx8_rowsumsq(ctypes.byref(_gemm(False, **over)), *rss, None) == -3, _lib.lib.ltxmi_last_error()
        for over in (dict(), dict(kind=1), dict(rows=1), dict(D=8192, ldx=8200, ldq=8208, lds=259, temb_ld=6 * 8192),
                     dict(D=2080, ldx=2080, ldq=2080, lds=65), dict(rows_per_group=13, temb_ld=0)):
            assert _lib.lib.ltxmi_norm_modulate_mx8(*_norm(**over), None) == -3, _lib.lib.ltxmi_last_error()


def test_ops_refuse_host_tensors_and_wrong_shapes():
    import torch
    from ltxmi import ops
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.norm_modulate_mx8(x, 1e-6, ops.NORM_RMS, x[0], x, x[0], x, 1)
    q, s = torch.zeros(4, 128, dtype=torch.float8_e4m3fn), torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.gemm_mx8(q, s, q, s, rowsumsq=torch.zeros(4, 1), rowsumsq_cols=64)
