"""The third extension header include/ltxmi_mx_t5.h on the CPU: every declaration is exported with the signature ltxmi/_lib_mxt.py
parsed, the base ABI and the two earlier extensions are untouched, and every refusal the header documents comes back before
anything is launched (no device is visible to a CPU run; the addresses are fake and never dereferenced)."""
import ctypes

import pytest

from test_mx8_abi import BASE, GATE, INVALID, UNSUPPORTED, _gemm

NAMES = ["ltxmi_gated_gelu_mx8", "ltxmi_gemm_mx8_skinny", "ltxmi_gemm_mx8_skinny_form", "ltxmi_rmsnorm_weight_mx8"]


def test_every_declaration_is_exported_with_the_parsed_signature():
    from ltxmi import _abi, _lib, _lib_mx, _lib_mxa, _lib_mxt
    abi = _abi.parse(open(_lib_mxt.HEADER_PATH).read(), _lib_mxt.STRUCT_NAMES, _lib_mxt.KNOWN_STRUCTS)
    assert sorted(abi.signatures) == NAMES == sorted(_lib_mxt.SIGNATURES)
    for n, (res, args) in abi.signatures.items():
        fn = getattr(_lib.lib, n)
        assert fn.restype is res and [a.__name__ for a in fn.argtypes] == [a.__name__ for a in args], n
    assert not abi.structs
    assert abi.constants == dict(LTXMI_MXT_FORM_AUTO=0, LTXMI_MXT_FORM_128X64=1, LTXMI_MXT_FORM_64X64=2,
                                 LTXMI_MXT_STAGES=_lib_mxt.STAGES, LTXMI_MXT_MAX_ROWS=512)
    assert 3 <= _lib_mxt.STAGES <= 6 and _lib_mxt.FORMS == (1, 2)
    # the struct is the first extension's own class, not a copy
    for n in ("ltxmi_gemm_mx8_skinny", "ltxmi_gemm_mx8_skinny_form"):
        assert _lib_mxt.SIGNATURES[n][1][0]._type_ is _lib_mx.GemmMx8Args
    assert [len(_lib_mxt.SIGNATURES[n][1]) for n in NAMES] == [9, 3, 2, 11]
    assert _lib_mxt.MXT_VERSION == "1" and _lib_mxa.MXA_VERSION == "1" and _lib_mx.MX_VERSION == "1"
    assert not set(_lib_mxt.SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib_mx.SIGNATURES) | set(_lib_mxa.SIGNATURES))
    assert _lib.lib.ltxmi_version().decode() == "ltxmi " + _lib.ABI.strings["LTXMI_VERSION"]


def test_a_struct_pointer_the_parser_was_not_told_about_is_refused():
    from ltxmi import _abi, _lib_mxt
    with pytest.raises(_abi.HeaderError, match="ltxmi_gemm_mx8_args"):
        _abi.parse(open(_lib_mxt.HEADER_PATH).read(), {})


# (what, struct overrides, form, status, a word of the message): first what ltxmi_gemm_mx8 refuses for the struct
NOBIAS = dict(bias=None)
SKINNY_REFUSED = [
    ("Aq NULL", dict(Aq=None), 0, INVALID, "NULL"), ("W_scales NULL", dict(W_scales=None), 0, INVALID, "NULL"),
    ("no output", dict(C=None), 0, INVALID, "exactly one"), ("M 0", dict(M=0), 0, INVALID, "non-positive"),
    ("SILU", dict(epilogue=2), 0, INVALID, "bad epilogue"),
    ("GATE_RESIDUAL without a residual", dict(GATE, residual=None, **NOBIAS), 0, INVALID, "residual"),
    ("K 192", dict(K=192), 0, UNSUPPORTED, "multiple of 128"), ("N 264", dict(N=264), 0, UNSUPPORTED, "multiple of 32"),
    ("lda % 16", dict(lda=264), 0, UNSUPPORTED, "16-byte"), ("A_scales + 2", dict(A_scales=BASE + 2), 0, UNSUPPORTED, "4-byte"),
    ("bias + 4", dict(bias=BASE + 4), 0, UNSUPPORTED, "bias"), ("ldc < N", dict(ldc=256), 0, UNSUPPORTED, "8-byte"),
    # then its own
    ("Cq set", dict(C=None, Cq=BASE + (5 << 20), ldcq=288, C_scales=BASE + (6 << 20), ldc_s=9), 0, UNSUPPORTED, "bf16 output only"),
    ("GELU", dict(epilogue=1), 0, UNSUPPORTED, "epilogue 1"),
    ("a gate table", dict(GATE, gate_table=BASE, gate_temb=BASE, rows_per_group=1, **NOBIAS), 0, UNSUPPORTED, "gate_table"),
    ("bias with GATE_RESIDUAL", dict(GATE), 0, UNSUPPORTED, "bias together with GATE_RESIDUAL"),
    ("M 513", dict(M=513), 0, UNSUPPORTED, "row limit"), ("M 513, forced", dict(M=513), 2, UNSUPPORTED, "row limit"),
    ("form 3", {}, 3, UNSUPPORTED, "names no tile form"), ("form -1", {}, -1, UNSUPPORTED, "names no tile form"),
]


@pytest.mark.parametrize("case", SKINNY_REFUSED, ids=lambda c: c[0])
def test_gemm_mx8_skinny_and_its_plan_refuse(case):
    from ltxmi import _lib
    what, over, form, status, word = case
    for call in (lambda a: _lib.lib.ltxmi_gemm_mx8_skinny(ctypes.byref(a), form, None),
                 lambda a: _lib.lib.ltxmi_gemm_mx8_skinny_form(ctypes.byref(a), form)):
        assert call(_gemm(False, **over)) == status, _lib.lib.ltxmi_last_error()
        assert word.encode() in _lib.lib.ltxmi_last_error()


def _norm(**over):
    a = dict(x=BASE, ldx=64, q=BASE + (1 << 20), ldq=64, scales=BASE + (2 << 20), lds=2, rows=4, D=64, weight=BASE + (3 << 20), eps=1e-6)
    a.update(over)
    return tuple(a.values())


NORM_REFUSED = [
    ("x NULL", dict(x=None), INVALID, "NULL"), ("q NULL", dict(q=None), INVALID, "NULL"), ("scales NULL", dict(scales=None), INVALID, "NULL"),
    ("weight NULL", dict(weight=None), INVALID, "NULL"), ("rows 0", dict(rows=0), INVALID, "non-positive"),
    ("D -32", dict(D=-32), INVALID, "non-positive"),
    ("D 8", dict(D=8), UNSUPPORTED, "multiple of 32"), ("D 48", dict(D=48), UNSUPPORTED, "multiple of 32"),
    ("D 1000", dict(D=1000, ldx=1000, ldq=1008, lds=32), UNSUPPORTED, "multiple of 32"),
    ("D 8224", dict(D=8224, ldx=8224, ldq=8224, lds=257), UNSUPPORTED, "<= 8192"),
    ("ldx % 8", dict(ldx=68), UNSUPPORTED, "stride"), ("ldx < D", dict(ldx=56), UNSUPPORTED, "stride"),
    ("ldq % 16", dict(ldq=72), UNSUPPORTED, "stride"), ("ldq < D", dict(ldq=48), UNSUPPORTED, "stride"),
    ("lds < D / 32", dict(lds=1), UNSUPPORTED, "stride"),
    ("x + 8", dict(x=BASE + 8), UNSUPPORTED, "16-byte"), ("q + 8", dict(q=BASE + 8), UNSUPPORTED, "16-byte"),
    ("weight + 8", dict(weight=BASE + 8), UNSUPPORTED, "16-byte"),
]


@pytest.mark.parametrize("case", NORM_REFUSED, ids=lambda c: c[0])
def test_rmsnorm_weight_mx8_refuses(case):
    from ltxmi import _lib
    what, over, status, word = case
    assert _lib.lib.ltxmi_rmsnorm_weight_mx8(*_norm(**over), None) == status, _lib.lib.ltxmi_last_error()
    assert word.encode() in _lib.lib.ltxmi_last_error()


def _gelu(**over):
    a = dict(h=BASE, ldh=128, q=BASE + (1 << 20), ldq=64, scales=BASE + (2 << 20), lds=2, rows=4, F=64)
    a.update(over)
    return tuple(a.values())


GELU_REFUSED = [
    ("h NULL", dict(h=None), INVALID, "NULL"), ("q NULL", dict(q=None), INVALID, "NULL"), ("scales NULL", dict(scales=None), INVALID, "NULL"),
    ("rows 0", dict(rows=0), INVALID, "non-positive"), ("F 0", dict(F=0), INVALID, "non-positive"),
    ("F 8", dict(F=8), UNSUPPORTED, "multiple of 32"), ("F 1000", dict(F=1000, ldh=2000, ldq=1008, lds=32), UNSUPPORTED, "multiple of 32"),
    ("ldh < 2 F", dict(ldh=120), UNSUPPORTED, "stride"), ("ldh % 8", dict(ldh=132), UNSUPPORTED, "stride"),
    ("ldq % 16", dict(ldq=72), UNSUPPORTED, "stride"), ("ldq < F", dict(ldq=48), UNSUPPORTED, "stride"),
    ("lds < F / 32", dict(lds=1), UNSUPPORTED, "stride"),
    ("h + 8", dict(h=BASE + 8), UNSUPPORTED, "16-byte"), ("q + 8", dict(q=BASE + 8), UNSUPPORTED, "16-byte"),
]


@pytest.mark.parametrize("case", GELU_REFUSED, ids=lambda c: c[0])
def test_gated_gelu_mx8_refuses(case):
    from ltxmi import _lib
    what, over, status, word = case
    assert _lib.lib.ltxmi_gated_gelu_mx8(*_gelu(**over), None) == status, _lib.lib.ltxmi_last_error()
    assert word.encode() in _lib.lib.ltxmi_last_error()


def test_null_struct_and_accepted_calls_reach_the_launch():
    from ltxmi import _lib
    import torch
    assert _lib.lib.ltxmi_gemm_mx8_skinny(None, 0, None) == INVALID and b"NULL" in _lib.lib.ltxmi_last_error()
    assert _lib.lib.ltxmi_gemm_mx8_skinny_form(None, 0) == INVALID and b"NULL" in _lib.lib.ltxmi_last_error()
    if not torch.cuda.is_available():              # accepted arguments get as far as the launch, which has no device
        for over, form in ((dict(), 0), (dict(M=1), 1), (dict(M=512, bias=None), 2), (dict(GATE, bias=None), 0),
                           (dict(GATE, bias=None, residual=BASE + (5 << 20)), 1)):          # the last: the residual is C
            assert _lib.lib.ltxmi_gemm_mx8_skinny(ctypes.byref(_gemm(False, **over)), form, None) == -3, _lib.lib.ltxmi_last_error()
        for over in (dict(), dict(rows=1), dict(D=8192, ldx=8200, ldq=8208, lds=259), dict(D=4096, ldx=4096, ldq=4096, lds=128),
                     dict(D=2080, ldx=2080, ldq=2080, lds=65)):
            assert _lib.lib.ltxmi_rmsnorm_weight_mx8(*_norm(**over), None) == -3, _lib.lib.ltxmi_last_error()
        for over in (dict(), dict(rows=1), dict(F=10240, ldh=20480, ldq=10240, lds=320), dict(rows=1 << 20, F=2080, ldh=4168, ldq=2096, lds=66)):
            assert _lib.lib.ltxmi_gated_gelu_mx8(*_gelu(**over), None) == -3, _lib.lib.ltxmi_last_error()


def test_ops_refuse_host_tensors_and_wrong_shapes():
    import torch
    from ltxmi import ops
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.rmsnorm_weight_mx8(x, x[0], 1e-6)
    with pytest.raises(TypeError):
        ops.gated_gelu_mx8(x)
    q, s = torch.zeros(4, 128, dtype=torch.float8_e4m3fn), torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.gemm_mx8_skinny(q, s, q, s)
    with pytest.raises(TypeError):
        ops.gemm_mx8_skinny_form(q, s, q, s)
