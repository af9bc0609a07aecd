"""The fourth extension header include/ltxmi_mx_lora.h on the CPU: its one declaration is exported with the signature
ltxmi/_lib_mxl.py parsed, the other headers are untouched, and every refusal the header documents comes back before anything is
launched (no device is visible to a CPU run; the addresses are fake and never dereferenced).  ``ops.gemm_mx8`` takes device
tensors only, so "a refused call through it raises and leaves a sentinel-filled output as it was" is held on the device, by
tests/test_gpu_mxl_kernels.py::test_a_refused_call_raises_and_writes_nothing; here are the refusals ops makes before any tensor
is looked at."""
import ctypes

import pytest

from test_mx8_abi import BASE, GATE, INVALID, UNSUPPORTED, _gemm

RSS = BASE + (8 << 20)
NO_RSS, OK3 = (None, 0, 0), (RSS, 64, 1)


def _pair(**over):
    from ltxmi import _lib_mxl
    p = _lib_mxl.GemmMx8Pair()
    p.A2q, p.lda2, p.A2_scales, p.lda2_s = BASE + (9 << 20), 128, BASE + (10 << 20), 4
    p.W2q, p.ldw2, p.W2_scales, p.ldw2_s = BASE + (11 << 20), 128, BASE + (12 << 20), 4
    p.K2, p.group_cols = 128, 0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _call(args, pair, rss=NO_RSS):
    from ltxmi import _lib
    return _lib.lib.ltxmi_gemm_mx8_pair2(ctypes.byref(args) if args is not None else None,
                                         ctypes.byref(pair) if pair is not None else None, *rss, None)


def test_the_declaration_is_exported_with_the_parsed_signature():
    from ltxmi import _abi, _lib, _lib_mx, _lib_mxa, _lib_mxl, _lib_mxt
    abi = _abi.parse(open(_lib_mxl.HEADER_PATH).read(), _lib_mxl.STRUCT_NAMES, _lib_mxl.KNOWN_STRUCTS)
    assert sorted(abi.signatures) == ["ltxmi_gemm_mx8_pair2"] == sorted(_lib_mxl.SIGNATURES)
    res, args = abi.signatures["ltxmi_gemm_mx8_pair2"]
    fn = _lib.lib.ltxmi_gemm_mx8_pair2
    assert fn.restype is res and [a.__name__ for a in fn.argtypes] == [a.__name__ for a in args]
    assert sorted(abi.structs) == ["GemmMx8Pair"] and not abi.constants
    sig = _lib_mxl.SIGNATURES["ltxmi_gemm_mx8_pair2"][1]
    assert len(sig) == 6 and sig[0]._type_ is _lib_mx.GemmMx8Args and sig[1]._type_ is _lib_mxl.GemmMx8Pair
    assert [f[0] for f in _lib_mxl.GemmMx8Pair._fields_] == ["A2q", "lda2", "A2_scales", "lda2_s", "W2q", "ldw2", "W2_scales", "ldw2_s",
                                                             "K2", "group_cols"]
    assert ctypes.sizeof(_lib_mxl.GemmMx8Pair) == 72
    assert _lib_mxl.MXL_VERSION == "1" and _lib_mxa.MXA_VERSION == "1" and _lib_mx.MX_VERSION == "1"
    others = set(_lib.SIGNATURES) | set(_lib_mx.SIGNATURES) | set(_lib_mxa.SIGNATURES) | set(_lib_mxt.SIGNATURES)
    assert not set(_lib_mxl.SIGNATURES) & others
    assert _lib.lib.ltxmi_version().decode() == "ltxmi " + _lib.ABI.strings["LTXMI_VERSION"]


def test_a_struct_pointer_the_parser_was_not_told_about_is_refused():
    from ltxmi import _abi, _lib_mxl
    with pytest.raises(_abi.HeaderError, match="ltxmi_gemm_mx8_args"):
        _abi.parse(open(_lib_mxl.HEADER_PATH).read(), _lib_mxl.STRUCT_NAMES)


MXO = dict(C=None, Cq=BASE + (5 << 20), ldcq=288, C_scales=BASE + (6 << 20), ldc_s=9)
# (what, struct overrides, pair overrides, (rowsumsq, cols, ld), status, a word of the message)
REFUSED = [
    # what ltxmi_gemm_mx8 refuses for the struct
    ("Aq NULL", dict(Aq=None), {}, NO_RSS, INVALID, "NULL"), ("no output", dict(C=None), {}, NO_RSS, INVALID, "exactly one"),
    ("M 0", dict(M=0), {}, NO_RSS, INVALID, "non-positive"), ("SILU", dict(epilogue=2), {}, NO_RSS, INVALID, "bad epilogue"),
    ("GATE_RESIDUAL with Cq", dict(MXO, **GATE), {}, NO_RSS, INVALID, "MX output"),
    ("GATE_RESIDUAL without a residual", dict(GATE, residual=None), {}, NO_RSS, INVALID, "residual"),
    ("K 192", dict(K=192), {}, NO_RSS, UNSUPPORTED, "multiple of 128"), ("N 264", dict(N=264), {}, NO_RSS, UNSUPPORTED, "multiple of 32"),
    ("lda % 16", dict(lda=264), {}, NO_RSS, UNSUPPORTED, "16-byte"), ("lda 2^24", dict(lda=1 << 24), {}, NO_RSS, UNSUPPORTED, "2^31"),
    ("A_scales + 2", dict(A_scales=BASE + 2), {}, NO_RSS, UNSUPPORTED, "4-byte"),
    ("C of 2^32 bytes", dict(M=4096, ldc=1 << 19), {}, NO_RSS, UNSUPPORTED, "2^32"),
    # what ltxmi_gemm_mx8_rowsumsq refuses, with a rowsumsq
    ("GELU with row sums", dict(epilogue=1), {}, OK3, INVALID, "epilogue NONE"), ("Cq with row sums", MXO, {}, OK3, INVALID, "Cq set"),
    ("cols 0", {}, {}, (RSS, 0, 1), INVALID, "rowsumsq_cols"), ("cols % 64", {}, {}, (RSS, 96, 2), INVALID, "rowsumsq_cols"),
    ("cols > N", {}, {}, (RSS, 320, 5), INVALID, "rowsumsq_cols"), ("ld < cols / 64", {}, {}, (RSS, 256, 3), INVALID, "rowsumsq_ld"),
    ("rowsumsq + 2", {}, {}, (RSS + 2, 64, 1), UNSUPPORTED, "4-byte aligned"),
    ("sums of 2^32 bytes", {}, {}, (RSS, 64, 1 << 22), UNSUPPORTED, "2^32"),
    # the pair's own
    ("A2q NULL", {}, dict(A2q=None), NO_RSS, INVALID, "NULL second pair"),
    ("A2_scales NULL", {}, dict(A2_scales=None), NO_RSS, INVALID, "NULL second pair"),
    ("W2q NULL", {}, dict(W2q=None), NO_RSS, INVALID, "NULL second pair"),
    ("W2_scales NULL", {}, dict(W2_scales=None), NO_RSS, INVALID, "NULL second pair"),
    ("K2 0", {}, dict(K2=0), NO_RSS, INVALID, "K2="), ("K2 -128", {}, dict(K2=-128), NO_RSS, INVALID, "K2="),
    ("K2 64", {}, dict(K2=64), NO_RSS, INVALID, "K2="), ("K2 192", {}, dict(K2=192, lda2=192, ldw2=192, lda2_s=8, ldw2_s=8), NO_RSS, INVALID, "K2="),
    ("group_cols -256", dict(N=512, ldc=512), dict(group_cols=-256), NO_RSS, INVALID, "group_cols"),
    ("group_cols 128", dict(N=512, ldc=512), dict(group_cols=128, lda2=512, lda2_s=16), NO_RSS, INVALID, "group_cols"),
    ("group_cols does not divide N", dict(N=768, ldc=768), dict(group_cols=512, lda2=256, lda2_s=8), NO_RSS, INVALID, "group_cols"),
    ("lda2 % 16", {}, dict(lda2=136), NO_RSS, UNSUPPORTED, "lda2"), ("ldw2 % 16", {}, dict(ldw2=136), NO_RSS, UNSUPPORTED, "lda2"),
    ("lda2 < K2", {}, dict(K2=256, lda2=128, ldw2=256, lda2_s=8, ldw2_s=8), NO_RSS, UNSUPPORTED, "lda2"),
    ("ldw2 < K2", {}, dict(K2=256, lda2=256, ldw2=128, lda2_s=8, ldw2_s=8), NO_RSS, UNSUPPORTED, "lda2"),
    ("lda2 < groups K2", dict(N=768, ldc=768), dict(group_cols=256, lda2=256, lda2_s=12), NO_RSS, UNSUPPORTED, "lda2"),
    ("lda2_s % 4", {}, dict(lda2_s=6), NO_RSS, UNSUPPORTED, "lda2_s"), ("ldw2_s % 4", {}, dict(ldw2_s=6), NO_RSS, UNSUPPORTED, "lda2_s"),
    ("lda2_s < K2 / 32", {}, dict(K2=256, lda2=256, ldw2=256, lda2_s=4, ldw2_s=8), NO_RSS, UNSUPPORTED, "lda2_s"),
    ("ldw2_s < K2 / 32", {}, dict(K2=256, lda2=256, ldw2=256, lda2_s=8, ldw2_s=4), NO_RSS, UNSUPPORTED, "lda2_s"),
    ("lda2_s < groups K2 / 32", dict(N=768, ldc=768), dict(group_cols=256, lda2=384, lda2_s=8), NO_RSS, UNSUPPORTED, "lda2_s"),
    ("A2q + 8", {}, dict(A2q=BASE + 8), NO_RSS, UNSUPPORTED, "16-byte"), ("W2q + 8", {}, dict(W2q=BASE + 8), NO_RSS, UNSUPPORTED, "16-byte"),
    ("A2_scales + 2", {}, dict(A2_scales=BASE + 2), NO_RSS, UNSUPPORTED, "4-byte"),
    ("W2_scales + 2", {}, dict(W2_scales=BASE + 2), NO_RSS, UNSUPPORTED, "4-byte"),
    ("lda2 2^23", {}, dict(lda2=1 << 23), NO_RSS, UNSUPPORTED, "2^31"), ("ldw2 2^23", {}, dict(ldw2=1 << 23), NO_RSS, UNSUPPORTED, "2^31"),
    ("lda2_s 2^23", {}, dict(lda2_s=1 << 23), NO_RSS, UNSUPPORTED, "2^31"), ("ldw2_s 2^23", {}, dict(ldw2_s=1 << 23), NO_RSS, UNSUPPORTED, "2^31"),
    ("lda_s 2^23", dict(lda_s=1 << 23), {}, NO_RSS, UNSUPPORTED, "2^31"), ("ldw_s 2^23", dict(ldw_s=1 << 23), {}, NO_RSS, UNSUPPORTED, "2^31"),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c[0])
def test_gemm_mx8_pair2_refuses(case):
    from ltxmi import _lib
    what, over, pover, rss, status, word = case
    assert _call(_gemm(False, **over), _pair(**pover), rss) == status, _lib.lib.ltxmi_last_error()
    assert word.encode() in _lib.lib.ltxmi_last_error(), _lib.lib.ltxmi_last_error()


def test_null_structs_and_accepted_calls_reach_the_launch():
    from ltxmi import _lib
    import torch
    assert _call(None, _pair()) == INVALID and b"NULL" in _lib.lib.ltxmi_last_error()
    assert _call(_gemm(), None) == INVALID and b"NULL second pair" in _lib.lib.ltxmi_last_error()
    if not torch.cuda.is_available():              # accepted arguments get as far as the launch, which has no device
        q3 = dict(group_cols=256, lda2=384, lda2_s=12)
        for mx, over, pover, rss in ((False, {}, {}, NO_RSS), (True, {}, {}, NO_RSS), (True, dict(epilogue=1), {}, NO_RSS),
                                     (False, dict(epilogue=1), {}, NO_RSS), (False, dict(GATE), {}, NO_RSS),
                                     (False, dict(GATE, gate_table=BASE, gate_temb=BASE, rows_per_group=7), {}, NO_RSS),
                                     (False, {}, {}, OK3), (False, dict(M=1), {}, (RSS, 256, 4)),
                                     (False, {}, {}, (None, 96, -5)),                    # without rowsumsq its arguments are ignored
                                     (False, dict(N=768, ldc=768), q3, (RSS, 256, 4)),
                                     (False, dict(N=1024, ldc=1024), dict(group_cols=512, lda2=256, lda2_s=8), NO_RSS),
                                     (False, {}, dict(K2=256, lda2=272, ldw2=256, lda2_s=12, ldw2_s=8), NO_RSS)):
            assert _call(_gemm(mx, **over), _pair(**pover), rss) == -3, _lib.lib.ltxmi_last_error()


def test_ops_refuses_half_a_pair_and_host_tensors_before_any_call():
    import torch
    from ltxmi import ops
    q, s = torch.zeros(4, 128, dtype=torch.float8_e4m3fn), torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="go together"):
        ops.gemm_mx8(q, s, q, s, a2=(q, s))
    with pytest.raises(ValueError, match="go together"):
        ops.gemm_mx8(q, s, q, s, w2=(q, s))
    with pytest.raises(TypeError):
        ops.gemm_mx8(q, s, q, s, a2=(q, s), w2=(q, s))
    w = torch.zeros(768, 128, dtype=torch.float8_e4m3fn), torch.zeros(768, 4, dtype=torch.uint8)
    for bad in (512, -256):                             # a group width that does not divide N is named before the entry sees it
        with pytest.raises(ValueError, match=f"a2_group_cols={bad}"):
            ops.gemm_mx8(q, s, *w, a2=(q, s), w2=w, a2_group_cols=bad)
