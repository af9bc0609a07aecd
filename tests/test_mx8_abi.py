"""The extension header include/ltxmi_mx.h on the CPU: every declaration is exported with the signature ltxmi/_lib_mx.py parsed,
the struct is where the compiler puts it (tests/native/mx8_layout.cpp, the pattern of abi_layout), the base ABI is untouched,
and every refusal the header documents comes back before anything is launched (no device is visible to a CPU run)."""
import ctypes
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ltx-video-gpupoor_amd", "csrc")
INVALID, UNSUPPORTED = -1, -2
BASE = 1 << 30                                      # fake, 64-byte aligned addresses: nothing is dereferenced


def test_every_declaration_is_exported_with_the_parsed_signature():
    from ltxmi import _abi, _lib, _lib_mx
    abi = _abi.parse(open(_lib_mx.HEADER_PATH).read(), _lib_mx.STRUCT_NAMES)
    assert sorted(abi.signatures) == ["ltxmi_gemm_mx8", "ltxmi_quantize_mx8_bf16"] == sorted(_lib_mx.SIGNATURES)
    for n, (res, args) in abi.signatures.items():
        fn = getattr(_lib.lib, n)
        assert fn.restype is res and [a.__name__ for a in fn.argtypes] == [a.__name__ for a in args], n
    assert _lib_mx.SIGNATURES["ltxmi_gemm_mx8"][1][0]._type_ is _lib_mx.GemmMx8Args
    assert _lib_mx.MX_VERSION == "1" and _lib_mx.MX_BLOCK == 32
    # the base ABI does not know them, and the library's version is the base header's
    assert not set(_lib_mx.SIGNATURES) & set(_lib.SIGNATURES)
    assert _lib.lib.ltxmi_version().decode() == "ltxmi " + _lib.ABI.strings["LTXMI_VERSION"]


def test_struct_is_where_the_compiler_puts_it():
    from ltxmi import _lib_mx
    b = subprocess.run(["make", "mx8_layout"], cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([os.path.join(CSRC, "mx8_layout")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    layout = json.loads(r.stdout)
    assert set(layout["structs"]) == set(_lib_mx.STRUCT_NAMES)
    want = layout["structs"]["ltxmi_gemm_mx8_args"]
    cls = _lib_mx.GemmMx8Args
    assert ctypes.sizeof(cls) == want["size"]
    assert [n for n, _ in cls._fields_] == list(want["fields"])
    for n, (offset, size) in want["fields"].items():
        assert (getattr(cls, n).offset, getattr(cls, n).size) == (offset, size), n
    assert layout["constants"] == _lib_mx.CONSTANTS and layout["version"] == _lib_mx.MX_VERSION


def _gemm(mx=False, **over):
    from ltxmi import _lib_mx
    a = _lib_mx.GemmMx8Args()
    M, N, K = 300, 288, 256
    a.Aq, a.lda, a.A_scales, a.lda_s = BASE, K, BASE + (1 << 20), K // 32
    a.Wq, a.ldw, a.W_scales, a.ldw_s = BASE + (2 << 20), K, BASE + (3 << 20), K // 32
    a.bias = BASE + (4 << 20)
    if mx:
        a.Cq, a.ldcq, a.C_scales, a.ldc_s = BASE + (5 << 20), N, BASE + (6 << 20), N // 32
    else:
        a.C, a.ldc = BASE + (5 << 20), N
    a.M, a.N, a.K = M, N, K
    for k, v in over.items():
        setattr(a, k, v)
    return a


GATE = dict(epilogue=3, residual=BASE + (7 << 20), ldr=288)
GEMM_REFUSED = [
    ("Aq NULL", False, dict(Aq=None), INVALID, "NULL"), ("A_scales NULL", False, dict(A_scales=None), INVALID, "NULL"),
    ("Wq NULL", False, dict(Wq=None), INVALID, "NULL"), ("W_scales NULL", False, dict(W_scales=None), INVALID, "NULL"),
    ("no output", False, dict(C=None), INVALID, "exactly one"), ("both outputs", True, dict(C=BASE), INVALID, "exactly one"),
    ("Cq without C_scales", True, dict(C_scales=None), INVALID, "C_scales"),
    ("M 0", False, dict(M=0), INVALID, "non-positive"), ("N -32", False, dict(N=-32), INVALID, "non-positive"),
    ("K 0", False, dict(K=0), INVALID, "non-positive"),
    ("SILU", False, dict(epilogue=2), INVALID, "bad epilogue"), ("epilogue 4", False, dict(epilogue=4), INVALID, "bad epilogue"),
    ("GATE_RESIDUAL with Cq", True, dict(GATE), INVALID, "MX output"),
    ("no residual", False, dict(GATE, residual=None), INVALID, "residual"), ("ldr < N", False, dict(GATE, ldr=280), INVALID, "residual"),
    ("ldr % 4", False, dict(GATE, ldr=290), INVALID, "residual"),
    ("gate_table alone", False, dict(GATE, gate_table=BASE), INVALID, "gate_temb"),
    ("rows_per_group 0", False, dict(GATE, gate_table=BASE, gate_temb=BASE, rows_per_group=0), INVALID, "rows_per_group"),
    ("gate_ld % 4", False, dict(GATE, gate_table=BASE, gate_temb=BASE, rows_per_group=1, gate_ld=6), INVALID, "gate_temb"),
    ("K 192", False, dict(K=192), UNSUPPORTED, "multiple of 128"), ("K 64", False, dict(K=64), UNSUPPORTED, "multiple of 128"),
    ("N 264", False, dict(N=264), UNSUPPORTED, "multiple of 32"), ("N 8", False, dict(N=8), UNSUPPORTED, "multiple of 32"),
    ("lda % 16", False, dict(lda=264), UNSUPPORTED, "16-byte"), ("ldw < K", False, dict(ldw=128), UNSUPPORTED, "16-byte"),
    ("Aq + 8", False, dict(Aq=BASE + 8), UNSUPPORTED, "16-byte"), ("Wq + 4", False, dict(Wq=BASE + 4), UNSUPPORTED, "16-byte"),
    ("lda 2^24", False, dict(lda=1 << 24), UNSUPPORTED, "2^31"),
    ("lda_s % 4", False, dict(lda_s=10), UNSUPPORTED, "4-byte"), ("ldw_s < K / 32", False, dict(ldw_s=4), UNSUPPORTED, "4-byte"),
    ("A_scales + 2", False, dict(A_scales=BASE + 2), UNSUPPORTED, "4-byte"),
    ("bias + 4", False, dict(bias=BASE + 4), UNSUPPORTED, "bias"),
    ("C + 4", False, dict(C=BASE + 4), UNSUPPORTED, "8-byte"), ("ldc % 4", False, dict(ldc=290), UNSUPPORTED, "8-byte"),
    ("ldc < N", False, dict(ldc=256), UNSUPPORTED, "8-byte"),
    ("Cq + 2", True, dict(Cq=BASE + 2), UNSUPPORTED, "Cq"), ("ldcq % 4", True, dict(ldcq=290), UNSUPPORTED, "Cq"),
    ("ldc_s < N / 32", True, dict(ldc_s=8), UNSUPPORTED, "Cq"),
    ("C of 2^32 bytes", False, dict(M=4096, ldc=1 << 19), UNSUPPORTED, "2^32"), ("Cq of 2^32 bytes", True, dict(M=8192, ldcq=1 << 19), UNSUPPORTED, "2^32"),
    ("C_scales of 2^32 bytes", True, dict(M=8192, ldc_s=1 << 19), UNSUPPORTED, "2^32"),
    ("residual + 4", False, dict(GATE, residual=BASE + 4), UNSUPPORTED, "8-byte aligned"),
    ("gate_temb + 2", False, dict(GATE, gate_table=BASE, gate_temb=BASE + 2, rows_per_group=1), UNSUPPORTED, "8-byte aligned"),
]


@pytest.mark.parametrize("case", GEMM_REFUSED, ids=lambda c: c[0])
def test_gemm_mx8_refuses(case):
    from ltxmi import _lib
    what, mx, over, status, word = case
    assert _lib.lib.ltxmi_gemm_mx8(ctypes.byref(_gemm(mx, **over)), None) == status, _lib.lib.ltxmi_last_error()
    assert word.encode() in _lib.lib.ltxmi_last_error()


def test_gemm_mx8_null_struct_and_accepted_calls_reach_the_launch():
    from ltxmi import _lib
    import torch
    assert _lib.lib.ltxmi_gemm_mx8(None, None) == INVALID and b"NULL" in _lib.lib.ltxmi_last_error()
    if not torch.cuda.is_available():              # accepted arguments get as far as the launch, which has no device
        for a in (_gemm(), _gemm(True), _gemm(epilogue=1), _gemm(True, epilogue=1), _gemm(**GATE), _gemm(M=1), _gemm(bias=None)):
            assert _lib.lib.ltxmi_gemm_mx8(ctypes.byref(a), None) == -3, _lib.lib.ltxmi_last_error()


QUANT_REFUSED = [
    ((None, 64, BASE, 64, BASE, 2, 4, 64), INVALID, "NULL"), ((BASE, 64, None, 64, BASE, 2, 4, 64), INVALID, "NULL"),
    ((BASE, 64, BASE, 64, None, 2, 4, 64), INVALID, "NULL"),
    ((BASE, 64, BASE, 64, BASE, 2, 0, 64), INVALID, "non-positive"), ((BASE, 64, BASE, 64, BASE, 2, 4, -32), INVALID, "non-positive"),
    ((BASE, 64, BASE, 64, BASE, 2, 4, 48), UNSUPPORTED, "multiple of 32"), ((BASE, 40, BASE, 64, BASE, 2, 4, 40), UNSUPPORTED, "multiple of 32"),
    ((BASE, 56, BASE, 64, BASE, 2, 4, 64), UNSUPPORTED, "stride"), ((BASE, 68, BASE, 64, BASE, 2, 4, 64), UNSUPPORTED, "stride"),
    ((BASE, 64, BASE, 72, BASE, 2, 4, 64), UNSUPPORTED, "stride"), ((BASE, 64, BASE, 48, BASE, 2, 4, 64), UNSUPPORTED, "stride"),
    ((BASE, 64, BASE, 64, BASE, 1, 4, 64), UNSUPPORTED, "stride"),
    ((BASE + 8, 64, BASE, 64, BASE, 2, 4, 64), UNSUPPORTED, "16-byte"), ((BASE, 64, BASE + 8, 64, BASE, 2, 4, 64), UNSUPPORTED, "16-byte"),
]


@pytest.mark.parametrize("case", QUANT_REFUSED, ids=lambda c: f"{c[2]}-{c[1]}-{c[0][1:4]}-{c[0][5:]}")
def test_quantize_mx8_refuses(case):
    from ltxmi import _lib
    args, status, word = case
    assert _lib.lib.ltxmi_quantize_mx8_bf16(*args, None) == status, _lib.lib.ltxmi_last_error()
    assert word.encode() in _lib.lib.ltxmi_last_error()


def test_ops_refuse_host_tensors_and_wrong_dtypes():
    import torch
    from ltxmi import mx8, ops
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.quantize_mx8(x)
    q, s = torch.zeros(4, 128, dtype=torch.float8_e4m3fn), torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.gemm_mx8(q, s, q, s)
    with pytest.raises(ValueError):
        mx8.dequantize(q, s[:, :3])
    assert mx8.dequantize(q.view(torch.uint8), s).shape == (4, 128)
    v = torch.tensor([[1.5] * 32]).to(torch.float8_e4m3fn)
    assert mx8.dequantize(v, torch.tensor([[130]], dtype=torch.uint8)).tolist() == [[12.0] * 32]
