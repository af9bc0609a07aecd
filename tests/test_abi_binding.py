"""The ctypes binding is read from include/ltxmi.h (ltxmi/_abi.py, ltxmi/_lib.py).  Four checks hold it, all on the CPU:
the compiler's own reading of the header (tests/native/abi_layout.cpp: every size, offset and constant), the pin of the
ABI as the hand-written tables of 0.9 had it (tests/golden/abi_0_9.json), what the parser refuses, and the version test
between header and library."""
import ctypes
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ltx-video-gpupoor_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_0_9.json")

STRUCTS = ("GemmArgs", "GemmPair", "AttnArgs", "AttnRelBiasArgs", "AttnMergeArgs", "Conv3dArgs", "Conv3dRouteInfo")
OPS_CONSTANTS = ("EPI_NONE", "EPI_GELU_TANH", "EPI_SILU", "EPI_GATE_RESIDUAL", "NORM_RMS", "NORM_LAYER",
                 "PAD_ZEROS", "PAD_REPLICATE", "PAD_REFLECT",
                 "GEMM_TILE128", "GEMM_TILE256", "GEMM_PERSISTENT256", "GEMM_PAIR2_TILE128", "GEMM_PAIR2_TILE256",
                 "CONV_GEMM128", "CONV_GEMM256", "CONV_DIRECT8", "CONV_DIRECT4", "GUIDANCE_WORKSPACE_FLOATS")


def abi_dump(_lib, ops):
    """The binding as data: per struct its size and (field, ctypes type name, offset) in order, per function the restype's and
    the argtypes' names, and the constants under their Python names.  tests/golden/abi_0_9.json is this dump of the last
    hand-written tables."""
    structs = {}
    for name in STRUCTS:
        cls = getattr(_lib, name)
        structs[name] = dict(size=ctypes.sizeof(cls), fields=[[n, t.__name__, getattr(cls, n).offset] for n, t in cls._fields_])
    functions = {n: dict(restype=res.__name__, argtypes=[a.__name__ for a in args])
                 for n, (res, args) in sorted(_lib.SIGNATURES.items())}
    constants = {n: getattr(ops, n) for n in OPS_CONSTANTS}
    constants["ATTN_MERGE_MAX"] = _lib.ATTN_MERGE_MAX
    return dict(structs=structs, functions=functions, constants=constants)


# ------------------------------------------------------------------ 1. the compiler's reading of the header
@pytest.fixture(scope="module")
def layout():
    b = subprocess.run(["make", "abi_layout"], cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([os.path.join(CSRC, "abi_layout")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_every_struct_field_and_constant_is_where_the_compiler_puts_it(layout):
    from ltxmi import _lib
    assert set(layout["structs"]) == set(_lib.STRUCT_NAMES)                # the program lists every struct of the header ...
    fields = 0
    for c_name, want in layout["structs"].items():
        cls = getattr(_lib, _lib.STRUCT_NAMES[c_name])
        assert ctypes.sizeof(cls) == want["size"], c_name
        assert [n for n, _ in cls._fields_] == list(want["fields"]), c_name  # ... and every field, in order
        for n, (offset, size) in want["fields"].items():
            f = getattr(cls, n)
            assert (f.offset, f.size) == (offset, size), (c_name, n)
            fields += 1
    assert len(layout["structs"]) == 7 and fields >= 120
    assert layout["constants"] == _lib.CONSTANTS                            # every enum constant and integer #define
    assert layout["version"] == _lib.ABI.strings["LTXMI_VERSION"]


def test_ops_constants_are_the_headers(layout):
    from ltxmi import _lib, ops
    c = layout["constants"]
    for n in OPS_CONSTANTS:
        assert getattr(ops, n) == c["LTXMI_" + n], n
    assert _lib.ATTN_MERGE_MAX == c["LTXMI_ATTN_MERGE_MAX"] == 8
    assert (ops.BLEND_F32, ops.BLEND_BF16, ops.BLEND_F16) == (c["LTXMI_BLEND_F32"], c["LTXMI_BLEND_BF16"], c["LTXMI_BLEND_F16"])
    assert (ops.BLEND_F32, ops.BLEND_BF16, ops.BLEND_F16) == (0, 1, 2)     # the codes ltxmi_tile_blend has always taken


# ------------------------------------------------------------------ 2. the ABI is the one of the hand-written tables
def test_binding_equals_the_pinned_abi():
    """A pull request that changes the ABI changes tests/golden/abi_0_9.json, and says so."""
    from ltxmi import _lib, ops
    want = json.load(open(GOLDEN))
    got = abi_dump(_lib, ops)
    assert got["structs"] == want["structs"]
    assert got["functions"] == want["functions"]
    assert got["constants"] == want["constants"]
    assert len(want["functions"]) == 47 and len(want["structs"]) == 7


# ------------------------------------------------------------------ 3. what the parser takes and what it refuses
NAMES = {"ltxmi_t": "T", "ltxmi_u": "U"}
ACCEPTED = """
/* every accepted form; a comment with ; and ( in it */
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define LTXMI_N 3   /* an array length; ( */
#define LTXMI_VERSION "1.2.3"
typedef enum ltxmi_e { LTXMI_A = 0, LTXMI_B = -2,  /* ; */
                       LTXMI_C = 7 } ltxmi_e;
typedef struct ltxmi_t {
    const void* a; int64_t b;      /* two declarations on a line; int x; */
    int32_t M, N, K;
    const float* p[LTXMI_N]; int64_t s[LTXMI_N], t[2];
    uint32_t* counter; float f; int i;
} ltxmi_t;
typedef struct ltxmi_u { int32_t r; } ltxmi_u;
const char* ltxmi_name(void);
int64_t ltxmi_bytes(const ltxmi_t* args);
int ltxmi_call(const ltxmi_t* args, ltxmi_u* out, const float* x, int64_t ldx,
               int32_t rows, float eps, const int64_t* ids,
               int32_t, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_every_accepted_form():
    from ltxmi import _abi
    c = ctypes
    abi = _abi.parse(ACCEPTED, NAMES)
    T, U = abi.structs["T"], abi.structs["U"]
    assert T.__name__ == "T" and list(abi.structs) == ["T", "U"]
    assert T._fields_ == [("a", c.c_void_p), ("b", c.c_int64), ("M", c.c_int32), ("N", c.c_int32), ("K", c.c_int32),
                          ("p", c.c_void_p * 3), ("s", c.c_int64 * 3), ("t", c.c_int64 * 2),
                          ("counter", c.c_void_p), ("f", c.c_float), ("i", c.c_int32)]
    assert abi.constants == dict(LTXMI_N=3, LTXMI_A=0, LTXMI_B=-2, LTXMI_C=7)
    assert abi.strings == dict(LTXMI_VERSION="1.2.3")
    assert abi.signatures == {
        "ltxmi_name": (c.c_char_p, []),
        "ltxmi_bytes": (c.c_int64, [c.POINTER(T)]),
        "ltxmi_call": (c.c_int32, [c.POINTER(T), c.POINTER(U), c.c_void_p, c.c_int64, c.c_int32, c.c_float, c.c_void_p,
                                  c.c_int32, c.c_void_p])}


REFUSED = [
    ("unknown scalar type", "typedef struct ltxmi_t { double x; } ltxmi_t;", "double"),
    ("unknown pointee", "typedef struct ltxmi_t { const short* x; } ltxmi_t;", "short"),
    ("unsigned scalar", "typedef struct ltxmi_t { uint32_t x; } ltxmi_t;", "uint32_t"),
    ("two-word type", "typedef struct ltxmi_t { unsigned int x; } ltxmi_t;", "unsigned int x"),
    ("pointer to pointer", "typedef struct ltxmi_t { void** x; } ltxmi_t;", "** x"),
    ("array length that is no define", "typedef struct ltxmi_t { int32_t x[LTXMI_M]; } ltxmi_t;", "LTXMI_M"),
    ("array length defined as a string", '#define LTXMI_M "3"\ntypedef struct ltxmi_t { int32_t x[LTXMI_M]; } ltxmi_t;', "LTXMI_M"),
    ("a define that is no integer literal", "#define LTXMI_M (1 + 2)\n", "LTXMI_M"),
    ("a function-like macro", "#define LTXMI_F(x) x\n", "LTXMI_F"),
    ("struct without a Python name", "typedef struct ltxmi_v { int32_t x; } ltxmi_v;", "ltxmi_v"),
    ("nested struct", "typedef struct ltxmi_t { struct { int32_t x; } in; } ltxmi_t;", "ltxmi_t"),
    ("bit-field", "typedef struct ltxmi_t { int32_t x : 3; } ltxmi_t;", "x : 3"),
    ("function pointer field", "typedef struct ltxmi_t { int (*cb)(int); } ltxmi_t;", "cb"),
    ("function pointer parameter", "int ltxmi_f(int (*cb)(int));", "ltxmi_f"),
    ("unnamed parameter of unknown type", "int ltxmi_f(int32_t, foo_t);", "foo_t"),
    ("named parameter of unknown type", "int ltxmi_f(size_t n);", "size_t"),
    ("struct passed by value", "typedef struct ltxmi_t { int32_t x; } ltxmi_t;\nint ltxmi_f(ltxmi_t a);", "ltxmi_t"),
    ("pointer to a struct declared nowhere", "int ltxmi_f(const ltxmi_t* a);", "ltxmi_t"),
    ("unknown return type", "double ltxmi_f(void);", "double"),
    ("char* parameter", "int ltxmi_f(const char* s);", "char"),
    ("enum constant without a value", "typedef enum ltxmi_e { LTXMI_A, LTXMI_B = 1 } ltxmi_e;", "LTXMI_A"),
    ("a plain typedef", "typedef int ltxmi_int;", "typedef int ltxmi_int"),
    ("a global", "extern int ltxmi_flag;", "ltxmi_flag"),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c[0])
def test_parser_refuses_what_is_outside_the_subset(case):
    from ltxmi import _abi
    what, text, word = case
    with pytest.raises(_abi.HeaderError) as e:
        _abi.parse(text, NAMES)
    assert word in str(e.value), str(e.value)                              # the message shows the offending declaration


# ------------------------------------------------------------------ 4. header and library are one version
def test_real_header_and_library_load_and_a_foreign_version_is_refused():
    from ltxmi import _lib
    header = open(_lib.HEADER_PATH).read()
    abi, lib = _lib._load(header)
    version = abi.strings["LTXMI_VERSION"]
    assert lib.ltxmi_version().decode() == "ltxmi " + version == "ltxmi 0.9.0"
    assert set(abi.signatures) == set(_lib.SIGNATURES)
    assert f'#define LTXMI_VERSION "{version}"' in header
    with pytest.raises(ImportError) as e:
        _lib._load(header.replace(f'#define LTXMI_VERSION "{version}"', '#define LTXMI_VERSION "0.9.1"'))
    assert "ltxmi 0.9.1" in str(e.value) and "ltxmi 0.9.0" in str(e.value)
    with pytest.raises(ImportError):                                        # a header without the define says nothing: refused
        _lib._load(header.replace("#define LTXMI_VERSION", "#define LTXMI_VERSION_"))
