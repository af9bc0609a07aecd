"""ctypes binding of the third extension header include/ltxmi_mx_t5.h (what the MX-FP8 T5 encoder adds), read from it at import
as ltxmi/_lib_mxa.py reads include/ltxmi_mx_attn.h: the same parser (ltxmi/_abi.py), the same library object.  The header declares
no struct of its own; its prototypes point to ``ltxmi_gemm_mx8_args`` of ltxmi_mx.h, which the parser is told about.
"""
import os

from . import _abi, _lib, _lib_mx

HEADER_PATH = os.path.join(os.path.dirname(_lib.HEADER_PATH), "ltxmi_mx_t5.h")
STRUCT_NAMES = {}
KNOWN_STRUCTS = {"ltxmi_gemm_mx8_args": _lib_mx.GemmMx8Args}

if not os.path.exists(HEADER_PATH):
    raise ImportError(f"ltxmi: {HEADER_PATH} is missing -- the MX-FP8 T5 binding is read from it. There is no fallback path.")
with open(HEADER_PATH) as _f:
    ABI = _abi.parse(_f.read(), STRUCT_NAMES, KNOWN_STRUCTS)
lib = _lib.lib
for _name, (_res, _args) in ABI.signatures.items():
    _fn = getattr(lib, _name)          # AttributeError if a declared symbol is not exported
    _fn.restype = _res
    _fn.argtypes = _args
SIGNATURES = ABI.signatures
CONSTANTS = ABI.constants
MXT_VERSION = ABI.strings["LTXMI_MXT_VERSION"]
FORM_AUTO, FORM_128X64, FORM_64X64 = (CONSTANTS["LTXMI_MXT_FORM_" + n] for n in ("AUTO", "128X64", "64X64"))
FORMS = (FORM_128X64, FORM_64X64)
STAGES = CONSTANTS["LTXMI_MXT_STAGES"]
MAX_ROWS = CONSTANTS["LTXMI_MXT_MAX_ROWS"]
check = _lib.check
