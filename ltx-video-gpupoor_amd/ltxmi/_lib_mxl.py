"""ctypes binding of the fourth extension header include/ltxmi_mx_lora.h (LoRA adapters applied unmerged on MX-FP8 linears), read
from it at import as ltxmi/_lib_mx.py reads include/ltxmi_mx.h: the same parser (ltxmi/_abi.py), the same library object.  The
header declares the second operand pair's struct; its prototype also points to ``ltxmi_gemm_mx8_args`` of ltxmi_mx.h, which the
parser is told about.
"""
import os

from . import _abi, _lib, _lib_mx

HEADER_PATH = os.path.join(os.path.dirname(_lib.HEADER_PATH), "ltxmi_mx_lora.h")
STRUCT_NAMES = {"ltxmi_gemm_mx8_pair": "GemmMx8Pair"}
KNOWN_STRUCTS = {"ltxmi_gemm_mx8_args": _lib_mx.GemmMx8Args}

if not os.path.exists(HEADER_PATH):
    raise ImportError(f"ltxmi: {HEADER_PATH} is missing -- the MX-FP8 LoRA binding is read from it. There is no fallback path.")
with open(HEADER_PATH) as _f:
    ABI = _abi.parse(_f.read(), STRUCT_NAMES, KNOWN_STRUCTS)
lib = _lib.lib
for _name, (_res, _args) in ABI.signatures.items():
    _fn = getattr(lib, _name)          # AttributeError if a declared symbol is not exported
    _fn.restype = _res
    _fn.argtypes = _args
globals().update(ABI.structs)          # GemmMx8Pair
SIGNATURES = ABI.signatures
CONSTANTS = ABI.constants
MXL_VERSION = ABI.strings["LTXMI_MXL_VERSION"]
check = _lib.check
