"""ctypes binding of the extension header include/ltxmi_mx.h (the MX-FP8 entries), read from it at import as ltxmi/_lib.py reads
include/ltxmi.h: the same parser (ltxmi/_abi.py), the same library object.  include/ltxmi.h and ``_lib.SIGNATURES`` stay the
frozen base ABI; what this header declares is bound here and listed in ``SIGNATURES`` / ``CONSTANTS`` of this module.
"""
import os

from . import _abi, _lib

HEADER_PATH = os.path.join(os.path.dirname(_lib.HEADER_PATH), "ltxmi_mx.h")
STRUCT_NAMES = {"ltxmi_gemm_mx8_args": "GemmMx8Args"}

if not os.path.exists(HEADER_PATH):
    raise ImportError(f"ltxmi: {HEADER_PATH} is missing -- the MX-FP8 binding is read from it. There is no fallback path.")
with open(HEADER_PATH) as _f:
    ABI = _abi.parse(_f.read(), STRUCT_NAMES)
lib = _lib.lib
for _name, (_res, _args) in ABI.signatures.items():
    _fn = getattr(lib, _name)          # AttributeError if a declared symbol is not exported
    _fn.restype = _res
    _fn.argtypes = _args
globals().update(ABI.structs)          # GemmMx8Args
SIGNATURES = ABI.signatures
CONSTANTS = ABI.constants
MX_VERSION = ABI.strings["LTXMI_MX_VERSION"]
MX_BLOCK = CONSTANTS["LTXMI_MX_BLOCK"]
check = _lib.check
