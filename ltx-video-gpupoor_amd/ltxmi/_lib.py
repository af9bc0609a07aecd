"""ctypes binding of libltxmi.so, read from include/ltxmi.h at import (ltxmi/_abi.py): nothing of the header is restated here.

The library is the ONLY compute path of this package: if it cannot be loaded the
import fails loudly -- there is no PyTorch/CPU fallback.
"""
import ctypes
import os

# torch FIRST: its wheel ships a HIP runtime of its own (torch/lib/libamdhip64.so).  Loaded before torch, libltxmi.so pulls in the
# system's /opt/rocm runtime instead, the process then holds two HIP runtimes, and the library's calls (hipGetDevice, launches on
# torch's streams) go to the one torch never initialised: "cannot query the current device" on the first kernel.  With torch's
# runtime already in the process the library's DT_NEEDED entry resolves to it.
import torch  # noqa: F401

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# LTXMI_LIB: tuning knob only (A/B runs of two builds of the SAME library); never a fallback path
LIB_PATH = os.environ.get("LTXMI_LIB") or os.path.join(_HERE, "libltxmi.so")
# the header the library was compiled against, where csrc/Makefile finds it
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "ltxmi.h"))

# every struct of the header and the name of its class here; a struct the header gains needs an entry (else the import fails)
STRUCT_NAMES = {"ltxmi_gemm_args": "GemmArgs", "ltxmi_gemm_pair": "GemmPair", "ltxmi_attn_args": "AttnArgs",
                "ltxmi_attn_merge_args": "AttnMergeArgs", "ltxmi_conv3d_args": "Conv3dArgs",
                "ltxmi_conv3d_route_info": "Conv3dRouteInfo", "ltxmi_attn_relbias_args": "AttnRelBiasArgs"}


def _load(header):
    """``header``: the text of include/ltxmi.h -> (its _abi.Abi, the library with every prototype's restype / argtypes set)."""
    abi = _abi.parse(header, STRUCT_NAMES)
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"ltxmi: {LIB_PATH} is missing -- build it with `make -C ltx-video-gpupoor_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no fallback path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in abi.signatures.items():
        fn = getattr(lib, name)      # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    want, got = f"ltxmi {abi.strings.get('LTXMI_VERSION')}", lib.ltxmi_version().decode()
    if got != want:
        raise ImportError(f"ltxmi: {LIB_PATH} is `{got}` but {HEADER_PATH} is `{want}`: the binding is read from the header, so "
                          "the two must be one version -- rebuild the library (`make -C ltx-video-gpupoor_amd/csrc`).")
    return abi, lib


if not os.path.exists(HEADER_PATH):
    raise ImportError(f"ltxmi: {HEADER_PATH} is missing -- the binding is read from it (the package runs from its source tree, "
                      "next to include/). There is no fallback path.")
with open(HEADER_PATH) as _f:
    ABI, lib = _load(_f.read())
globals().update(ABI.structs)        # GemmArgs, GemmPair, ...: the struct classes, under the names STRUCT_NAMES gives them
SIGNATURES = ABI.signatures          # name -> (restype, argtypes)
CONSTANTS = ABI.constants            # every enum constant and integer #define, by its name in the header
ATTN_MERGE_MAX = CONSTANTS["LTXMI_ATTN_MERGE_MAX"]


class LtxmiError(RuntimeError):
    pass


def check(status, what):
    if status != 0:
        raise LtxmiError(f"{what} failed ({status}): {lib.ltxmi_last_error().decode()}")
