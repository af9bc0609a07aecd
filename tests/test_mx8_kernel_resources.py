"""Register allocation of the MX-FP8 kernels (CPU: hipcc cross-compiles for gfx950).  The GEMM sits at the 256-register limit of
a 512-thread workgroup by design (128 accumulators, one k-step of fragments, the next k-step's weight fragments); what it spills
is spilled in the prologue and the epilogue, and the K loop -- and the two peeled K-tiles behind it -- must stay free of scratch
traffic: a run-time condition inside the K-tile once made hipcc keep two copies of every fragment and spill 140 registers into
the loop, at no cost to any parity test."""
import os
import re
import subprocess

from test_kernel_resources import CSRC, FLAGS, _pinned, _usage

# <EPI, MXOUT> -> (VGPRs spilled, SGPRs spilled, scratch bytes per lane, waves per SIMD).  EPI 0 plain, 1 GELU, 3 gate + residual,
# 5 residual; MXOUT b1 = the e4m3 + scales output
GEMM_PINS = {'Li0ELb1E': (3, 0, 16, 2), 'Li1ELb1E': (3, 0, 16, 2), 'Li0ELb0E': (2, 0, 12, 2), 'Li1ELb0E': (2, 0, 12, 2), 'Li3ELb0E': (43, 0, 168, 2), 'Li5ELb0E': (2, 0, 12, 2)}


def test_gemm_mx8_instances_keep_their_registers_and_occupancy(tmp_path):
    usage = _usage("gemm_mx8.hip", tmp_path, extra=[])
    _pinned(usage, GEMM_PINS, "gemm_mx8_kernel")
    for name, u in usage.items():
        assert u["VGPRs"] == 256 and u["AGPRs"] == 0, (name, u)


def test_gemm_mx8_k_loop_has_no_scratch_traffic(tmp_path):
    """Every instance: between the K loop's header and its back-edge there are the 16 MFMAs of a K-tile and no scratch access."""
    asm = tmp_path / "gemm_mx8.s"
    flags = [f for f in FLAGS if not f.startswith("-Rpass") and f != "-c"]
    out = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-S", os.path.join(CSRC, "gemm_mx8.hip"), "-o", str(asm)],
                         capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = re.findall(r"^(_ZN5ltxmi15gemm_mx8_kernel\w+):[^\n]*\n(.*?)s_endpgm", asm.read_text(), re.S | re.M)
    assert len(kernels) == len(GEMM_PINS)
    for name, body in kernels:
        lines = body.splitlines()
        heads = [i for i, l in enumerate(lines) if "Inner Loop Header" in l]
        assert len(heads) == 1, (name, len(heads))
        label = re.match(r"(\.LBB\d+_\d+):", lines[heads[0]] if lines[heads[0]].startswith(".LBB") else lines[heads[0] - 1]).group(1)
        back = max(i for i, l in enumerate(lines) if re.search(r"s_c?branch\w*\s+" + re.escape(label) + r"\b", l))
        loop = lines[heads[0]:back + 1]
        assert sum("v_mfma_scale_f32_32x32x64_f8f6f4" in l for l in loop) == 16, name
        assert not [l for l in loop if "scratch_" in l], name
        assert sum("s_barrier" in l for l in loop) == 1, name


def test_quantiser_does_not_spill(tmp_path):
    usage = _usage("quant_mx8.hip", tmp_path, extra=[])
    assert len(usage) == 1
    for name, u in usage.items():
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["Occupancy [waves/SIMD]"] == 8, (name, u)
