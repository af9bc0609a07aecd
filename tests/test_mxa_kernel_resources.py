"""Register allocation of the kernels behind include/ltxmi_mx_attn.h (CPU: hipcc cross-compiles for gfx950).  The row-sum GEMM is
the plain bf16-output MX-FP8 GEMM with four more accumulators in the epilogue: it gets the checks
tests/test_mx8_kernel_resources.py makes on that kernel's instances.  The fused norm + quantise kernel is an HBM-bound row pass
like norm_modulate_kernel, whose occupancy is what hides its load latency: no instance may spill or run fewer waves than the
norm_modulate_kernel instance with the same chunk count.  Resource remarks and loop structure only."""
import os
import re
import subprocess

from test_kernel_resources import CSRC, FLAGS, _usage

# (VGPRs spilled, SGPRs spilled, scratch bytes per lane, waves per SIMD), as the build that introduced the kernel gave them
RSS_PIN = (3, 0, 16, 2)
# <NCH, LAYER> -> the waves per SIMD tests/test_kernel_resources.py pins for norm_modulate_kernel<NCH, LAYER>
NORM_FLOOR = {"Li1ELb0E": 8, "Li1ELb1E": 8, "Li4ELb0E": 7, "Li4ELb1E": 6, "Li16ELb0E": 2, "Li16ELb1E": 2}


def test_rowsumsq_gemm_keeps_its_registers_and_occupancy(tmp_path):
    usage = _usage("gemm_mx8_rss.hip", tmp_path, extra=[])
    assert list(usage) == ["_ZN5ltxmi24gemm_mx8_rowsumsq_kernelENS_12Mx8RssParamsE"], sorted(usage)
    u = next(iter(usage.values()))
    assert u["VGPRs"] == 256 and u["AGPRs"] == 0, u
    got = (u["VGPRs Spill"], u["SGPRs Spill"], u["ScratchSize [bytes/lane]"], u["Occupancy [waves/SIMD]"])
    assert got == RSS_PIN, got


def test_rowsumsq_gemm_k_loop_has_no_scratch_traffic(tmp_path):
    """Between the K loop's header and its back-edge: the 16 MFMAs of a K-tile, one barrier and no scratch access."""
    asm = tmp_path / "gemm_mx8_rss.s"
    flags = [f for f in FLAGS if not f.startswith("-Rpass") and f != "-c"]
    out = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-S", os.path.join(CSRC, "gemm_mx8_rss.hip"), "-o", str(asm)],
                         capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = re.findall(r"^(_ZN5ltxmi24gemm_mx8_rowsumsq_kernel\w+):[^\n]*\n(.*?)s_endpgm", asm.read_text(), re.S | re.M)
    assert len(kernels) == 1
    name, body = kernels[0]
    lines = body.splitlines()
    heads = [i for i, l in enumerate(lines) if "Inner Loop Header" in l]
    assert len(heads) == 1, (name, len(heads))
    label = re.match(r"(\.LBB\d+_\d+):", lines[heads[0]] if lines[heads[0]].startswith(".LBB") else lines[heads[0] - 1]).group(1)
    back = max(i for i, l in enumerate(lines) if re.search(r"s_c?branch\w*\s+" + re.escape(label) + r"\b", l))
    loop = lines[heads[0]:back + 1]
    assert sum("v_mfma_scale_f32_32x32x64_f8f6f4" in l for l in loop) == 16, name
    assert not [l for l in loop if "scratch_" in l], name
    assert sum("s_barrier" in l for l in loop) == 1, name


def test_fused_norm_quantise_does_not_spill_and_keeps_the_norm_kernels_occupancy(tmp_path):
    usage = _usage("norm_mx8.hip", tmp_path, extra=[])
    assert len(usage) == len(NORM_FLOOR), sorted(usage)
    for inst, floor in NORM_FLOOR.items():
        name = [k for k in usage if "24norm_modulate_mx8_kernelI" + inst + "E" in k]
        assert len(name) == 1, (inst, sorted(usage))
        u = usage[name[0]]
        assert (u["VGPRs Spill"], u["SGPRs Spill"], u["ScratchSize [bytes/lane]"]) == (0, 0, 0), (name[0], u)
        assert u["Occupancy [waves/SIMD]"] >= floor, (name[0], u, floor)
