"""Register-allocation guard for the hand-scheduled kernels (CPU: hipcc cross-compiles for gfx950 without a GPU).

The pipelined attention kernels sit at the 256-register limit by design; an innocent-looking edit around them can make hipcc
share state between the two forms of the work item and spill 150 registers into the key loop -- which costs nothing in any
parity test and doubled the launch time when it happened (round 4).  ``-Rpass-analysis=kernel-resource-usage`` reports the
spills per kernel: the normal-run instances of the self-attention kernel must stay where they were, the short-key kernel must
not spill at all."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ltx-video-gpupoor_amd", "csrc")
ATTN_EXTRA = ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans", "-fhonor-infinities"]       # the Makefile's EXTRA of the attention files
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffast-math", "-fno-finite-math-only",
         "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c"]


def _usage(source, tmp_path, extra=ATTN_EXTRA):
    out = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, os.path.join(CSRC, source), "-o", str(tmp_path / "o.o")],
                         capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    return usage


def test_self_attention_kernel_spills(tmp_path):
    usage = _usage("attention_pipe.hip", tmp_path)
    normal = {k: v for k, v in usage.items() if "attn_pipe_kernel" in k and k.endswith("Lb0EEEvNS_10AttnParamsE")}
    assert len(normal) == 2, list(usage)                       # QSCALED = true / false, FORCE_EXACT = false
    for name, u in normal.items():
        assert u["VGPRs"] == 256 and u["Occupancy [waves/SIMD]"] == 2, (name, u)
        assert u["VGPRs Spill"] <= 24, (name, u)                # 16 / 19 as measured; 150+ = the two forms share state again


def test_short_key_attention_kernel_does_not_spill(tmp_path):
    usage = _usage("attention_cross.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "attn_cross_kernel" in k}
    assert len(kernels) == 4, list(usage)
    for name, u in kernels.items():
        assert u["VGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0 and u["Occupancy [waves/SIMD]"] >= 2, (name, u)


def test_pipelined_head_dim_128_kernel_keeps_its_register_split(tmp_path):
    usage = _usage("attention_pipe128.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "attn_pipe128_kernel" in k}
    assert len(kernels) == 1, list(usage)
    for name, u in kernels.items():
        assert u["VGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0 and u["Occupancy [waves/SIMD]"] == 1, (name, u)
        assert u["AGPRs"] > 0, (name, u)                        # the hand-pinned accumulator split is in force


def test_generic_attention_kernel_does_not_spill(tmp_path):
    usage = _usage("attention.hip", tmp_path)
    # <head_dim, key bias, 32-row query blocks per wave> -> occupancy floor (waves per SIMD) per instance
    floor = {"Li64ELb0ELi1E": 3, "Li64ELb1ELi1E": 3, "Li64ELb0ELi2E": 2, "Li128ELb0ELi1E": 2, "Li128ELb1ELi1E": 2}
    kernels = {k: v for k, v in usage.items() if "attn_fwd_kernel" in k}
    assert len(kernels) == 5, list(usage)
    for name, u in kernels.items():
        inst = [f for f in floor if "attn_fwd_kernelI" + f in name]
        assert len(inst) == 1, name
        assert u["VGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["Occupancy [waves/SIMD]"] >= floor[inst[0]], (name, u)


def _pinned(usage, pins, what):
    """pins: {mangled template arguments: (VGPRs spilled, SGPRs spilled, scratch bytes per lane, waves per SIMD)}"""
    kernels = {k: v for k, v in usage.items() if what in k}
    assert len(kernels) == len(pins), sorted(kernels)
    for inst, want in pins.items():
        name = [k for k in kernels if what + "I" + inst + "E" in k]
        assert len(name) == 1, (inst, sorted(kernels))
        u = kernels[name[0]]
        got = (u["VGPRs Spill"], u["SGPRs Spill"], u["ScratchSize [bytes/lane]"], u["Occupancy [waves/SIMD]"])
        assert got == want, (name[0], got, want)


def test_gemm_kernels_keep_their_spills_and_occupancy(tmp_path):
    """Every instance of gemm.hip where the commit that introduced csrc/epilogue.h found it (tools/codegen_diff.py against its
    parent: identical).  The persistent kernel lives with 68 .. 87 spilled VGPRs by design of its epilogue; a shared helper or an
    edit beside it that moves these figures has changed the K loop's register allocation."""
    usage = _usage("gemm.hip", tmp_path, extra=[])
    # <BM, BN, WAVES_M, WAVES_N, EPI, MODE>: EPI 0 plain, 1 GELU, 2 SiLU, 3 gate + residual, 4 depth-to-space, 5 residual, 6 row sums;
    # MODE 1 = the implicit-GEMM convolution
    tile = {"Li128ELi128ELi2ELi2ELi0ELi0E": (0, 0, 0, 3), "Li128ELi128ELi2ELi2ELi0ELi1E": (0, 0, 0, 2),
            "Li128ELi128ELi2ELi2ELi1ELi0E": (0, 0, 0, 3), "Li128ELi128ELi2ELi2ELi2ELi0E": (0, 0, 0, 3),
            "Li128ELi128ELi2ELi2ELi3ELi0E": (0, 0, 0, 2), "Li128ELi128ELi2ELi2ELi4ELi1E": (0, 0, 0, 2),
            "Li128ELi128ELi2ELi2ELi5ELi0E": (0, 0, 0, 2), "Li128ELi128ELi2ELi2ELi5ELi1E": (0, 0, 0, 2),
            "Li128ELi128ELi2ELi2ELi6ELi0E": (0, 0, 0, 3),
            "Li256ELi256ELi2ELi4ELi0ELi0E": (0, 0, 0, 2), "Li256ELi256ELi2ELi4ELi0ELi1E": (6, 0, 28, 2),
            "Li256ELi256ELi2ELi4ELi1ELi0E": (0, 0, 0, 2), "Li256ELi256ELi2ELi4ELi2ELi0E": (0, 0, 0, 2),
            "Li256ELi256ELi2ELi4ELi3ELi0E": (0, 0, 0, 2), "Li256ELi256ELi2ELi4ELi4ELi1E": (6, 0, 28, 2),
            "Li256ELi256ELi2ELi4ELi5ELi0E": (0, 0, 0, 2), "Li256ELi256ELi2ELi4ELi5ELi1E": (6, 0, 28, 2),
            "Li256ELi256ELi2ELi4ELi6ELi0E": (0, 0, 0, 2)}
    _pinned(usage, tile, "gemm_bf16_nt_kernel")
    # <BM, BN, WAVES_M, WAVES_N, EPI>
    persistent = {"Li256ELi256ELi2ELi4ELi1E": (68, 15, 248, 2), "Li256ELi256ELi2ELi4ELi2E": (68, 13, 248, 2),
                  "Li256ELi256ELi2ELi4ELi3E": (87, 29, 276, 2), "Li256ELi256ELi2ELi4ELi5E": (84, 17, 256, 2),
                  "Li256ELi256ELi2ELi4ELi6E": (77, 21, 248, 2)}
    _pinned(usage, persistent, "gemm_bf16_nt_persistent_kernel")


def test_direct_convolution_kernels_do_not_spill(tmp_path):
    """Every instance of conv_direct.hip as the same commit found it: no spill, no scratch; two workgroups of the four-wave form
    (and two waves per SIMD of the eight-wave form) stay resident."""
    usage = _usage("conv_direct.hip", tmp_path, extra=[])
    _pinned(usage, {"Li%dE" % e: (0, 0, 0, 2) for e in range(3)}, "conv3d_direct_kernel")                 # <EPI>, eight waves
    _pinned(usage, {"Li%dE" % e: (0, 0, 0, 2) for e in range(7)}, "conv3d_direct_v3_kernel")              # <EPI>, four waves
    _pinned(usage, {"Li4ELi128E": (0, 0, 0, 8), "Li4ELi256E": (0, 0, 0, 8), "Li8ELi256E": (0, 0, 0, 8), "Li12ELi256E": (0, 0, 0, 8),
                    "Li16ELi256E": (0, 0, 0, 8)}, "conv_split_finalize_kernel")                             # <CPT, NT>


def _no_spill_and_occupancy(usage, pins):
    """pins: {kernel name: {mangled template arguments ("" = not a template): waves per SIMD}}, every instance of the file:
    none spills a VGPR or an SGPR, none has scratch, each keeps its occupancy."""
    assert len(usage) == sum(len(v) for v in pins.values()), sorted(usage)
    for kernel, insts in pins.items():
        for inst, occupancy in insts.items():
            tag = "%d%s%s" % (len(kernel), kernel, "I" + inst + "E" if inst else "")
            name = [k for k in usage if tag in k]
            assert len(name) == 1, (kernel, inst, sorted(usage))
            u = usage[name[0]]
            got = (u["VGPRs Spill"], u["SGPRs Spill"], u["ScratchSize [bytes/lane]"], u["Occupancy [waves/SIMD]"])
            assert got == (0, 0, 0, occupancy), (name[0], got, occupancy)


def test_row_kernels_do_not_spill_and_keep_their_occupancy(tmp_path):
    """Every instance of rowops.hip (22), stream32.hip (14) and t5.hip (11) where the commit that introduced csrc/rows.h found it
    (tools/codegen_diff.py --sequence against its parent: identical).  They are HBM-bound one-wave-per-row passes that hold a
    row in registers: a spill puts the row into scratch, and occupancy is what hides their load latency.  <NCH> = 16-byte chunks
    per lane; the NCH = 16 two-row qkv_norm_rope_pack_kernel sits at one wave per SIMD (256 VGPRs and AGPRs) by design."""
    nch = lambda o1, o4, o16: {"Li1E": o1, "Li4E": o4, "Li16E": o16}
    _no_spill_and_occupancy(_usage("rowops.hip", tmp_path, extra=[]), {
        # <NCH, LAYER>
        "norm_modulate_kernel": {"Li1ELb0E": 8, "Li1ELb1E": 8, "Li4ELb0E": 7, "Li4ELb1E": 6, "Li16ELb0E": 2, "Li16ELb1E": 2},
        "rmsnorm_rope_kernel": nch(8, 8, 2),
        "pixelnorm_ada_silu_kernel": nch(8, 8, 3),
        "pixelnorm_ada_silu_narrow_kernel": {"Li8E": 8, "Li16E": 8, "Li32E": 8},                           # <lanes per row>
        "layernorm_affine_kernel": nch(8, 8, 2),
        "qkv_norm_rope_pack_kernel": nch(8, 4, 1),
        "rowsumsq_rstd_kernel": {"": 8}})
    _no_spill_and_occupancy(_usage("stream32.hip", tmp_path, extra=[]), {
        # <NCH, LAYER>
        "norm_modulate_f32in_kernel": {"Li1ELb0E": 8, "Li1ELb1E": 8, "Li4ELb0E": 7, "Li4ELb1E": 7, "Li8ELb0E": 4, "Li8ELb1E": 4,
                                       "Li16ELb0E": 2, "Li16ELb1E": 2},
        # <GATED, ROUND, COPY>
        "gate_residual_f32_kernel": {"Lb0ELb0ELb0E": 8, "Lb0ELb0ELb1E": 8, "Lb1ELb0ELb0E": 8, "Lb1ELb0ELb1E": 8, "Lb1ELb1ELb0E": 8,
                                     "Lb1ELb1ELb1E": 8}})
    _no_spill_and_occupancy(_usage("t5.hip", tmp_path, extra=[]), {
        "rmsnorm_weight_kernel": {"Li1E": 8, "Li4E": 8, "Li8E": 5, "Li16E": 2},                            # <NCH>
        "attn_relbias_kernel": {"Li1E": 8, "Li2E": 8, "Li4E": 6, "Li8E": 4, "Li16E": 2},                   # <key steps of 32>
        "gated_gelu_kernel": {"": 8}, "embedding_kernel": {"": 8}})
