"""Register-allocation guard for the two-pair GEMM kernels (CPU: hipcc cross-compiles for gfx950 without a GPU), with the
flags and the parser of tests/test_kernel_resources.py.  The 256x256 form holds 128 accumulator registers and both sets of
fragments next to four per-lane operand offsets: every instance must stay free of spills and scratch with two waves per SIMD
(two workgroups of the 128x128 form per CU)."""
from test_kernel_resources import _usage


def test_two_pair_gemm_kernels_do_not_spill(tmp_path):
    usage = _usage("gemm_pair2.hip", tmp_path, extra=[])
    kernels = {k: v for k, v in usage.items() if "gemm_bf16_nt_pair2_kernel" in k}
    # <BM, BN, WAVES_M, WAVES_N, EPI>: two tile forms x EPI 0 plain, 1 GELU, 2 SiLU, 3 gate + residual, 5 residual, 6 row sums
    want = {"Li%dELi%dELi2ELi%dELi%dE" % (t, t, wn, e) for t, wn in ((128, 2), (256, 4)) for e in (0, 1, 2, 3, 5, 6)}
    assert len(kernels) == 12, sorted(usage)
    for inst in want:
        name = [k for k in kernels if "gemm_bf16_nt_pair2_kernelI" + inst + "E" in k]
        assert len(name) == 1, (inst, sorted(kernels))
        u = kernels[name[0]]
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, (name[0], u)
        assert u["Occupancy [waves/SIMD]"] >= 2, (name[0], u)
    # the names the guard of gemm.hip counts its own instances by must not match these
    assert not any("gemm_bf16_nt_kernel" in k or "gemm_bf16_nt_persistent_kernel" in k for k in usage)
