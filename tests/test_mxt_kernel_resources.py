"""Register allocation of the kernels behind include/ltxmi_mx_t5.h (CPU: hipcc cross-compiles for gfx950).  From the compiler's
resource remarks only.

The skinny GEMM counts on several workgroups per CU (two of the 128 x 64 form, three of the 64 x 64 form by their LDS): no
instance may spill, and its registers must allow that many waves.  The two fused row passes are HBM-bound like their bf16 twins of
t5.hip, whose occupancy is what hides their load latency: no instance may spill or run fewer waves per SIMD than its twin."""
import re

from test_kernel_resources import _usage

NO_SPILL = ("VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]")


def test_skinny_gemm_instances_do_not_spill(tmp_path):
    usage = _usage("gemm_mx8_skinny.hip", tmp_path, extra=[])
    kernels = {k: v for k, v in usage.items() if "gemm_mx8_skinny_kernel" in k}
    assert len(kernels) == len(usage) == 4, sorted(usage)                      # <128 | 64 rows, with | without the residual>
    for bm, resid in ((128, 0), (128, 1), (64, 0), (64, 1)):
        name = [k for k in kernels if f"gemm_mx8_skinny_kernelILi{bm}ELb{resid}EE" in k]
        assert len(name) == 1, (bm, resid, sorted(kernels))
        u = kernels[name[0]]
        assert [u[k] for k in NO_SPILL] == [0, 0, 0], (name[0], u)
        # one wave per SIMD and workgroup: the LDS allows 2 / 3 workgroups per CU, the registers must too
        assert u["Occupancy [waves/SIMD]"] >= (2 if bm == 128 else 3), (name[0], u)


def test_fused_row_passes_do_not_spill_and_keep_their_twins_occupancy(tmp_path):
    twins = _usage("t5.hip", tmp_path, extra=[])
    usage = _usage("t5_mx8.hip", tmp_path, extra=[])
    assert len(usage) == 5, sorted(usage)                                      # the norm's four chunk counts and the gated GELU
    pairs = 0
    for name, u in usage.items():
        assert [u[k] for k in NO_SPILL] == [0, 0, 0], (name, u)
        m = re.search(r"rmsnorm_weight_mx8_kernelILi(\d+)E", name)
        twin = [k for k in twins if (f"rmsnorm_weight_kernelILi{m.group(1)}E" in k if m else "gated_gelu_kernel" in k)]
        assert len(twin) == 1 and ("gated_gelu_mx8_kernel" in name or m), (name, sorted(twins))
        assert u["Occupancy [waves/SIMD]"] >= twins[twin[0]]["Occupancy [waves/SIMD]"], (name, u, twins[twin[0]])
        pairs += 1
    assert pairs == 5
