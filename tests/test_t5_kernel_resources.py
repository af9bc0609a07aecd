"""Register allocation of the T5 attention kernel (CPU: hipcc cross-compiles for gfx950).  A query's whole score row lives in
registers -- 4 per 16 keys -- so every instance must stay free of spills and scratch, at the occupancy DESIGN.md states
("T5 text encoder": 8 / 8 / 6 / 4 / 2 waves per SIMD by registers for up to 32 / 64 / 128 / 256 / 512 keys)."""
import re

from test_kernel_resources import _usage

OCCUPANCY = {1: 8, 2: 8, 4: 6, 8: 4, 16: 2}            # 32-key steps of the instance -> waves per SIMD


def test_relbias_attention_kernel_does_not_spill(tmp_path):
    usage = _usage("t5.hip", tmp_path, extra=[])
    kernels = {k: v for k, v in usage.items() if "attn_relbias_kernel" in k}
    assert len(kernels) == len(OCCUPANCY), list(usage)
    for name, u in kernels.items():
        nt = int(re.search(r"attn_relbias_kernelILi(\d+)E", name).group(1))
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["Occupancy [waves/SIMD]"] == OCCUPANCY[nt], (name, u)
    # the row kernels beside it: no scratch either
    for name, u in usage.items():
        assert u["VGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, (name, u)
