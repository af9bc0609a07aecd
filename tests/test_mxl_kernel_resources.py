"""Register allocation of the two-pair MX-FP8 GEMM behind include/ltxmi_mx_lora.h (CPU: hipcc cross-compiles for gfx950).  Its
instances are those of the one-pair kernel (tests/test_mx8_kernel_resources.py, tests/test_mxa_kernel_resources.py) with the
sources addressed through buffer descriptors: each sits at 256 VGPRs with the occupancy of its one-pair twin, what it spills is
pinned at what the build that introduced it gave, and its K loop holds the 16 MFMAs of a K-tile, one barrier and no scratch
access.  Resource remarks and loop structure only."""
import os
import re
import subprocess

from test_kernel_resources import CSRC, FLAGS, _pinned, _usage
from test_mx8_kernel_resources import GEMM_PINS
from test_mxa_kernel_resources import RSS_PIN

# <EPI, MXOUT, RSS> -> (VGPRs spilled, SGPRs spilled, scratch bytes per lane, waves per SIMD).  EPI 0 plain, 1 GELU, 3 gate +
# residual, 5 residual; MXOUT b1 = the e4m3 + scales output; RSS b1 = the row sums of squares
PAIR2_PINS = {'Li0ELb1ELb0E': (3, 0, 16, 2), 'Li1ELb1ELb0E': (3, 0, 16, 2), 'Li0ELb0ELb0E': (2, 0, 12, 2), 'Li1ELb0ELb0E': (2, 0, 12, 2),
              'Li3ELb0ELb0E': (42, 0, 164, 2), 'Li5ELb0ELb0E': (2, 0, 12, 2), 'Li0ELb0ELb1E': (3, 0, 16, 2)}
# the one-pair twin of each instance
TWINS = {k: GEMM_PINS[k[:-len('Lb0E')]] for k in PAIR2_PINS if k.endswith('Lb0E')}
TWINS['Li0ELb0ELb1E'] = RSS_PIN


def test_pair2_instances_keep_their_registers_and_their_twins_occupancy(tmp_path):
    usage = _usage("gemm_mx8_pair2.hip", tmp_path, extra=[])
    _pinned(usage, PAIR2_PINS, "gemm_mx8_pair2_kernel")
    for name, u in usage.items():
        assert u["VGPRs"] == 256 and u["AGPRs"] == 0, (name, u)
    assert set(TWINS) == set(PAIR2_PINS)
    for inst, pin in PAIR2_PINS.items():
        assert pin[3] == TWINS[inst][3] == 2, (inst, pin, TWINS[inst])
        assert pin[0] <= TWINS[inst][0] and pin[1] <= TWINS[inst][1], ("spills more than its one-pair twin", inst, pin, TWINS[inst])


def test_pair2_k_loop_is_a_k_tile_without_scratch_traffic(tmp_path):
    """Every instance: between the K loop's header and its back-edge there are the 16 MFMAs of a K-tile, one barrier and no
    scratch access."""
    asm = tmp_path / "gemm_mx8_pair2.s"
    flags = [f for f in FLAGS if not f.startswith("-Rpass") and f != "-c"]
    out = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-S", os.path.join(CSRC, "gemm_mx8_pair2.hip"), "-o", str(asm)],
                         capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = re.findall(r"^(_ZN5ltxmi21gemm_mx8_pair2_kernel\w+):[^\n]*\n(.*?)s_endpgm", asm.read_text(), re.S | re.M)
    assert len(kernels) == len(PAIR2_PINS)
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
