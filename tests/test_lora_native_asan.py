"""Host code of the two-pair GEMM entries under AddressSanitizer (CPU only; the device code is not instrumented).  `make asan`
builds libltxmi_asan.so and tests/native/gemm_pair2_host_asan.cpp, a stand-alone program that walks the entry check of
ltxmi_gemm_pair2_bf16 / ltxmi_gemm_pair2_kernel_id and the launcher with NO device visible, so nothing is launched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ltx-video-gpupoor_amd", "csrc")


def test_two_pair_gemm_host_code_under_asan():
    b = subprocess.run(["make", "-j4", "asan"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([os.path.join(CSRC, "asan", "gemm_pair2_host_asan")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert " 0 unexpected" in r.stdout
    assert "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
