"""The bf16 GEMM on a real MI355X, kernel by kernel: every case first asserts WHICH kernel its call takes
(ops.gemm_kernel_id: 0 the 128x128 tile kernel, 1 the non-persistent 256x256 one, 2 the persistent 256x256 one), writes its
output as a view inside a sentinel-filled buffer, and is judged against the float64 truth of tests/gemm_cases.py by that
module's three metrics (whole tensor; per row and per 256-column block; per element against the sum of magnitudes).  The
truth is computed on the device in float64 (rocBLAS, independent of this library); the cases, their input families and
the slack are defined and pinned on the CPU (tests/gemm_cases.py, tests/test_gemm_cases.py).

Paths: one / two / three tiles per persistent workgroup, the tile-count threshold from both sides, K = 64 .. 8192, minimal
and ragged shapes, every epilogue with and without a bias.  Operand forms on the persistent and on the 128x128 kernel: the
K-blocked A of the Ulysses return exchange (bit-equal to the contiguous call), gate + residual with group boundaries inside
a fragment / on tile boundaries / one group, in place and out of place, residuals the persistent kernel hands to the
non-persistent 256x256 kernel, C with ldc % 8 == 4 on an 8-byte boundary, and the row sums of squares cut inside a wave's
sub-tile.  Persistent cases run twice into fresh buffers and must give equal bits.

FINDINGS of the first run: no case failed (closest figure: per-block L2 at 0.84 of its limit, the gated epilogue on the
``large`` family).  The persistent kernel stores correctly to a C on an 8-byte boundary with ldc % 8 == 4, so the entry
check stands and the requirement line of include/ltxmi.h was corrected to it.

The closest figure per metric, as a fraction of its limit, is printed when the module is done."""
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"

_worst = {}
_cache = []          # [(key, inputs, truth, mag)], the last two: neighbouring cases share inputs and truth


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _cache.clear()
    if _worst:
        print("\ngemm paths, closest figures (fraction of the limit): " +
              "  ".join(f"{k} {v:.3f} [{w}]" for k, (v, w) in sorted(_worst.items())))
        assert all(v <= 1.0 for v, _ in _worst.values())


def _note(f, what):
    for k, v in f.items():
        if v > _worst.get(k, (-1.0, ""))[0]:
            _worst[k] = (v, what)


def _inputs(c):
    key = (c["family"], c["M"], c["N"], c["K"], c["epi"], c["bias"], c.get("rows_per_group"))
    for k, d, t, m in _cache:
        if k == key:
            return d, t, m
    del _cache[:-1]
    d = gc.make(c["family"], c["M"], c["N"], c["K"], c["epi"], c["bias"], c.get("rows_per_group"), device=DEV)
    t, m = gc.gemm_op(d, c["epi"])
    _cache.append((key, d, t, m))
    return d, t, m


def _run(c, d, a=None):
    from ltxmi import ops
    kw, out_buf, out = gc.call_args(c, d, a)
    assert ops.gemm_kernel_id(**kw) == c["id"], "the case does not reach the kernel it is about"
    ops.gemm(**kw)
    torch.cuda.synchronize()
    assert gc.sentinels_intact(out_buf, out), "wrote outside the output view"
    return out


@pytest.mark.parametrize("c", gc.GPU_CASES, ids=gc.case_id)
def test_gemm_case(c):
    what = gc.case_id(c)
    d, truth, mag = _inputs(c)
    out = _run(c, d)
    _note(gc.compare(out, truth, mag, what=what), what)
    if c["id"] == 2:
        assert torch.equal(_run(c, d), out), "two runs of the persistent kernel differ"
    if "P" in c:
        # the K-blocked operand is the same matrix: same bits as the call on the contiguous A
        assert torch.equal(gc.gather_a(gc.block_a(d["a"], c["P"])[0], c["K"], c["K"] // c["P"], c["M"] * (c["K"] // c["P"])), d["a"])
        assert torch.equal(_run(c, d, a=d["a"]), out), "K-blocked A and contiguous A differ"


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_gemm_row_sums_stop_inside_a_ragged_tile(bias):
    """rowsumsq_cols = 64 < N = 136, M = 129, K = 64, with and without a bias, on the two tile kernels (one epilogue, shared
    with the two-pair kernels): sums of the stored bf16 output, the output bit-equal to the call without them, nothing
    written past the 64 columns' one block, and the same bits from both kernels."""
    from ltxmi import ops
    (M, N, K), cols = gc.ROWSUMSQ_EDGE
    c = dict(M=M, N=N, K=K, epi="none", family="plain", bias=bias, algo=0)
    d, truth, mag = _inputs(c)
    nb = cols // 64
    got = []
    for algo, want in ((128, 0), (256, 1)):
        ca = dict(c, algo=algo, id=want)
        plain = _run(ca, d)
        kw, out_buf, out = gc.call_args(ca, d)
        ss = torch.full((M + 2, nb + 3), -7.0, dtype=torch.float32, device=DEV)
        assert ops.gemm_kernel_id(rowsumsq=ss[1:M + 1], rowsumsq_cols=cols, **kw) == want
        ops.gemm(rowsumsq=ss[1:M + 1], rowsumsq_cols=cols, **kw)
        torch.cuda.synchronize()
        assert gc.sentinels_intact(out_buf, out)
        assert torch.equal(out, plain), f"algo {algo}: the output changes with rowsumsq"
        want_ss = out[:, :cols].double().reshape(M, nb, 64).pow(2).sum(-1)
        torch.testing.assert_close(ss[1:M + 1, :nb].double(), want_ss, rtol=1e-5, atol=1e-6)
        assert bool((ss[:, nb:] == -7.0).all()) and bool((ss[0] == -7.0).all()) and bool((ss[M + 1] == -7.0).all())
        got.append((out, ss))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), "the two tile kernels differ"
    _note(gc.compare(got[0][0], truth, mag, what=f"rowsumsq edge bias={bias}"), f"rowsumsq edge bias={bias}")


@pytest.mark.parametrize("cols", gc.ROWSUMSQ_COLS)
def test_gemm_row_sums_cut_inside_a_sub_tile(cols):
    """rowsumsq_cols a multiple of 64 but not of 256, ragged M, sentinel columns in the sums: on the three kernels the sums
    are the float64 sums of squares of the stored bf16 output (rtol 1e-5 / atol 1e-6), the output is bit-equal to the call
    without them, and the sums are bit-equal across the kernels (what sumsq4 exists for)."""
    from ltxmi import ops
    M, N, K = gc.ROWSUMSQ_SHAPE
    c = dict(M=M, N=N, K=K, epi="none", family="plain", bias=True, algo=0)
    d, truth, mag = _inputs(c)
    nb = cols // 64
    sums = []
    for algo, want in ((0, 2), (128, 0), (256, 1)):
        ca = dict(c, algo=algo, id=want)
        plain = _run(ca, d)
        kw, out_buf, out = gc.call_args(ca, d)
        ss = torch.full((M + 2, nb + 3), -7.0, dtype=torch.float32, device=DEV)
        assert ops.gemm_kernel_id(rowsumsq=ss[1:M + 1], rowsumsq_cols=cols, **kw) == want
        ops.gemm(rowsumsq=ss[1:M + 1], rowsumsq_cols=cols, **kw)
        torch.cuda.synchronize()
        assert gc.sentinels_intact(out_buf, out)
        assert torch.equal(out, plain), f"algo {algo}: the output changes with rowsumsq"
        want_ss = out[:, :cols].double().reshape(M, nb, 64).pow(2).sum(-1)
        torch.testing.assert_close(ss[1:M + 1, :nb].double(), want_ss, rtol=1e-5, atol=1e-6)
        assert bool((ss[:, nb:] == -7.0).all()) and bool((ss[0] == -7.0).all()) and bool((ss[M + 1] == -7.0).all())
        sums.append(ss)
        if algo == 0:
            # the persistent kernel twice into fresh buffers: equal bits, output and sums
            kw2, out_buf2, out2 = gc.call_args(ca, d)
            ss2 = torch.full_like(ss, -7.0)
            ops.gemm(rowsumsq=ss2[1:M + 1], rowsumsq_cols=cols, **kw2)
            torch.cuda.synchronize()
            assert gc.sentinels_intact(out_buf2, out2)
            assert torch.equal(out2, out) and torch.equal(ss2, ss), "two runs of the persistent kernel differ"
            _note(gc.compare(out, truth, mag, what=f"rowsumsq cols {cols}"), f"rowsumsq cols {cols}")
    assert torch.equal(sums[0], sums[1]) and torch.equal(sums[0], sums[2]), "row sums of squares differ between kernels"
