"""The two-pair GEMM (ltxmi_gemm_pair2_bf16) on a real MI355X.  Every case of tests/lora_gemm_cases.py asserts which kernel
its call takes (3 the 128x128 two-pair kernel, 4 the 256x256 one), writes into a view inside a sentinel-filled buffer, and must

  * equal, by torch.equal, what ``ops.gemm`` gives on the materialised concatenation [A | A2_g], [W | W2] with K = K1 + K2
    (grouped cases: per group, on the group's column slice) -- the K-tiles are accumulated in the same order and the epilogue
    is the same sequence, so the bits are the same whichever kernel the concatenated call takes;
  * meet the three metrics of tests/gemm_cases.py against the float64 truth of that concatenation.

Then: the two forms agree with each other bit for bit, the row sums of squares equal those of the concatenated call, and a
refused call raises and leaves its output as it was."""
import pytest
import torch

import gemm_cases as gc
import lora_gemm_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"

_cache = []          # [(key, inputs)]: neighbouring cases share inputs


def _inputs(c):
    key = (c["family"], c["M"], c["N"], c["K"], c["epi"], c["bias"], c.get("rows_per_group"))
    for k, d in _cache:
        if k == key:
            return d
    del _cache[:]
    d = gc.make(c["family"], c["M"], c["N"], c["K"], c["epi"], c["bias"], c.get("rows_per_group"), device=DEV)
    _cache.append((key, d))
    return d


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


def _run_pair(c, d, **over):
    from ltxmi import ops
    kw, out_buf, out = lc.call_args(c, d)
    kw.update(over)
    if not over:
        assert ops.gemm_kernel_id(**kw) == c["id"], "the case does not reach the kernel it is about"
    ops.gemm(**kw)
    torch.cuda.synchronize()
    assert gc.sentinels_intact(out_buf, out), "wrote outside the output view"
    return out


def _run_concatenated(c, dg):
    """ops.gemm on the concatenation, kernel chosen by shape, same output / residual forms as the case."""
    from ltxmi import ops
    cc = dict(c, algo=0, M=dg["a"].shape[0], N=dg["w"].shape[0], K=dg["a"].shape[1])
    kw, out_buf, out = gc.call_args(cc, dg)
    ops.gemm(**kw)
    torch.cuda.synchronize()
    assert gc.sentinels_intact(out_buf, out)
    return out


@pytest.mark.parametrize("c", lc.GPU_CASES, ids=lc.case_id)
def test_two_pair_case(c):
    what = lc.case_id(c)
    d = _inputs(c)
    out = _run_pair(c, d)
    gcols = c["group_cols"] or c["N"]
    for g in range(c["groups"]):
        dg = lc.concatenation(c, d, g)
        mine = out[:, g * gcols:(g + 1) * gcols]
        ref = _run_concatenated(c, dg)
        assert torch.equal(mine, ref), f"{what}: group {g} differs from ops.gemm on the concatenation " \
                                       f"({int((mine != ref).sum())} values, max |diff| {float((mine.float() - ref.float()).abs().max()):.3e})"
        truth, mag = gc.gemm_op(dg, c["epi"])
        gc.compare(mine, truth, mag, what=f"{what} group {g}")


def test_the_two_forms_agree_bit_for_bit():
    c = next(c for c in lc.GPU_CASES if (c["M"], c["N"]) == lc.BIG_MN and c["epi"] == "gate" and c["K1"] == 2048)
    d = _inputs(c)
    from ltxmi import ops
    kw = lc.call_args(c, d)[0]
    assert ops.gemm_kernel_id(**dict(kw, algo=128)) == 3 and ops.gemm_kernel_id(**dict(kw, algo=256)) == 4
    assert torch.equal(_run_pair(c, d, algo=128), _run_pair(c, d, algo=256))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_row_sums_stop_inside_a_ragged_tile(bias):
    """rowsumsq_cols = 64 < N = 136, M = 129, K = 64 + 64, with and without a bias: on both forms the output and the sums are
    the bits of ops.gemm with the sums on the concatenation, and nothing is written past the one block of sums."""
    from ltxmi import ops
    (M, N, _), cols = gc.ROWSUMSQ_EDGE
    c = lc._case((M, N), 64, 64, bias=bias)
    d = _inputs(c)
    ref_ss = torch.full((M, 4), -7.0, dtype=torch.float32, device=DEV)
    ref = ops.gemm(d["a"], d["w"], d["bias"], rowsumsq=ref_ss, rowsumsq_cols=cols)
    torch.cuda.synchronize()
    for algo, want in ((128, 3), (256, 4)):
        kw, out_buf, out = lc.call_args(c, d)
        ss = torch.full((M + 2, 4), -7.0, dtype=torch.float32, device=DEV)
        kw.update(algo=algo, rowsumsq=ss[1:M + 1], rowsumsq_cols=cols)
        assert ops.gemm_kernel_id(**kw) == want
        ops.gemm(**kw)
        torch.cuda.synchronize()
        assert gc.sentinels_intact(out_buf, out)
        assert torch.equal(out, ref), f"algo {algo}: differs from ops.gemm on the concatenation"
        assert torch.equal(ss[1:M + 1], ref_ss), f"algo {algo}: row sums differ"
        assert bool((ss[:, 1:] == -7.0).all()) and bool((ss[0] == -7.0).all()) and bool((ss[M + 1] == -7.0).all())
        want_ss = out[:, :cols].double().pow(2).sum(-1, keepdim=True)
        torch.testing.assert_close(ss[1:M + 1, :1].double(), want_ss, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("cols", lc.ROWSUMSQ_COLS)
def test_row_sums_of_squares_see_the_adapter(cols):
    """The q row sums of a packed QKV projection with an adapter: on both forms the sums and the output are the bits of the
    concatenated call's, sentinel rows and columns of the sums stay, and the sums are those of the stored bf16 output."""
    from ltxmi import ops
    M, N = 1100, 768
    c = lc._case((M, N), 128, 64, groups=3, group_cols=256)
    d = _inputs(c)
    nb = cols // 64
    results = []
    for algo, want in ((128, 3), (256, 4)):
        kw, out_buf, out = lc.call_args(c, d)
        ss = torch.full((M + 2, nb + 3), -7.0, dtype=torch.float32, device=DEV)
        kw.update(algo=algo, rowsumsq=ss[1:M + 1], rowsumsq_cols=cols)
        assert ops.gemm_kernel_id(**kw) == want
        ops.gemm(**kw)
        torch.cuda.synchronize()
        assert gc.sentinels_intact(out_buf, out)
        want_ss = out[:, :cols].double().reshape(M, nb, 64).pow(2).sum(-1)
        torch.testing.assert_close(ss[1:M + 1, :nb].double(), want_ss, rtol=1e-5, atol=1e-6)
        assert bool((ss[:, nb:] == -7.0).all()) and bool((ss[0] == -7.0).all()) and bool((ss[M + 1] == -7.0).all())
        assert torch.equal(out, _run_pair(c, d, algo=algo)), "the output changes with rowsumsq"
        results.append((out, ss))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    # the concatenated call of each group, with the sums where the group holds q columns
    out, ss = results[0]
    for g in range(3):
        dg = lc.concatenation(c, d, g)
        lo = g * 256
        gcols = min(max(cols - lo, 0), 256)
        ref_ss = torch.full((M, 4), -7.0, dtype=torch.float32, device=DEV)
        ref = ops.gemm(dg["a"], dg["w"], dg["bias"], rowsumsq=ref_ss if gcols else None, rowsumsq_cols=gcols)
        torch.cuda.synchronize()
        assert torch.equal(out[:, lo:lo + 256], ref)
        if gcols:
            assert torch.equal(ss[1:M + 1, lo // 64:(lo + gcols) // 64], ref_ss[:, :gcols // 64]), f"group {g}: row sums differ"


def test_refused_calls_raise_and_leave_the_output_untouched():
    from ltxmi import ops
    from ltxmi._lib import LtxmiError
    c = lc._case(lc.SMALL_MN, 128, 64)
    d = _inputs(c)
    bf = torch.bfloat16
    M, N = lc.SMALL_MN
    kw, out_buf, out = lc.call_args(c, d)
    bad = [dict(a2=kw["a2"][:, :32].contiguous(), w2=kw["w2"][:, :32].contiguous()),              # K2 = 32
           dict(a2_group_cols=128),                                                                 # 264 % 128 != 0 (shape check)
           dict(a2=torch.zeros(M, 72, dtype=bf, device=DEV)[:, 4:68]),                              # A2 off a 16-byte boundary
           dict(w2=torch.zeros(N, 72, dtype=bf, device=DEV)[:, 4:68]),
           dict(a2=torch.zeros(M, 68, dtype=bf, device=DEV)[:, :64]),                               # lda2 % 8 != 0
           dict(algo=7),
           dict(w2=None),
           dict(a2=kw["a2"][:M - 1])]
    for over in bad:
        with pytest.raises((LtxmiError, ValueError)):
            ops.gemm(**dict(kw, **over))
    torch.cuda.synchronize()
    assert bool((out_buf == gc.SENTINEL).all()), "a refused call wrote to its output"
    # a K-blocked first operand takes no second pair
    blocked = gc.block_a(d["a"][:, :128].contiguous(), 2)
    with pytest.raises(LtxmiError):
        ops.gemm(**dict(kw, a=blocked[0], a_kblock=64, a_kblock_stride=M * 64))
    torch.cuda.synchronize()
    assert bool((out_buf == gc.SENTINEL).all())
