"""CPU pins of tests/gemm_cases.py: the slack is what the module says it measured, the fp32 restatement meets every metric
on every (family, epilogue, K) the GPU file uses, every GPU case is headed for the kernel it names, and the truth's
K-blocked gather and group indexing equal a naive loop."""
import pytest
import torch

import gemm_cases as gc


def test_slack_is_the_measured_excess():
    worst = gc.measure_excess()
    assert set(worst) == set(gc.MEASURED_EXCESS_BY_EPI)
    for epi, m in worst.items():
        rec = gc.MEASURED_EXCESS_BY_EPI[epi]
        print(f"{epi}: measured {m:.3e} ({m / 2.0 ** -24:.2f} x 2^-24), recorded {rec:.3e}")
        assert m <= rec <= 1.25 * m, (epi, m, rec)
    assert gc.MEASURED_EXCESS == max(gc.MEASURED_EXCESS_BY_EPI.values())
    assert gc.SLACK == 4.0 * gc.MEASURED_EXCESS


def test_slack_cases_cover_the_gpu_cases():
    used = {(c["family"], c["epi"], c["K"]) for c in gc.GPU_CASES}
    assert used <= set(gc.SLACK_CASES)
    assert {k for _, _, k in used} >= {64, 128, 192, 256, 320, 8192}
    assert len({gc.case_id(c) for c in gc.GPU_CASES}) == len(gc.GPU_CASES)


@pytest.mark.parametrize("family,epi,K", gc.SLACK_CASES, ids=lambda v: str(v))
def test_fp32_restatement_meets_every_metric(family, epi, K):
    M, N = gc.SLACK_MN
    assert (family, epi) not in gc.DROPPED
    d = gc.make(family, M, N, K, epi)
    for t in d.values():
        if torch.is_tensor(t):
            assert t.dtype == gc.BF and bool(torch.isfinite(t.float()).all())
    truth, mag = gc.gemm_op(d, epi)
    gc.compare(gc.restate(d, epi), truth, mag, what=f"restate {family} {epi} K{K}")


def test_dropped_list():
    assert gc.DROPPED == {}
    assert len({e for _, e in gc.DROPPED}) == len(gc.DROPPED)          # at most one family per epilogue


def test_cancel_family_cancels():
    """The band is there: the chosen element of each column is below 2^-8 of its sum of magnitudes; gated, every element."""
    M, N, K = 200, 264, 192
    d = gc.make("cancel", M, N, K, "none")
    t, mag = gc.gemm_op(d, "none")
    cols = torch.arange(N)
    assert float((t.abs() / mag)[(7 * cols + 3) % M, cols].max()) <= 2.0 ** -8
    d = gc.make("cancel", M, N, K, "gate")
    t, mag = gc.gemm_op(d, "gate")
    assert float((t.abs() / mag).max()) <= 2.0 ** -8
    # ... and an epilogue that rounds to bf16 before its last addition is caught by the per-element metric
    early = ((d["a"].float() @ d["w"].float().T + d["bias"].float()) * gc.gate_rows(d, M, torch.float32)).to(gc.BF).float()
    with pytest.raises(AssertionError):
        gc.compare((early + d["residual"].float()).to(gc.BF), t, mag, what="rounded early")


@pytest.mark.parametrize("c", gc.GPU_CASES, ids=gc.case_id)
def test_every_gpu_case_names_its_kernel(c):
    from ltxmi import ops
    kw, _, _ = gc.call_args(c, gc.empty_inputs(c))
    assert ops.gemm_kernel_id(**kw) == c["id"]


@pytest.mark.parametrize("cols", gc.ROWSUMSQ_COLS)
def test_rowsumsq_cases_name_their_kernels(cols):
    from ltxmi import ops
    M, N, K = gc.ROWSUMSQ_SHAPE
    c = dict(M=M, N=N, K=K, epi="none", family="plain", bias=True, algo=0)
    ss = torch.empty(M, cols // 64 + 3)
    for algo, want in ((0, 2), (128, 0), (256, 1)):
        kw, _, _ = gc.call_args(dict(c, algo=algo), gc.empty_inputs(c))
        assert ops.gemm_kernel_id(rowsumsq=ss, rowsumsq_cols=cols, **kw) == want


def test_rowsumsq_edge_case_names_its_kernels():
    from ltxmi import ops
    (M, N, K), cols = gc.ROWSUMSQ_EDGE
    assert cols < N and N % 16 == 8 and M % 16 == 1
    ss = torch.empty(M, cols // 64 + 3)
    for bias in (True, False):
        c = dict(M=M, N=N, K=K, epi="none", family="plain", bias=bias, algo=0)
        for algo, want in ((0, 0), (128, 0), (256, 1)):
            kw, _, _ = gc.call_args(dict(c, algo=algo), gc.empty_inputs(c))
            assert ops.gemm_kernel_id(rowsumsq=ss, rowsumsq_cols=cols, **kw) == want


def test_edge_cases_reach_both_tile_kernels():
    for want in (0, 1):
        mine = [c for c in gc.EDGE_CASES if c["id"] == want]
        assert {c["epi"] for c in mine if not c["bias"]} == set(gc.EPIS)
        assert {c["K"] for c in mine} == {64, 128, 192} and {c["M"] for c in mine} == {17, 129, 257}
        assert {c["N"] for c in mine} == {8, 136}


def test_truth_indexing_equals_a_naive_loop():
    """5 x 16 x 128: K-blocked gather (two blocks of 64) and rows_per_group = 2 against element-by-element loops."""
    M, N, K, P, rpg = 5, 16, 128, 2, 2
    d = gc.make("plain", M, N, K, "gate", rows_per_group=rpg)
    blocked = gc.block_a(d["a"], P)
    flat = blocked.reshape(-1).double()
    a = gc.gather_a(blocked[0], K, K // P, M * (K // P))
    assert torch.equal(a, d["a"])
    got, mag = gc.gemm_op(d, "gate", a=a)
    w, b, gt, ge, r = (d[k].double() for k in ("w", "bias", "gate_table", "temb_full", "residual"))
    for m in range(M):
        for n in range(N):
            acc = mg = 0.0
            for k in range(K):
                av = float(flat[(k // 64) * (M * 64) + m * 64 + k % 64])
                acc += av * float(w[n, k])
                mg += abs(av * float(w[n, k]))
            g1, g2 = float(gt[n]), float(ge[m // rpg, 2 * N + n])
            want = float(r[m, n]) + (g1 + g2) * (acc + float(b[n]))
            wmag = (mg + abs(float(b[n]))) * (abs(g1) + abs(g2)) + abs(float(r[m, n]))
            assert abs(float(got[m, n]) - want) <= 1e-12 * wmag
            assert abs(float(mag[m, n]) - wmag) <= 1e-12 * wmag
