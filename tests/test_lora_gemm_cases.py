"""CPU pins of tests/lora_gemm_cases.py: the fp32 restatement meets every metric of tests/gemm_cases.py on every (family,
epilogue, K1 + K2) the GPU file uses, the slack of that module covers the totals it has not measured itself, every GPU case
is headed for the two-pair kernel it names, and the entry check refuses what include/ltxmi.h says it refuses -- all without
a device."""
import ctypes

import pytest
import torch

import gemm_cases as gc
import lora_gemm_cases as lc


def test_case_table_covers_what_it_claims():
    ids = [lc.case_id(c) for c in lc.GPU_CASES]
    assert len(set(ids)) == len(ids)
    for want, mn in ((3, lc.SMALL_MN), (4, lc.BIG_MN)):
        mine = [c for c in lc.GPU_CASES if (c["M"], c["N"]) == mn and c["id"] == want and not c["algo"]]
        assert {(c["K1"], c["K2"]) for c in mine} == set(lc.K_SPLITS)
        assert {c["epi"] for c in mine} == {"none", "gelu", "silu", "gate", "residual"}
        assert {c["family"] for c in mine} == {"plain", "cancel"}
        assert {c["bias"] for c in mine} == {True, False}
        assert {(c["rows_per_group"], c["in_place"]) for c in mine if c["epi"] == "gate" and "in_place" in c} == \
            {(37, True), (37, False), (256, True), (256, False)}
        assert any(c.get("a2_view") for c in mine)
    grouped = {(c["id"], c["group_cols"]) for c in lc.GPU_CASES if c["group_cols"]}
    assert grouped == {(3, 256), (4, 256), (3, 128)}
    assert any((c["M"], c["N"], c["K1"], c["K2"], c["id"]) == (1, 8, 64, 64, 3) for c in lc.GPU_CASES)


def test_slack_covers_the_new_totals():
    """Totals of K that gemm_cases.SLACK_CASES does not hold are measured here; none may exceed what its SLACK rests on."""
    new = [k for k in lc.SLACK_CASES if k not in set(gc.SLACK_CASES)]
    assert {K for _, _, K in new} >= {2176}
    worst = gc.measure_excess(cases=new)
    for epi, m in worst.items():
        print(f"{epi}: measured {m:.3e} ({m / 2.0 ** -24:.2f} x 2^-24), limit {gc.MEASURED_EXCESS:.3e}")
        assert m <= gc.MEASURED_EXCESS, (epi, m)


@pytest.mark.parametrize("family,epi,K", lc.SLACK_CASES, ids=lambda v: str(v))
def test_fp32_restatement_meets_every_metric(family, epi, K):
    M, N = gc.SLACK_MN
    d = gc.make(family, M, N, K, epi)
    truth, mag = gc.gemm_op(d, epi)
    gc.compare(gc.restate(d, epi), truth, mag, what=f"restate {family} {epi} K{K}")


def test_split_and_concatenation_are_the_same_numbers():
    """Cutting at K1 and putting back together is the identity; a group's concatenation is its slice of the packed product."""
    c = next(c for c in lc.GPU_CASES if c["groups"] == 6)
    d = gc.make(c["family"], 40, c["N"], c["K"], c["epi"], c["bias"])
    a1, w1, a2, w2 = lc.split(c, d)
    assert a2.shape == (40, 6 * 64) and w2.shape == (c["N"], 64)
    for g in range(6):
        want = a1.double() @ w1.double().T + a2[:, g * 64:(g + 1) * 64].double() @ w2.double().T + d["bias"].double()
        got, _ = gc.gemm_op(lc.concatenation(c, d, g), "none")
        assert float((got - want[:, g * 128:(g + 1) * 128]).abs().max()) < 1e-12          # float64, values of order 1
    c1 = lc.GPU_CASES[0]
    d = gc.make(c1["family"], 40, 16, c1["K"], c1["epi"], c1["bias"])
    a1, w1, a2, w2 = lc.split(c1, d)
    assert torch.equal(torch.cat([a1, a2], 1), d["a"]) and torch.equal(torch.cat([w1, w2], 1), d["w"])
    assert lc.concatenation(c1, d) is d


@pytest.mark.parametrize("c", lc.GPU_CASES, ids=lc.case_id)
def test_every_gpu_case_names_its_kernel(c):
    from ltxmi import ops
    kw, _, _ = lc.call_args(c, lc.empty_inputs(c))
    assert ops.gemm_kernel_id(**kw) == c["id"]
    if c["M"] > 1:       # (a one-row slice counts as contiguous and keeps its stride)
        assert kw["a2"].stride(0) == (c["K"] if c.get("a2_view") else c["groups"] * c["K2"])


def test_kernel_id_thresholds_through_ops():
    """256x256 when M >= 768, N >= 256, ceil(M/256) ceil(N/256) >= 128 and group_cols % 256 == 0; else 128x128."""
    from ltxmi import ops
    e = lambda *s: torch.empty(*s, dtype=torch.bfloat16)
    w, w2 = e(4096, 128), e(4096, 64)
    ident = lambda M, **kw: ops.gemm_kernel_id(e(M, 128), w, a2=e(M, kw.pop("cols", 64)), w2=w2, **kw)
    assert ident(2048) == ops.GEMM_PAIR2_TILE256 == 4                     # 8 x 16 = 128 tiles
    assert ident(2047, algo=128) == ops.GEMM_PAIR2_TILE128 == 3
    assert ops.gemm_kernel_id(e(2048, 128), w[:3840], a2=e(2048, 64), w2=w2[:3840]) == 3      # 120 tiles
    assert ops.gemm_kernel_id(e(767, 128), e(11008, 128), a2=e(767, 64), w2=e(11008, 64)) == 3
    assert ops.gemm_kernel_id(e(32768, 128), w[:248], a2=e(32768, 64), w2=w2[:248]) == 3
    assert ident(2048, a2_group_cols=256, cols=16 * 64) == 4
    assert ident(2048, a2_group_cols=128, cols=32 * 64) == 3               # a 256-column tile would straddle two groups
    assert ident(2048, a2_group_cols=128, cols=32 * 64, algo=256) == -1
    assert ident(16, algo=256) == 4
    # without the second pair the call is the one it always was
    assert ops.gemm_kernel_id(e(2048, 128), w) == ops.GEMM_PERSISTENT256
    with pytest.raises(ValueError):
        ops.gemm_kernel_id(e(2048, 128), w, a2=e(2048, 64))                # a2 without w2
    with pytest.raises(ValueError):
        ops.gemm_kernel_id(e(2048, 128), w, a2=e(2047, 64), w2=w2)
    with pytest.raises(TypeError):
        ops.gemm_kernel_id(e(2048, 128), w, a2=e(2048, 64).float(), w2=w2)


@pytest.mark.parametrize("case", lc.REFUSALS, ids=lambda c: c[0])
def test_entry_check_refusal_table(case):
    from ltxmi import _lib
    what, over, want = case
    a, p = lc.geometry(over)
    got = lc.kernel_id(a, p)
    assert got == want, (what, got, _lib.lib.ltxmi_last_error())
    if want < 0:
        assert _lib.lib.ltxmi_last_error()
        # the launch refuses the same arguments with the same status, before it needs a device
        assert _lib.lib.ltxmi_gemm_pair2_bf16(ctypes.byref(a) if a is not None else None,
                                              ctypes.byref(p) if p is not None else None, None) == want


def test_the_two_pair_call_refuses_cpu_tensors():
    from ltxmi import ops
    e = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.gemm(e(4, 64), e(8, 64), a2=e(4, 64), w2=e(8, 64))
