"""CPU pin of tests/attn_output_cases.py, the infrastructure of tests/test_gpu_attention_output.py: the truth against the
oracle, the witnesses' conditions on the built inputs, the restatement's recorded figures, and -- the point -- every planted
defect rejected by the instrument that is there for it, on every case where it applies.  Cases run with two heads here
(``shrunk``): a row's arithmetic does not depend on the head count, and ``restate`` is told the kernel id."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attn_bias_cases as bc  # noqa: E402
import attn_output_cases as ac  # noqa: E402
from test_abi import ATTN_KERNEL_IDS  # noqa: E402

SMALL = [ac.shrunk(c) for c in ac.ALL_CASES]
BIAS_CASES = [c for c in SMALL if c.bias]
ids = ac.case_id


# ------------------------------------------------------------------ the case table
def test_every_case_reaches_the_kernel_it_names():
    """The selection restated in the cases module against the library's, on every case with its real strides, on both sides
    of every threshold the table uses, and on the rows of the id table of tests/test_abi.py."""
    from ltxmi import _lib
    seen = set()
    for c in ac.ALL_CASES:
        ks, vs = ac.kv_strides(c)
        assert ac.expected_id(c.B, c.H, c.Lq, c.Lk, c.dh, c.bias, ks, vs) == c.kid, c
        assert _lib.lib.ltxmi_attention_kernel_id(c.B, c.H, c.Lq, c.Lk, c.dh, int(c.bias), ks, vs) == c.kid, c
        seen.add(c.kid)
    assert seen == set(range(8))
    for row in ATTN_KERNEL_IDS:
        *shape, want = row
        if want < 0:
            continue                                                     # (argument errors: not a selection)
        assert ac.expected_id(shape[0], shape[1], shape[2], shape[3], shape[4], bool(shape[5]), shape[6], shape[7]) == want, row
    # the other side of each threshold: one workgroup fewer, one key fewer / more, the span just inside
    lib = _lib.lib.ltxmi_attention_kernel_id
    assert lib(2, 48, 256, 65, 64, 0, 3072, 3072) == 0 and lib(2, 48, 257, 65, 64, 0, 3072, 3072) == 3
    assert lib(1, 64, 256, 1024, 128, 0, 8192, 8192) == 4 and lib(1, 64, 257, 1023, 128, 0, 8192, 8192) == 4
    assert lib(2, 3, 1023, 256, 64, 1, 192, 192) == 1 and lib(2, 3, 1024, 257, 64, 1, 192, 192) == 1
    assert lib(2, 3, 1024, 256, 64, 0, 192, 192) == 7
    c2 = ac.CASES[2][0]
    ks, vs = ac.kv_strides(c2)
    assert lib(c2.B, c2.H, c2.Lq, c2.Lk, 64, 0, ks - 16, vs) == 3 and lib(c2.B, c2.H - 1, c2.Lq, c2.Lk, 64, 0, ks, vs) == 0


def test_grids_touch_every_value_of_the_table():
    want = {0: ({1, 31, 33, 128, 129, 200}, {1, 63, 64, 65, 129, 333}), 4: ({1, 33, 129, 257}, {1, 64, 65, 200, 1029}),
            2: ({257, 300, 512}, {65, 130}), 3: ({257, 300, 512}, {1, 63, 64, 65, 192, 193, 256, 257, 321, 449}),
            6: ({257, 300, 512}, {1024, 1025, 1087, 1089, 1100}),
            7: ({1024, 1025, 1151, 1153, 1300}, {1, 63, 64, 65, 128, 129, 192, 193, 255, 256})}
    want[1], want[5] = want[0], want[4]
    for kid, (lqs, lks) in want.items():
        assert {c.Lq for c in ac.CASES[kid]} == lqs and {c.Lk for c in ac.CASES[kid]} == lks, kid
    assert {c.bias for c in ac.CASES[7]} == {True, False}


# ------------------------------------------------------------------ truth
@pytest.mark.parametrize("c", [SMALL[5], ac.shrunk(ac.CASES[4][3]), ac.shrunk(ac.CASES[7][3])], ids=ids)
def test_truth_is_the_oracles_attention(c):
    from oracle import dit
    q, k, v = ac.family_inputs(c, "plain")
    t, mag = ac.truth(q, k, v)
    want = dit.sdpa_nhd(q.double(), k.double(), v.double())
    # (sdpa_nhd takes its scores and its softmax in fp32 whatever it is given: its own error, not the truth's)
    assert float((t - want).abs().max()) <= 5e-6
    assert bool((mag >= t.abs() - 1e-12).all())


@pytest.mark.parametrize("c", [BIAS_CASES[5], BIAS_CASES[-1]], ids=ids)
def test_truth_with_removed_keys_is_masked_truth(c):
    q, k, v = ac.family_inputs(c, "plain")
    for name, keep in ac.keep_patterns(c):
        for value in (-math.inf, float(torch.finfo(torch.float32).min)):
            t, _ = ac.truth(q, k, v, bc.bias_from(keep, value))
            assert float((t - bc.masked_truth(q, k, v, keep)).abs().max()) <= 1e-12, (name, value)


def test_finish_q_is_the_oracles_norm_and_rope():
    from oracle import dit
    c = ac.shrunk(ac.CASES[0][5])
    for per_sample in (False, True):
        raw, w, cos, sin, rows = ac.random_q_on_load(c, per_sample=per_sample)
        D = c.H * c.dh
        x = raw.double().view(c.B, c.Lq, D)
        qn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w.double()
        want = dit.apply_rotary_emb(qn, (cos.double().view(-1, c.Lq, D), sin.double().view(-1, c.Lq, D)))
        got = ac.finish_q(raw, w, 1e-6, cos, sin, c.B, c.Lq, c.H, c.dh)
        assert float((got.reshape(c.B, c.Lq, D) - want).abs().max()) <= 1e-12


# ------------------------------------------------------------------ the witnesses' conditions
@pytest.mark.parametrize("c", SMALL, ids=ids)
def test_selector_conditions(c):
    """float64 on the built inputs: gap >= 20 nats, the other keys' total weight <= 2^-12, scores within +-62 nats; pi covers
    what it must; the restatement of the case's kernel returns v[pi] bit for bit."""
    for amp_div in (1.0, 2.0):
        q, k, v, pi = ac.selector(c, a_div=amp_div)
        s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * (amp_div / math.sqrt(c.dh))
        sel = s.gather(-1, pi.view(1, 1, -1, 1).expand(c.B, c.H, c.Lq, 1))
        assert bool((sel == s.max(-1, keepdim=True).values).all())
        assert float(s.max()) <= 62.0 and float(s.min()) >= -62.0
        if c.Lk > 1:
            others = s.scatter(-1, pi.view(1, 1, -1, 1).expand(c.B, c.H, c.Lq, 1), -math.inf)
            assert float((sel[..., 0] - others.max(-1).values).min()) >= 20.0
            assert float(torch.exp(others - sel).sum(-1).max()) <= 2.0 ** -12
    covered = set(pi.tolist())
    assert covered >= (set(range(c.Lk)) if c.Lq >= c.Lk else set(ac.stratified_keys(c.Lk)))
    assert {0, min(63, c.Lk - 1), c.Lk - 1} <= covered and (c.Lk <= 64 or 64 in covered)
    bias = torch.zeros(c.B, c.Lk) if c.bias else None
    assert torch.equal(ac.restate(c.kid, q, k, v, bias, scale=2.0 / math.sqrt(c.dh)), v[:, pi])
    q, k, v, pi = ac.selector(c)
    assert torch.equal(ac.restate(c.kid, q, k, v, bias), v[:, pi])
    if c.kid in (3, 6):
        # the second amplitude: every score far outside the steady range (the exact form is what answers), same bits
        q, k, v, pi = ac.selector(c, amplitude=ac.REDO_AMPLITUDE)
        s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) / math.sqrt(c.dh)
        assert float(s.max(-1).values.min()) >= 250.0
        assert torch.equal(ac.restate(c.kid, q, k, v), v[:, pi])
        assert torch.equal(ac.restate(c.kid, q, k, v, force_exact=True), v[:, pi])


@pytest.mark.parametrize("kind", ["cos", "sin"])
@pytest.mark.parametrize("c", [SMALL[5], ac.shrunk(ac.CASES[3][9]), ac.shrunk(ac.CASES[4][4]), ac.shrunk(ac.CASES[6][4]),
                               ac.shrunk(ac.CASES[7][3])], ids=ids)
def test_selector_through_q_on_load(c, kind):
    """Raw q, weight and +-1 tables whose finished q (float64) is the selector's q to 1e-4 relative: one bf16 rounding
    returns it exactly, and the restatement (fp32 finish, the kernel's roundings) still returns v[pi]."""
    q, k, v, pi = ac.selector(c)
    for per_sample in (False, True):
        raw, w, cos, sin, rows = ac.q_on_load_inputs(q, kind, per_sample=per_sample)
        assert rows == (c.B * c.Lq if per_sample else c.Lq)
        fin = ac.finish_q(raw, w, 1e-6, cos, sin, c.B, c.Lq, c.H, c.dh)
        assert float(((fin - q.double()) / q.double()).abs().max()) <= 1e-4
        assert torch.equal(fin.float().to(ac.BF), q)
        bias = torch.zeros(c.B, c.Lk) if c.bias else None
        assert torch.equal(ac.restate(c.kid, None, k, v, bias, on_load=(raw, w, 1e-6, cos, sin)), v[:, pi])


@pytest.mark.parametrize("c", ac.ALL_CASES, ids=ids)
def test_uniform_conditions(c):
    """FULL head count (the GPU's inputs): non-zero integer values, no quotient near a bf16 tie -- plain, under every keep
    pattern and under the power-of-two bias of the bias cases -- and the restatement returns the truth's bits."""
    q, k, v = ac.uniform(c)
    assert bool((v.float().abs() >= 1).all() & (v.float().abs() <= 4).all() & (v.float() == v.float().round()).all())
    t, x, n = ac.uniform_truth(v)
    assert bool((n == c.Lk).all()) and ac.uniform_is_decidable(x, n)
    if c.H > 4:
        return
    assert torch.equal(ac.restate(c.kid, q, k, v, torch.zeros(c.B, c.Lk) if c.bias else None), t.expand(-1, c.Lq, -1, -1))
    if not c.bias:
        return
    for name, keep in ac.keep_patterns(c):
        t, x, n = ac.uniform_truth(v, keep)
        assert bool((n == keep.sum(-1)).all()) and ac.uniform_is_decidable(x, n), name
        assert torch.equal(ac.restate(c.kid, q, k, v, bc.bias_from(keep, -math.inf)), t.expand(-1, c.Lq, -1, -1)), name
    bias, e = ac.pow2_bias(c)
    t, x, n = ac.uniform_truth(v, e=e)
    assert ac.uniform_is_decidable(x, n)
    assert torch.equal(ac.restate(c.kid, q, k, v, bias), t.expand(-1, c.Lq, -1, -1))


# ------------------------------------------------------------------ the restatement's figures
def test_recorded_restatement_maxima_are_what_the_cpu_measures():
    worst = ac.measure_restatement()
    assert set(worst) == set(ac.MEASURED_RESTATEMENT_MAX)
    for key, m in sorted(worst.items()):
        rec = ac.MEASURED_RESTATEMENT_MAX[key]
        print(f"kernel {key[0]} {key[1]}: measured {m:.3e}, recorded {rec:.3e}")
        assert m <= rec <= 1.25 * m, (key, m, rec)
    # the fold's price on trained-like logits: id 4 re-rounds q x scale x log2(e); the unfolded ids stay at the P roundings
    assert ac.MEASURED_RESTATEMENT_MAX[(4, "peaked")] > 3 * ac.MEASURED_RESTATEMENT_MAX[(5, "peaked")]
    assert ac.MARGIN == 2.0


# ------------------------------------------------------------------ planted defects
def _bound_and_figures(c, family, defect, on_load=None):
    q, k, v = ac.family_inputs(c, family)
    bias = ac.soft_bias(c) if c.bias else None
    if on_load is not None:
        raw, w, cos, sin, _ = on_load
        q = ac.finish_q(raw, w, 1e-6, cos, sin, c.B, c.Lq, c.H, c.dh)
        on_load = (raw, w, 1e-6, cos, sin)
    t, mag = ac.truth(q, k, v, bias)
    good = float(ac.figure(ac.restate(c.kid, q, k, v, bias, on_load=on_load), t, mag).max())
    bad = float(ac.figure(ac.restate(c.kid, q, k, v, bias, on_load=on_load, defect=defect), t, mag).max())
    return ac.MARGIN * good, bad


@pytest.mark.parametrize("c", SMALL, ids=ids)
def test_planted_defects_are_rejected_by_the_witnesses(c):
    q, k, v, pi = ac.selector(c)
    qu, ku, vu = ac.uniform(c)
    zero = torch.zeros(c.B, c.Lk) if c.bias else None
    tu = ac.uniform_truth(vu)[0].expand(-1, c.Lq, -1, -1)
    A1 = ("drop_last_key", "swap_v_rows", "swap_out_rows")
    A2 = ("drop_last_key", "extra_zero_key", "last_key_twice")
    for d in A1:
        if ac.defect_applies(d, c):
            assert not torch.equal(ac.restate(c.kid, q, k, v, zero, defect=d), v[:, pi]), f"selector passes {d}"
    for d in A2:
        if ac.defect_applies(d, c) and not (d == "last_key_twice" and c.Lk == 1):     # (one key twice is that key)
            assert not torch.equal(ac.restate(c.kid, qu, ku, vu, zero, defect=d), tu), f"uniform passes {d}"
    if ac.defect_applies("bias_shift", c):
        for name, keep in ac.keep_patterns(c):
            if bool((torch.roll(keep, 1, 1) == keep).all()):
                continue                                                 # (a pattern the shift maps to itself)
            bias = bc.bias_from(keep, -math.inf)
            t = ac.uniform_truth(vu, keep)[0].expand(-1, c.Lq, -1, -1)
            assert not torch.equal(ac.restate(c.kid, qu, ku, vu, bias, defect="bias_shift"), t), f"uniform+{name} passes a shifted bias"


@pytest.mark.parametrize("c", [c for c in SMALL if c.Lk > 1], ids=ids)
def test_planted_defects_are_rejected_by_the_row_figure(c):
    """A missed rescale (row sum x (1 + 2^-6)) on ``offset``, where the normaliser shows; a softmax scale 2 % off on
    ``peaked``; a RoPE sign on one channel pair of one head with random tables."""
    bound, bad = _bound_and_figures(c, "offset", "rowsum_scale")
    assert bad > bound, ("rowsum_scale", bad, bound)
    # (id 4 re-rounds q x scale x log2(e) to bf16: on ``peaked`` that fold alone costs 1e-2 and a 2 % scale hides under
    # twice it -- the fold's price, profiles/attention_output_figures.md; ``plain`` rejects it there as everywhere)
    for family in ("plain", "peaked"):
        bound, bad = _bound_and_figures(c, family, "scale_2pct")
        assert bad > bound or (c.kid == 4 and family == "peaked"), ("scale_2pct", family, bad, bound)
    bound, bad = _bound_and_figures(c, "plain", "rope_sign", on_load=ac.random_q_on_load(c))
    assert bad > bound, ("rope_sign", bad, bound)
