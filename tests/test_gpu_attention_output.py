"""The attention output O of all eight kernels behind ``ltxmi_attention_fwd_bf16`` on a real MI355X, by the two instruments
of tests/attn_output_cases.py (pinned on the CPU by tests/test_attn_output_cases.py):

A. exact witnesses -- the selector (O == v[pi] bit for bit) and the uniform rows (O == bf16(sum w v / sum w) bit for bit);
B. a per-row figure against float64, bounded by MARGIN = 2 x the largest figure of the kernel family's restated arithmetic
   on the same inputs (both computed on the device).

Every launch asserts the kernel id it runs with the strides it passes.  The cases are the smallest shapes that reach each
kernel's tiling edges (``CASES``); the options -- packed q / strided k, v, a caller's softmax scale, a padded ``out`` view,
``out_segments``, q finished on load -- run on every id.  Bound of the one inexact witness: the short-key kernel (id 7)
stages the key bias as a bf16 hi + lo pair riding on the QK^T product, exact to 2^-16 relative, so under the ``ln 2^e`` bias
its output may differ from the truth by one bf16 ulp; ids 1 and 5 add the bias in fp32 and must be exact."""
import math

import pytest
import torch

import attn_bias_cases as bc
import attn_output_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
SENTINEL = -7.0
ids = ac.case_id
_WORST = {}                                                 # (kernel id, family) -> (restatement max, GPU max, worst ratio)


def _strided(vals, stride):
    """bf16 [B, L, H, dh] on the device with a token stride of ``stride`` elements ((H, dh) contiguous)."""
    B, L, H, dh = vals.shape
    if stride == H * dh:
        return vals.to(DEV)
    buf = torch.empty(B * L * stride, dtype=BF, device=DEV)
    view = torch.as_strided(buf, (B, L, H, dh), (L * stride, stride, dh, 1))
    view.copy_(vals)
    return view


def _place(c, q, k, v, packed=False):
    """The case's operands on the device: k at the case's token stride (id 2: past the 2 GiB span).  packed: q as a slice
    of a [B, Lq, 3, H, dh] projection buffer, k and v as the strided halves of one [B, Lk, 2, H, dh] buffer (id 2 keeps its
    far-apart k rows, or it would be another kernel)."""
    ks, _ = ac.kv_strides(c)
    if not packed:
        return q.to(DEV), _strided(k, ks), v.to(DEV)
    qbuf = torch.full((c.B, c.Lq, 3, c.H, c.dh), 3.0, dtype=BF, device=DEV)
    kvbuf = torch.full((c.B, c.Lk, 2, c.H, c.dh), 3.0, dtype=BF, device=DEV)
    qbuf[:, :, 1].copy_(q)
    kvbuf[:, :, 0].copy_(k)
    kvbuf[:, :, 1].copy_(v)
    return qbuf[:, :, 1], (_strided(k, ks) if c.kid == 2 else kvbuf[:, :, 0]), kvbuf[:, :, 1]


def _bias(c, bias=None):
    if bias is None:
        return torch.zeros(c.B, c.Lk, device=DEV) if c.bias else None
    return bias.to(DEV)


def _run(c, q, k, v, bias=None, **kw):
    from ltxmi import ops
    got = ops.attention_kernel_id(c.B, c.H, c.Lq, c.Lk, c.dh, bias is not None, k.stride(1), v.stride(1))
    assert got == c.kid, f"{ids(c)}: runs kernel {got}"
    return ops.attention(q, k, v, key_bias=bias, **kw)


def _counter():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _segments(Lq):
    """(segments P, tokens per segment): the smallest split of the token axis that is one."""
    P = next((p for p in range(2, Lq + 1) if Lq % p == 0), 1)
    return P, Lq // P


# ------------------------------------------------------------------ A1. the selector
@pytest.mark.parametrize("c", ac.ALL_CASES, ids=ids)
def test_selector_every_layout(c):
    """O == v[pi] bit for bit: plain operands; packed q and strided k / v; a caller's softmax_scale (x 2, the queries' amplitude
    halved); ``out`` as a padded-stride view inside a sentinel-filled buffer; ``out_segments`` (bit-equal to the unsegmented
    call, nothing written between the segments).  The steady form of ids 3 and 6 redoes nothing."""
    q, k, v, pi = ac.selector(c)
    want = v[:, pi].to(DEV)
    qd, kd, vd = _place(c, q, k, v)
    bias = _bias(c)
    counter = _counter()
    plain = _run(c, qd, kd, vd, bias, redo_counter=counter)
    assert torch.equal(plain, want), f"{ids(c)}: {int((plain != want).any(-1).sum())} of {c.B * c.Lq * c.H} rows are not v[pi]"
    if c.kid in (3, 6):
        assert int(counter.item()) == 0
    qp, kp, vp = _place(c, q, k, v, packed=True)
    assert torch.equal(_run(c, qp, kp, vp, bias), want), f"{ids(c)}: packed q / strided k, v"
    q2 = ac.selector(c, a_div=2.0)[0].to(DEV)
    assert torch.equal(_run(c, q2, kd, vd, bias, softmax_scale=2.0 / math.sqrt(c.dh)), want), f"{ids(c)}: softmax_scale"
    # out: rows (H + 1) dh apart, three rows of slack per batch
    buf = torch.full((c.B, c.Lq + 3, c.H + 1, c.dh), SENTINEL, dtype=BF, device=DEV)
    view = buf[:, :c.Lq, :c.H]
    got = _run(c, qd, kd, vd, bias, out=view)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(view, want)
    assert bool((buf[:, c.Lq:] == SENTINEL).all()) and bool((buf[:, :, c.H:] == SENTINEL).all()), f"{ids(c)}: wrote outside out"
    # out_segments: [P][B][Lq / P][H dh] with 16 elements of slack behind every segment
    P, seg = _segments(c.Lq)
    seg_elems = c.B * seg * c.H * c.dh
    send = torch.full((P, seg_elems + 16), SENTINEL, dtype=BF, device=DEV)
    out0 = send[0, :seg_elems].view(c.B, seg, c.H, c.dh)
    _run(c, qd, kd, vd, bias, out=out0, out_segments=(seg, seg_elems + 16))
    got = send[:, :seg_elems].reshape(P, c.B, seg, c.H, c.dh).permute(1, 0, 2, 3, 4).reshape(c.B, c.Lq, c.H, c.dh)
    assert torch.equal(got, plain) and torch.equal(got, want), f"{ids(c)}: segmented store, {P} segments of {seg}"
    assert bool((send[:, seg_elems:] == SENTINEL).all()), f"{ids(c)}: wrote between the segments"


@pytest.mark.parametrize("c", ac.CASES[3] + ac.CASES[6], ids=ids)
def test_selector_far_outside_the_steady_range(c):
    """(a, b) = (4, 8): every row's selected score is >= 256 nats, every work item leaves the steady form's range and is
    redone in the exact form -- the counter says B x H x tiles -- and O is still v[pi]; ``force_exact`` gives the same bits."""
    q, k, v, pi = ac.selector(c, amplitude=ac.REDO_AMPLITUDE)
    want = v[:, pi].to(DEV)
    qd, kd, vd = _place(c, q, k, v)
    counter = _counter()
    out = _run(c, qd, kd, vd, redo_counter=counter)
    assert int(counter.item()) == ac.steady_tiles(c), (int(counter.item()), ac.steady_tiles(c))
    assert torch.equal(out, want)
    assert torch.equal(_run(c, qd, kd, vd, force_exact=True), want)


def _on_load_cases():
    return [c for kid in sorted(ac.CASES) for c in (ac.CASES[kid][0], ac.CASES[kid][len(ac.CASES[kid]) // 2], ac.CASES[kid][-1])]


def _row_factor(raw, eps):
    return torch.rsqrt(raw.float().pow(2).mean(-1) + eps).contiguous()


@pytest.mark.parametrize("c", _on_load_cases(), ids=ids)
def test_selector_through_q_on_load(c):
    """q arrives raw and is finished by the kernel: weight = the amplitude, +-1 tables (cos alone; sin alone: the pair swap
    and its sign), shared (period Lq) and per sample (period B Lq), the row factor as one float per row and as per-64
    partial sums.  The finished q is the selector's q after its one rounding, so O == v[pi] bit for bit."""
    q, k, v, pi = ac.selector(c)
    want = v[:, pi].to(DEV)
    _, kd, vd = _place(c, q, k, v)
    bias = _bias(c)
    eps = 1e-6
    for kind in ("cos", "sin"):
        for per_sample in (False, True):
            raw, w, cos, sin, rows = ac.q_on_load_inputs(q, kind, per_sample=per_sample)
            raw, w, cos, sin = raw.to(DEV), w.to(DEV), cos.to(DEV), sin.to(DEV)
            q4 = raw.view(c.B, c.Lq, c.H, c.dh)
            for factor in (_row_factor(raw, eps), ac.partial_sums(raw)):
                counter = _counter()
                out = _run(c, q4, kd, vd, bias, q_norm=(factor, w, eps), rope=(cos, sin, rows), redo_counter=counter)
                what = f"{ids(c)}: {kind} tables, period {rows}, factor {tuple(factor.shape)}"
                assert torch.equal(out, want), f"{what}: {int((out != want).any(-1).sum())} rows are not v[pi]"
                if c.kid in (3, 6):
                    assert int(counter.item()) == 0, what


# ------------------------------------------------------------------ A2. uniform rows
@pytest.mark.parametrize("c", ac.ALL_CASES, ids=ids)
def test_uniform_rows(c):
    """q = 0: O == bf16(sum_j v_j / n) bit for bit, n the keys that take part -- Lk; for the bias kernels also the kept count
    of every keep pattern written as a 0 / -inf bias, and the power-of-two weights of a ``ln 2^e`` bias (id 7: within one
    bf16 ulp, see the module docstring)."""
    q, k, v = ac.uniform(c)
    qd, kd, vd = _place(c, q, k, v, packed=(c.Lk % 2 == 0))
    t, _, _ = ac.uniform_truth(v)
    want = t.to(DEV).expand(-1, c.Lq, -1, -1)
    counter = _counter()
    out = _run(c, qd, kd, vd, _bias(c), redo_counter=counter)
    assert torch.equal(out, want), f"{ids(c)}: {int((out != want).sum())} of {out.numel()} elements differ from the mean of {c.Lk} keys"
    if c.kid in (3, 6):
        assert int(counter.item()) == 0
        assert torch.equal(_run(c, qd, kd, vd, force_exact=True), want)
    if not c.bias:
        return
    for name, keep in ac.keep_patterns(c):
        want = ac.uniform_truth(v, keep)[0].to(DEV).expand(-1, c.Lq, -1, -1)
        for value in (-math.inf, float(torch.finfo(torch.float32).min)):
            out = _run(c, qd, kd, vd, bc.bias_from(keep, value).to(DEV))
            assert torch.equal(out, want), f"{ids(c)} {name} {value}: {int((out != want).sum())} elements differ"
    bias, e = ac.pow2_bias(c)
    want = ac.uniform_truth(v, e=e)[0].to(DEV).expand(-1, c.Lq, -1, -1)
    out = _run(c, qd, kd, vd, bias.to(DEV))
    if c.kid == 7:
        ulps = (out.view(torch.int16).int() - want.contiguous().view(torch.int16).int()).abs()
        print(f"{ids(c)} power-of-two bias: {int((ulps != 0).sum())} of {out.numel()} elements one ulp off")
        assert int(ulps.max()) <= 1
    else:
        assert torch.equal(out, want), f"{ids(c)} power-of-two bias: {int((out != want).sum())} elements differ"


# ------------------------------------------------------------------ B. the row figure
def _figures(c, family, q_truth, q, k, v, bias, what, on_load=None, scale=None, **kw):
    """GPU and restatement figures on one set of inputs (device tensors); asserts the bound, records the ratio."""
    t, mag = ac.truth(q_truth, k, v, bias, scale=scale)
    out = _run(c, q, k, v, bias, softmax_scale=scale, **kw)
    assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    gpu = ac.figure(out, t, mag)
    restated = ac.restate(c.kid, None if on_load else q, k, v, bias, scale=scale, on_load=on_load)
    rest = float(ac.figure(restated, t, mag).max())
    worst = float(gpu.max())
    ratio = worst / rest if rest > 0 else (0.0 if worst == 0 else math.inf)
    print(f"FIG {what}: restatement max {rest:.3e}, GPU max {worst:.3e} (median {float(gpu.median()):.3e}), ratio {ratio:.2f}; "
          f"{float((out != restated).float().mean()):.2e} of the elements differ from the restatement's bits")
    key = (c.kid, family)
    old = _WORST.get(key, (0.0, 0.0, 0.0))
    _WORST[key] = (max(old[0], rest), max(old[1], worst), max(old[2], ratio))
    assert worst <= ac.MARGIN * rest, f"{what}: row figure {worst:.3e} > {ac.MARGIN} x {rest:.3e} at {int(gpu.argmax())}"


@pytest.mark.parametrize("c", ac.ALL_CASES, ids=ids)
def test_row_figure_against_float64(c):
    """Every family on plain operands (a random key bias with a removed tail on the bias kernels); ``plain`` again with
    packed / strided operands and a caller's softmax_scale."""
    bias = ac.soft_bias(c).to(DEV) if c.bias else None
    for family in ac.FAMILIES:
        q, k, v = ac.family_inputs(c, family)
        qd, kd, vd = _place(c, q, k, v)
        counter = _counter()
        _figures(c, family, qd, qd, kd, vd, bias, f"{ids(c)} {family}", redo_counter=counter)
        if c.kid in (3, 6):
            # only the planted +320 nats leave the steady range: at least row 100's item of every (batch, head) is redone
            n = int(counter.item())
            assert n >= c.B * c.H if (family == "late_max" and c.Lk > 70) else n == 0, (family, n)
    q, k, v = ac.family_inputs(c, "plain", seed=1)
    qd, kd, vd = _place(c, q, k, v, packed=True)
    _figures(c, "plain", qd, qd, kd, vd, bias, f"{ids(c)} plain packed scale", scale=0.9 / math.sqrt(c.dh))
    for key in sorted(k_ for k_ in _WORST if k_[0] == c.kid):
        r, g, ratio = _WORST[key]
        print(f"WORST so far, kernel {key[0]} {key[1]}: restatement {r:.3e}, GPU {g:.3e}, worst ratio {ratio:.2f}")


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
@pytest.mark.parametrize("c", _on_load_cases(), ids=ids)
def test_row_figure_q_on_load(c, per_sample):
    """q finished on load with random tables, against the float64 truth built from the raw q, the weight and the tables by
    the oracle's expressions (``finish_q``): the row factor and the per-64 partial sums."""
    eps = 1e-6
    raw, w, cos, sin, rows = (t.to(DEV) if torch.is_tensor(t) else t for t in ac.random_q_on_load(c, per_sample=per_sample))
    q, k, v = ac.family_inputs(c, "plain", seed=2)
    _, kd, vd = _place(c, q, k, v)
    bias = ac.soft_bias(c).to(DEV) if c.bias else None
    q_truth = ac.finish_q(raw, w, eps, cos, sin, c.B, c.Lq, c.H, c.dh)
    q4 = raw.view(c.B, c.Lq, c.H, c.dh)
    for factor in (_row_factor(raw, eps), ac.partial_sums(raw)):
        _figures(c, "q_on_load", q_truth, q4, kd, vd, bias, f"{ids(c)} q on load, period {rows}, factor {tuple(factor.shape)}",
                 on_load=(raw, w, eps, cos, sin), q_norm=(factor, w, eps), rope=(cos, sin, rows))
