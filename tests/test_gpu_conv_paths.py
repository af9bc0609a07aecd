"""ltxmi_conv3d_ndhwc_bf16 on a real MI355X, route by route: every case of tests/conv_cases.py asserts the route the library
would take, runs into outputs (and a split workspace) that lie inside sentinel-filled buffers, and is judged against the float64
truth by the three metrics of that module -- or, in the exact family, bit for bit."""
import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _on_device(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


def _run(c, d, algo=None):
    """One guarded call -> (raw or None, activated or None).  The route is asserted first; afterwards the sentinels around y,
    y_norm and the workspace are intact and no input has changed."""
    from ltxmi import ops
    kw, bufs = cc.call_args(c, d, algo=algo)
    r = ops.conv3d_route(**kw)
    assert isinstance(r, dict) and not r.pop("second_launch"), r
    if algo is None:
        assert r == c["want"], (r, c["want"])
    else:
        assert r["route"] != c["want"]["route"], r
    before = {k: v.clone() for k, v in d.items() if torch.is_tensor(v)}
    out = ops.conv3d(**kw)
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert cc.guards_intact(buf), f"{name}: written outside the tensor"
    for k, v in before.items():
        assert torch.equal(d[k], v), f"input {k} changed"
    if c["norm"] == "second":
        assert out[0].data_ptr() == bufs["y"][1].data_ptr() and out[1].data_ptr() == bufs["y_norm"][1].data_ptr()
        return out
    assert out.data_ptr() == bufs["y"][1].data_ptr()
    return (None, out) if c["norm"] == "only" else (out, None)


@pytest.mark.parametrize("c", cc.GPU_CASES, ids=cc.case_id)
def test_conv_route(c):
    what = cc.case_id(c)
    d_cpu = cc.make(c)
    d = _on_device(d_cpu)
    raw, act = _run(c, d)
    if c["want"]["ksplit"] > 1:                    # the finalising pass sums the ranges in range order: the same bits every time
        raw2, act2 = _run(c, d)
        assert all(a is None or torch.equal(a, b) for a, b in ((raw, raw2), (act, act2))), f"{what}: two runs differ"
    if c["judge"] == "whole":
        t, mag = cc.truth(c)
        if c["norm"] == "only":
            cc.compare(act, t, mag, what=what + " activated")
        elif c["family"] == "exact":
            assert cc.exact_ok(t)
            bad = raw.float() != t.to(DEV)
            assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact truth, first at "
                                         f"{bad.nonzero()[0].tolist()}: {float(raw[bad][0])} for {float(t.to(DEV)[bad][0])}")
        else:
            cc.compare(raw, t, mag, what=what)
        if c["norm"] == "second":                  # the norm of the raw output's own bf16 values
            ta, maga = cc.norm_op(raw, d, cc.F64)
            cc.compare(act, ta, maga, what=what + " activated")
        return
    assert c["family"] == "plain" and c["norm"] is None
    magmax = 0.0
    for sl in cc.crops(c):
        t, mag, sel = cc.crop_truth(c, d_cpu, sl)
        cc.compare(raw[sel], t, mag, what=f"{what} crop {[s.start for s in sl[0]]}")
        magmax = max(magmax, float(mag.max()))
    if c["versus"] is not None:
        # The whole tensor against another route: two bf16 roundings of two fp32 sums of the same products.  Per element they
        # differ by at most one bf16 ulp of the larger (2^-7 of it) plus twice the slack on the sum of magnitudes, bounded by 1.5 x
        # the largest seen in the crops (a sum of K >= 576 independent |x w|: its spread is a few per cent); whole tensor: check.
        other, _ = _run(c, d, algo=c["versus"])
        a, b = raw.double(), other.double()
        lim = 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 2 * cc.SLACK * 1.5 * magmax
        worst = float(((a - b).abs() / lim).max())
        print(f"{what} vs algo {c['versus']}: elem {worst:.3f}")
        assert worst <= 1.0, f"{what}: differs from algo {c['versus']} by {worst:.3f} of the limit"
        check, _, _ = cc._check()
        check(raw, other.float(), what=f"{what} vs algo {c['versus']}")
