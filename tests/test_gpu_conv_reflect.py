"""ltxmi_conv3d_ndhwc_bf16 with spatial padding mode 2 (reflect) on a real MI355X, route by route: the harness of
tests/test_gpu_conv_paths.py on the cases of tests/conv_reflect_cases.py.  Every case asserts the route first (its replicate
twin's), runs into outputs and a workspace that lie inside sentinel-filled buffers, leaves its inputs unchanged, and is judged
against the reflect truth -- bit for bit in the exact family (where a call that replicated instead differs on every border
position), by the three metrics of tests/conv_cases.py otherwise."""
import pytest
import torch

import conv_cases as cc
import conv_reflect_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(c, d):
    """One guarded call -> (raw or None, activated or None)."""
    from ltxmi import ops
    kw, bufs = rc.call_args(c, d)
    r = ops.conv3d_route(**kw)
    assert isinstance(r, dict) and not r.pop("second_launch"), r
    assert r == c["want"], (r, c["want"])
    before = {k: v.clone() for k, v in d.items() if torch.is_tensor(v)}
    out = ops.conv3d(**kw)
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert rc.guards_intact(buf), f"{name}: written outside the tensor"
    for k, v in before.items():
        assert torch.equal(d[k], v), f"input {k} changed"
    if c["norm"] == "second":
        assert out[0].data_ptr() == bufs["y"][1].data_ptr() and out[1].data_ptr() == bufs["y_norm"][1].data_ptr()
        return out
    assert out.data_ptr() == bufs["y"][1].data_ptr()
    return (None, out) if c["norm"] == "only" else (out, None)


@pytest.mark.parametrize("c", rc.GPU_CASES, ids=rc.case_id)
def test_conv_reflect_route(c):
    what = rc.case_id(c)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in rc.make(c).items()}
    raw, act = _run(c, d)
    if c["want"]["ksplit"] > 1:                    # the finalising pass sums the ranges in range order: the same bits every time
        raw2, act2 = _run(c, d)
        assert all(a is None or torch.equal(a, b) for a, b in ((raw, raw2), (act, act2))), f"{what}: two runs differ"
    t, mag = rc.truth(c)
    if c["norm"] == "only":
        rc.compare(act, t, mag, what=what + " activated")
    elif c["family"] == "exact":
        assert rc.exact_ok(t)
        bad = raw.float() != t.to(DEV)
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact truth, first at "
                                     f"{bad.nonzero()[0].tolist()}: {float(raw[bad][0])} for {float(t.to(DEV)[bad][0])}")
    else:
        rc.compare(raw, t, mag, what=what)
    if c["norm"] == "second":                      # the norm of the raw output's own bf16 values
        ta, maga = cc.norm_op(raw, d, cc.F64)
        rc.compare(act, ta, maga, what=what + " activated")


def test_reflect_with_a_single_row_is_refused_before_any_launch():
    from ltxmi import ops
    from ltxmi._lib import LtxmiError
    c = cc._case((1, 2, 1, 5), 64, 8, cc.G128, family="plain")
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in cc.make(c).items()}
    kw, bufs = rc.call_args(c, d)
    assert ops.conv3d_route(**kw) == -1
    with pytest.raises(LtxmiError, match="reflect"):
        ops.conv3d(**kw)
    torch.cuda.synchronize()
    assert bool((bufs["y"][0] == cc.SENTINEL).all())               # nothing ran
    assert isinstance(ops.conv3d_route(**dict(kw, pad_replicate=ops.PAD_REPLICATE)), dict)
