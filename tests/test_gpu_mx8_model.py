"""``Transformer3DModel.quantize_ff()`` on a real MI355X: the feed-forward pair of every block in MX-FP8 (quantise(norm) -> FF1 with
GELU, written as MX-FP8 -> FF2 with gate + residual, or a plain bf16 output on the fp32 stream).

Truth: ``oracle/dit.py`` in float64 with its ``leaves`` feed-forward functions patched to quantise and de-quantise (the
restatement of tests/mx8_cases.py) where the product does -- FF1's input and weight, FF1's output after the GELU, FF2's weight --
as tests/test_gpu_lora.py patches them for adapters.  Yardstick: the same patched oracle run in bf16.  Assertion:
``assert_parity`` and ``RTOL`` of tests/test_gpu_model.py.  With ``mixed=True`` the oracle is tests/mixed_oracle.py, whose
residual stream is fp32 by construction: its truth runs every linear in fp32 (as tests/test_gpu_mixed.py and test_gpu_lora.py
take it), patched the same way.

Precision cost, printed and capped: the quantised model against the UNPATCHED fp32 oracle may err by at most
(patched float64 against unpatched float64, computed here: what the number format itself costs) + (the bf16 model's own error
against the unpatched fp32 oracle) + RTOL.

Also: ``unquantize_ff()`` restores the bits of the never-quantised model, a model that was never quantised runs the calls it
ran (``ops.gemm_mx8`` is not reached), ``keep_bf16=False`` computes the same bits from freed weights, an in-place edit of a
weight quantises again, ``quantize_ff()`` after ``fuse_lora`` quantises the fused weights, and every refusal raises."""
import pytest
import torch
import torch.nn.functional as F

import lora_cpu_cases as lcases
import mixed_oracle
import mx8_cases as mc
from test_gpu_model import BF, DEV, RTOL, _Holder, assert_parity, build_model, dit_case, rel

pytestmark = pytest.mark.gpu


def _qdq(v):
    """quantise -> de-quantise along the last axis, in v's dtype (exact there: 4 significant bits times a power of two)."""
    v2 = v.reshape(-1, v.shape[-1])
    s = mc.scale_bytes_real(v2)
    return mc.dequantize(mc.quantize_elements(v2, s), s).to(v.dtype).reshape(v.shape)


def _patch(mp):
    from oracle import leaves
    base_linear, base_gelu = leaves.linear, leaves.gelu_proj
    wq = {}

    def weight(sd, p):
        key = (p, sd[p + "weight"].dtype)
        if key not in wq:
            wq[key] = _qdq(sd[p + "weight"])
        return wq[key]

    def linear(x, sd, p):
        if p.endswith("ff.net.0.proj."):
            return F.linear(_qdq(x), weight(sd, p), sd.get(p + "bias"))
        if p.endswith("ff.net.2."):                       # its input is FF1's output, quantised by gelu_proj below
            return F.linear(x, weight(sd, p), sd.get(p + "bias"))
        return base_linear(x, sd, p)

    mp.setattr(leaves, "linear", linear)
    mp.setattr(leaves, "gelu_proj", lambda x, sd, p, approximate="tanh": _qdq(base_gelu(x, sd, p, approximate)))


def _oracle(c, dtype, mixed=False):
    """The oracle on the device in ``dtype`` (mixed: the linears in ``dtype``, the stream fp32)."""
    from oracle import dit
    cfg, sd32, (x, enc, mask, ts, frac, grid), okw = c["cfg"], c["sd32"], c["inputs"], c["okw"]
    if mixed:
        return mixed_oracle.run(sd32, cfg, x, enc, mask, ts, frac, grid, dtype, DEV, **okw)
    sd = {k: v.to(device=DEV, dtype=dtype) for k, v in sd32.items()}
    fc = tuple(t.to(DEV) for t in dit.precompute_freqs_cis(frac, cfg, dtype))
    kw = dict(okw)
    if kw.get("skip_layer_mask") is not None:
        kw["skip_layer_mask"] = kw["skip_layer_mask"].to(device=DEV, dtype=dtype)
    return dit.transformer3d_forward(sd, cfg, x.to(device=DEV, dtype=dtype), fc, enc.to(device=DEV, dtype=dtype), ts.to(DEV),
                                     encoder_attention_mask=mask.to(DEV), latent_shape=grid, **kw).cpu()


def _forward(c, mixed=False):
    m, (x, enc, mask, ts, frac, grid) = c["m"], c["inputs"]
    with torch.no_grad():
        return m(x.float().to(DEV) if mixed else x.to(DEV), freqs_cis=m.precompute_freqs_cis(frac.to(DEV)),
                 encoder_hidden_states=enc.to(DEV), encoder_attention_mask=mask.to(DEV), timestep=ts.to(DEV), latent_shape=grid,
                 ltxv_model=_Holder(), mixed=mixed, return_dict=False, **c["mkw"])[0]


_CASES = {}


def _case(name):
    """2b: one block at the 2B widths (32 x 64, FF 8192, caption 4096), N 624, B_eff 3 with the STG row.  2b4: four such layers,
    the STG row perturbed in layer 2.  13b: one block at the 13B widths (32 x 128, FF 16384), N 1040, B 2."""
    if name not in _CASES:
        import ltxmi
        from oracle import dit
        heads_dh, layers, grid, B, skip = {"2b": ((32, 64), 1, (3, 13, 16), 3, [0]), "2b4": ((32, 64), 4, (3, 13, 16), 3, [2]),
                                           "13b": ((32, 128), 1, (5, 13, 16), 2, None)}[name]
        cfg, sd32, x, enc, mask, ts, frac = dit_case(*heads_dh, layers, grid, B, 128, caption=4096, seed=16)
        m = build_model(cfg, sd32)
        okw, mkw = {}, {}
        if skip is not None:
            okw = dict(skip_layer_mask=dit.create_skip_layer_mask(layers, 1, 3, 2, skip, torch.float32),
                       skip_layer_strategy=dit.ATTENTION_VALUES)
            mkw = dict(skip_layer_mask=m.create_skip_layer_mask(1, 3, 2, skip), skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues)
        _CASES.clear()                                   # one case's model and weights at a time
        _CASES[name] = dict(cfg=cfg, sd32=sd32, inputs=(x, enc, mask, ts, frac, grid), m=m, okw=okw, mkw=mkw)
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _CASES.clear()


@pytest.mark.parametrize("name,mixed", [("2b", False), ("2b4", False), ("2b", True), ("2b4", True), ("13b", False)])
def test_quantised_feed_forward_against_the_patched_oracle(name, mixed, monkeypatch):
    c = _case(name)
    m = c["m"]
    hi = torch.float32 if mixed else torch.float64
    plain_hi, plain32 = _oracle(c, hi, mixed), _oracle(c, torch.float32, mixed)
    base = _forward(c, mixed)
    assert not m.ff_quantized
    with monkeypatch.context() as mp:
        _patch(mp)
        truth, eager = _oracle(c, hi, mixed), _oracle(c, BF, mixed)
    m.quantize_ff()
    try:
        assert m.ff_quantized
        out = _forward(c, mixed)
        what = f"{name}{' mixed' if mixed else ''}, feed-forward in MX-FP8"
        assert rel(out, base) > 1e-3, "quantize_ff() did nothing"
        assert_parity(out, truth, eager, what)
        format_cost, bf16_err, ours = rel(truth, plain_hi), rel(base, plain32), rel(out, plain32)
        print(f"{what}: precision cost: rel L2 against the UNPATCHED fp32 oracle {ours:.3e} (the bf16 model {bf16_err:.3e}; the "
              f"format alone, patched against unpatched oracle, {format_cost:.3e}); cap {format_cost + bf16_err + RTOL:.3e}")
        assert ours <= format_cost + bf16_err + RTOL
        assert torch.equal(_forward(c, mixed), out), "two quantised forwards differ"
    finally:
        m.unquantize_ff()
    assert not m.ff_quantized
    assert torch.equal(_forward(c, mixed), base), "unquantize_ff() does not restore the output"


def test_unquantised_model_runs_the_calls_it_ran():
    """Never quantised, and quantised then unquantised: no MX-FP8 launch, the same bits."""
    from ltxmi import ops
    c = _case("2b")
    m = c["m"]
    base, base_mixed = _forward(c), _forward(c, True)
    seen = []
    real_q, real_g = ops.quantize_mx8, ops.gemm_mx8
    ops.quantize_mx8 = lambda *a, **k: (seen.append("q"), real_q(*a, **k))[1]
    ops.gemm_mx8 = lambda *a, **k: (seen.append("g"), real_g(*a, **k))[1]
    try:
        assert torch.equal(_forward(c), base) and not seen
        m.quantize_ff()
        _forward(c)
        assert seen.count("g") == 2 and seen.count("q") == 3          # FF1, FF2; two weights once, the activations
        _forward(c)
        assert seen.count("g") == 4 and seen.count("q") == 4          # the weights come from the cache
        m.unquantize_ff()
        del seen[:]
        assert torch.equal(_forward(c), base) and torch.equal(_forward(c, True), base_mixed) and not seen
    finally:
        ops.quantize_mx8, ops.gemm_mx8 = real_q, real_g
        if m.ff_quantized:
            m.unquantize_ff()
    assert set(m.state_dict()) == set(c["sd32"])


def test_keep_bf16_tracks_the_weights_and_keep_false_frees_them():
    c = _case("2b")
    m = c["m"]
    ff = m.transformer_blocks[0].ff
    sd_before = {k: v.clone() for k, v in m.state_dict().items()}
    m.quantize_ff()
    out = _forward(c)
    assert all(torch.equal(v, sd_before[k]) for k, v in m.state_dict().items()), "state_dict() changed under keep_bf16=True"
    # an in-place edit of a weight quantises again, and undoing it gives the first bits back
    w = ff.net[2].weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(0.5)
    assert rel(_forward(c), out) > 1e-3
    with torch.no_grad():
        w.copy_(saved)
    assert torch.equal(_forward(c), out)
    m.unquantize_ff()
    # keep_bf16=False: the same bits, the bf16 weights gone, and the three calls raise, naming themselves
    m.quantize_ff(keep_bf16=False)
    assert ff.net[0].proj.weight.numel() == 0 and ff.net[2].weight.numel() == 0 and ff.net[2].bias.numel() == 2048
    assert torch.equal(_forward(c), out)
    for call, word in ((m.unquantize_ff, "unquantize_ff"), (m.state_dict, "state_dict"),
                       (lambda: m.load_state_dict(c["sd32"]), "load_state_dict")):
        with pytest.raises(RuntimeError, match=word + r"\(\).*keep_bf16=False"):
            call()
    with pytest.raises(RuntimeError, match="quantised already"):
        m.quantize_ff()
    _CASES.clear()                                       # this model cannot be given back


def test_lora_and_the_quantised_feed_forward(monkeypatch):
    from ltxmi import loading, lora
    c = _case("2b")
    m = c["m"]
    cfg = c["cfg"]
    full = loading.load_lora(lcases.make_adapter_sd(cfg, 16, seed=5))
    attn_only = lora.LoraAdapter({p: v for p, v in full.modules.items() if ".ff." not in p})
    ff_only = lora.LoraAdapter({p: v for p, v in full.modules.items() if ".ff." in p})
    assert len(ff_only.modules) == 2 and len(attn_only.modules) == 8
    # quantize_ff() after fuse_lora quantises the FUSED weights: the oracle gets them merged (bf16, as the model holds them)
    m.fuse_lora(full, weight=0.5, name="f")
    fused_sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    m.quantize_ff()
    out = _forward(c)
    with monkeypatch.context() as mp:
        _patch(mp)
        cf = dict(c, sd32=fused_sd)
        truth, eager = _oracle(cf, torch.float64), _oracle(cf, BF)
    assert_parity(out, truth, eager, "2b, r16 fused, then feed-forward in MX-FP8")
    # on a quantised model an adapter that names a feed-forward linear is refused; one on the attention linears runs
    for call in (lambda: m.attach_lora(full), lambda: m.attach_lora(ff_only), lambda: m.fuse_lora(ff_only, name="g")):
        with pytest.raises(RuntimeError, match=r"unquantize_ff\(\) first"):
            call()
    assert m.lora_names() == [] and m.fused_lora_names() == ["f"]
    m.attach_lora(attn_only, weight=2.0, name="a")
    assert rel(_forward(c), out) > 1e-3
    m.detach_lora()
    assert torch.equal(_forward(c), out)
    # unfusing re-merges the bf16 weights in place: the quantised weights follow
    m.unfuse_lora()
    m.unquantize_ff()
    base = _forward(c)
    m.quantize_ff()
    q_base = _forward(c)
    m.fuse_lora(attn_only, name="h")
    m.unfuse_lora()
    assert torch.equal(_forward(c), q_base)
    m.unquantize_ff()
    assert torch.equal(_forward(c), base)
    # and the other way round: an adapter attached to the feed-forward has to go first
    m.attach_lora(ff_only, name="b")
    with pytest.raises(RuntimeError, match=r"detach_lora\(\) first"):
        m.quantize_ff()
    m.detach_lora()
    assert not m.ff_quantized
