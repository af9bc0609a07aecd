"""``Transformer3DModel.quantize_attention()`` on a real MI355X: the per-step attention linears of every block in MX-FP8 (the packed
attn1 q/k/v projection fed by the fused norm + quantise, attn1.to_out, attn2.to_q, attn2.to_out; ltxmi/attn_mx8.py).

Recipe, cases and assertions are those of tests/test_gpu_mx8_model.py (2b, 2b4, 2b mixed, 13b).  Truth: ``oracle/dit.py`` in float64
with ``leaves.linear`` patched to quantise and de-quantise (the restatement of tests/mx8_cases.py) the input and the weight of
attn1.to_q / to_k / to_v, attn1.to_out.0, attn2.to_q and attn2.to_out.0 -- attn2.to_k / to_v are left alone, as the product leaves
them bf16.  Yardstick: the same patched oracle in bf16.  ``assert_parity`` and ``RTOL`` of tests/test_gpu_model.py.  With
``mixed=True`` the oracle is tests/mixed_oracle.py, its linears in fp32 for the truth.

Precision cost, printed and capped as there: the quantised model against the UNPATCHED fp32 oracle may err by at most
(patched against unpatched truth: what the format itself costs) + (the bf16 model's own error) + RTOL.  Every case also runs with
``quantize_ff()`` on, both patches applied.

Also: a never-quantised model reaches neither new op and computes the same bits; ``ops.gemm_mx8`` is launched exactly once per
chosen linear and block for every ``linears`` subset; ``keep_bf16=False`` computes the same bits from freed weights and the three
calls raise; an in-place weight edit quantises again; ``fuse_lora`` then ``quantize_attention`` matches a model loaded on the merged
weights and then quantised; every LoRA and sequence-parallel refusal raises; an adapter on attn2.to_k / to_v still runs."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import lora_cpu_cases as lcases
from test_gpu_model import BF, RTOL, assert_parity, build_model, rel
from test_gpu_mx8_model import _CASES, _case, _forward, _oracle, _patch as _patch_ff, _qdq

pytestmark = pytest.mark.gpu

LINEARS = ("attn1.qkv", "attn1.to_out", "attn2.to_q", "attn2.to_out")
ORACLE_PATHS = {"attn1.qkv": ("attn1.to_q.", "attn1.to_k.", "attn1.to_v."), "attn1.to_out": ("attn1.to_out.0.",),
                "attn2.to_q": ("attn2.to_q.",), "attn2.to_out": ("attn2.to_out.0.",)}
_plain = {}          # (case, mixed) -> (unpatched truth, unpatched fp32 oracle, the bf16 model's output)


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _CASES.clear()
    _plain.clear()


def _patch(mp, linears=LINEARS, ff=False):
    """Quantise and de-quantise the input and the weight of the oracle's linears that ``linears`` names (and the feed-forward's)."""
    from oracle import leaves
    if ff:
        _patch_ff(mp)
    base_linear = leaves.linear
    ends = tuple(e for n in linears for e in ORACLE_PATHS[n])
    wq = {}

    def linear(x, sd, p):
        if not p.endswith(ends):
            return base_linear(x, sd, p)
        key = (p, sd[p + "weight"].dtype)
        if key not in wq:
            wq[key] = _qdq(sd[p + "weight"])
        return F.linear(_qdq(x), wq[key], sd.get(p + "bias"))

    mp.setattr(leaves, "linear", linear)


def _plain_runs(name, mixed):
    c = _case(name)
    if (name, mixed) not in _plain:
        for k in [k for k in _plain if k[0] != name]:
            del _plain[k]
        hi = torch.float32 if mixed else torch.float64
        _plain[(name, mixed)] = (_oracle(c, hi, mixed), _oracle(c, torch.float32, mixed), _forward(c, mixed))
    return (c,) + _plain[(name, mixed)]


@pytest.mark.parametrize("ff", [False, True], ids=["attention", "attention+ff"])
@pytest.mark.parametrize("name,mixed", [("2b", False), ("2b4", False), ("2b", True), ("2b4", True), ("13b", False)])
def test_quantised_attention_against_the_patched_oracle(name, mixed, ff, monkeypatch):
    from ltxmi import ops
    c, plain_hi, plain32, base = _plain_runs(name, mixed)
    m = c["m"]
    layers = len(m.transformer_blocks)
    hi = torch.float32 if mixed else torch.float64
    assert not m.attention_quantized and not m.ff_quantized
    with monkeypatch.context() as mp:
        _patch(mp, ff=ff)
        truth, eager = _oracle(c, hi, mixed), _oracle(c, BF, mixed)
    m.quantize_attention(linears=LINEARS)
    if ff:
        m.quantize_ff()
    launches = []
    real = ops.gemm_mx8
    ops.gemm_mx8 = lambda *a, **k: (launches.append(1), real(*a, **k))[1]
    try:
        assert m.attention_quantized and m.ff_quantized == ff
        out = _forward(c, mixed)
        assert len(launches) == (4 + 2 * ff) * layers, len(launches)
        what = f"{name}{' mixed' if mixed else ''}, attention linears{' and feed-forward' if ff else ''} in MX-FP8"
        assert rel(out, base) > 1e-3, "quantize_attention() did nothing"
        assert_parity(out, truth, eager, what)
        format_cost, bf16_err, ours = rel(truth, plain_hi), rel(base, plain32), rel(out, plain32)
        print(f"{what}: precision cost: rel L2 against the UNPATCHED fp32 oracle {ours:.3e} (the bf16 model {bf16_err:.3e}; the "
              f"format alone, patched against unpatched oracle, {format_cost:.3e}); cap {format_cost + bf16_err + RTOL:.3e}")
        assert ours <= format_cost + bf16_err + RTOL
        assert torch.equal(_forward(c, mixed), out), "two quantised forwards differ"
    finally:
        ops.gemm_mx8 = real
        m.unquantize_attention()
        if ff:
            m.unquantize_ff()
    assert not m.attention_quantized
    assert torch.equal(_forward(c, mixed), base), "unquantize_attention() does not restore the output"


SUBSETS = [s for r in range(1, 5) for s in itertools.combinations(LINEARS, r)]


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(s))
def test_every_subset_launches_what_it_names_and_matches_its_oracle(subset, monkeypatch):
    from ltxmi import ops
    c, _, _, base = _plain_runs("2b", False)
    m = c["m"]
    with monkeypatch.context() as mp:
        _patch(mp, subset)
        truth, eager = _oracle(c, torch.float64), _oracle(c, BF)
    seen = {"gemm_mx8": 0, "norm_modulate_mx8": 0, "quantize_mx8": 0}
    real = {n: getattr(ops, n) for n in seen}

    def counted(n):
        def f(*a, **k):
            seen[n] += 1
            return real[n](*a, **k)
        return f
    m.quantize_attention(linears=reversed(subset))           # any order, any iterable
    try:
        _forward(c)                                          # the weights are quantised here
        for n in seen:
            setattr(ops, n, counted(n))
        out = _forward(c)
        assert seen["gemm_mx8"] == len(subset), seen
        assert seen["norm_modulate_mx8"] == ("attn1.qkv" in subset), seen
        assert seen["quantize_mx8"] == len(subset) - ("attn1.qkv" in subset), seen      # one activation pass per other linear
        assert_parity(out, truth, eager, "2b, " + " + ".join(subset) + " in MX-FP8")
    finally:
        for n in seen:
            setattr(ops, n, real[n])
        m.unquantize_attention()
    assert torch.equal(_forward(c), base)


def test_unquantised_model_runs_the_calls_it_ran():
    """Never quantised, and quantised then unquantised: neither new op is reached, the same bits."""
    from ltxmi import ops
    c = _case("2b")
    m = c["m"]
    base, base_mixed = _forward(c), _forward(c, True)
    seen = []
    names = ("quantize_mx8", "gemm_mx8", "norm_modulate_mx8")
    real = {n: getattr(ops, n) for n in names}
    for n in names:
        setattr(ops, n, lambda *a, _n=n, **k: (seen.append(_n), real[_n](*a, **k))[1])
    try:
        assert torch.equal(_forward(c), base) and torch.equal(_forward(c, True), base_mixed) and not seen
        m.quantize_ff()                                      # quantize_ff alone: the calls it made before this feature
        _forward(c)
        assert "norm_modulate_mx8" not in seen and seen.count("gemm_mx8") == 2
        m.unquantize_ff()
        m.quantize_attention()
        _forward(c)
        m.unquantize_attention()
        del seen[:]
        assert torch.equal(_forward(c), base) and torch.equal(_forward(c, True), base_mixed) and not seen
    finally:
        for n in names:
            setattr(ops, n, real[n])
        if m.attention_quantized:
            m.unquantize_attention()
    assert set(m.state_dict()) == set(c["sd32"])


def test_attention_skip_strategy_takes_the_bf16_norm():
    """The AttentionSkip blend reads norm1's bf16 output: the block then runs norm_modulate + quantise instead of the fused form,
    and the result is the one the quantised linears give on that input (the same bits as the fused form's by construction)."""
    import ltxmi
    from ltxmi import ops
    c = _case("2b")
    m = c["m"]
    mkw = dict(c["mkw"], skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionSkip)
    cs = dict(c, mkw=mkw)
    m.quantize_attention(linears=LINEARS)
    seen = []
    real = ops.norm_modulate_mx8
    ops.norm_modulate_mx8 = lambda *a, **k: (seen.append(1), real(*a, **k))[1]
    try:
        out = _forward(cs)
        assert not seen and bool(torch.isfinite(out.float()).all())
        _forward(c)
        assert len(seen) == 1
    finally:
        ops.norm_modulate_mx8 = real
        m.unquantize_attention()


def test_keep_bf16_tracks_the_weights_and_keep_false_frees_them():
    c = _case("2b")
    m = c["m"]
    b = m.transformer_blocks[0]
    sd_before = {k: v.clone() for k, v in m.state_dict().items()}
    m.quantize_attention(linears=LINEARS)
    out = _forward(c)
    assert all(torch.equal(v, sd_before[k]) for k, v in m.state_dict().items()), "state_dict() changed under keep_bf16=True"
    for w in (b.attn1.to_k.weight, b.attn1.to_out[0].weight, b.attn2.to_q.weight, b.attn2.to_out[0].weight):
        saved = w.detach().clone()                           # an in-place edit quantises again; undoing it gives the bits back
        with torch.no_grad():
            w.mul_(0.5)
        assert rel(_forward(c), out) > 1e-4
        with torch.no_grad():
            w.copy_(saved)
        assert torch.equal(_forward(c), out)
    with pytest.raises(RuntimeError, match="quantised already"):
        m.quantize_attention()
    m.unquantize_attention()
    # keep_bf16=False on two of the four: the same bits as keep_bf16=True on those two, their weights gone, the others kept
    two = ("attn1.qkv", "attn2.to_out")
    m.quantize_attention(linears=two)
    out2 = _forward(c)
    m.unquantize_attention()
    m.quantize_attention(keep_bf16=False, linears=two)
    freed = [b.attn1.to_q, b.attn1.to_k, b.attn1.to_v, b.attn2.to_out[0]]
    kept = [b.attn1.to_out[0], b.attn2.to_q, b.attn2.to_k, b.attn2.to_v]
    assert all(l.weight.numel() == 0 for l in freed) and all(l.weight.numel() > 0 for l in kept)
    assert b.attn2.to_out[0].bias.numel() == 2048 and "qkv" not in b.attn1.derived_slots()
    assert torch.equal(_forward(c), out2) and torch.equal(_forward(c, True), _forward(c, True))
    for call, word in ((m.unquantize_attention, "unquantize_attention"), (m.state_dict, "state_dict"),
                       (lambda: m.load_state_dict(c["sd32"]), "load_state_dict")):
        with pytest.raises(RuntimeError, match=word + r"\(\).*keep_bf16=False"):
            call()
    m.quantize_ff()                                          # composes with the other switch after the fact
    assert bool(torch.isfinite(_forward(c).float()).all())
    _CASES.clear()                                           # this model cannot be given back


def test_lora_and_the_quantised_attention(monkeypatch):
    from ltxmi import loading, lora
    c = _case("2b")
    m = c["m"]
    cfg = c["cfg"]
    full = loading.load_lora(lcases.make_adapter_sd(cfg, 16, seed=5))
    pick = lambda f: lora.LoraAdapter({p: v for p, v in full.modules.items() if f(p)})
    text_kv = pick(lambda p: p.endswith(("attn2.to_k", "attn2.to_v")))
    ff_only = pick(lambda p: ".ff." in p)
    one = {n: pick(lambda p, e=e: p.endswith(e)) for n, e in (("attn1.qkv", "attn1.to_v"), ("attn1.to_out", "attn1.to_out.0"),
                                                               ("attn2.to_q", "attn2.to_q"), ("attn2.to_out", "attn2.to_out.0"))}
    assert len(text_kv.modules) == 2 and len(ff_only.modules) == 2 and all(len(a.modules) == 1 for a in one.values())
    # fuse_lora then quantize_attention == a model loaded on the merged weights, then quantised
    m.fuse_lora(full, weight=0.5, name="f")
    merged = {k: v.float().cpu() for k, v in m.state_dict().items()}
    m.quantize_attention(linears=LINEARS)
    out = _forward(c)
    m2 = build_model(cfg, merged)
    m2.quantize_attention(linears=LINEARS)
    assert torch.equal(_forward(dict(c, m=m2)), out)
    del m2
    with monkeypatch.context() as mp:
        _patch(mp)
        cf = dict(c, sd32=merged)
        assert_parity(out, _oracle(cf, torch.float64), _oracle(cf, BF), "2b, r16 fused, then attention linears in MX-FP8")
    # on a quantised model an adapter that names a quantised linear is refused, attached or fused
    for name, adapter in one.items():
        for call in (lambda: m.attach_lora(adapter), lambda: m.fuse_lora(adapter, name="g"), lambda: m.attach_lora(full)):
            with pytest.raises(RuntimeError, match=r"unquantize_attention\(\) first"):
                call()
    assert m.lora_names() == [] and m.fused_lora_names() == ["f"]
    # adapters on attn2.to_k / to_v and on the feed-forward run as before
    for adapter in (text_kv, ff_only):
        m.attach_lora(adapter, weight=2.0, name="a")
        assert rel(_forward(c), out) > 1e-4
        m.detach_lora()
        assert torch.equal(_forward(c), out)
    # unfusing re-merges the bf16 weights in place: the quantised weights follow
    m.unfuse_lora()
    m.unquantize_attention()
    base = _forward(c)
    # a linear left out of the choice takes adapters; the chosen ones refuse
    m.quantize_attention(linears=("attn1.qkv", "attn2.to_q"))
    q_base = _forward(c)
    m.attach_lora(one["attn1.to_out"], weight=2.0, name="o")
    assert rel(_forward(c), q_base) > 1e-4
    m.detach_lora()
    with pytest.raises(RuntimeError, match=r"unquantize_attention\(\) first"):
        m.attach_lora(one["attn2.to_q"])
    m.fuse_lora(one["attn2.to_out"], name="h")
    m.unfuse_lora()
    assert torch.equal(_forward(c), q_base)
    m.unquantize_attention()
    assert torch.equal(_forward(c), base)
    # and the other way round: an adapter attached to a chosen linear has to go first; one elsewhere does not matter
    m.attach_lora(one["attn1.qkv"], name="b")
    with pytest.raises(RuntimeError, match=r"detach_lora\(\) first"):
        m.quantize_attention()
    m.quantize_attention(linears=("attn1.to_out", "attn2.to_q", "attn2.to_out"))
    assert bool(torch.isfinite(_forward(c).float()).all())
    m.unquantize_attention()
    m.detach_lora()
    assert not m.attention_quantized and torch.equal(_forward(c), base)


def test_sequence_parallel_paths_refuse_a_quantised_attention():
    from ltxmi import distributed
    c = _case("2b")
    m = c["m"]
    m.quantize_attention(linears=("attn2.to_q",))            # attn1 itself untouched: the block's hook still refuses
    try:
        for mode, who in (("ulysses", "UlyssesAttnProcessor"), ("ring", "RingAttnProcessor")):
            distributed.enable_sequence_parallel(m, mode=mode)
            try:
                with pytest.raises(NotImplementedError, match=who + r".*quantize_attention\(\)"):
                    _forward(c)
            finally:
                distributed.disable_sequence_parallel(m)
        x, enc, mask, ts, frac, grid = c["inputs"]
        with pytest.raises(NotImplementedError, match=r"usp_dit_forward.*quantize_attention\(\)"):
            distributed.usp_dit_forward(m, x, None)
    finally:
        m.unquantize_attention()
    # and quantize_attention refuses a model whose processors are the sequence-parallel ones
    distributed.enable_sequence_parallel(m)
    try:
        with pytest.raises(NotImplementedError, match="UlyssesAttnProcessor"):
            m.quantize_attention()
        assert not m.attention_quantized
    finally:
        distributed.disable_sequence_parallel(m)
