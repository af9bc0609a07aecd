"""``attach_lora(..., mx8=True)`` without a device: which slots become MX-FP8 pairs and which stay bf16 for every ``linears``
choice of ``quantize_attention`` with and without ``quantize_ff``, stacking and padding of the rank to 128, the packed
projection's groups, the life cycle, the unchanged refusals of ``mx8=False`` and ``keep_bf16=False`` models.  The quantised
state is set through the state objects and ``ops.quantize_mx8`` is the CPU restatement of tests/mx8_cases.py
(tests/test_gpu_lora_mx8_model.py holds the rest on the MI355X)."""
import itertools

import pytest
import torch

import mx8_cases as mc
from test_mx8_model_cpu import _model

BF = torch.bfloat16
D, LAYERS = 256, 2
MX_SLOT = {"attn1.qkv": ("attn1", "qkv"), "attn1.to_out": ("attn1", "out"), "attn2.to_q": ("attn2", "q"), "attn2.to_out": ("attn2", "out")}
ALL_SLOTS = [("attn1", "qkv"), ("attn1", "out"), ("attn2", "q"), ("attn2", "kv"), ("attn2", "out"), ("ff", "ff1"), ("ff", "ff2")]


@pytest.fixture(autouse=True)
def _cpu_quantiser(monkeypatch):
    from ltxmi import ops
    monkeypatch.setattr(ops, "quantize_mx8", lambda x, out=None: mc.quantize(x))


def _adapter(m, r, seed=0, alpha=None, only=None):
    from ltxmi import lora
    g = torch.Generator().manual_seed(seed)
    mods = {}
    for i, b in enumerate(m.transformer_blocks):
        for t in lora.BLOCK_TARGETS:
            if only is not None and t not in only:
                continue
            n, k = {"ff.net.0.proj": (4 * D, D), "ff.net.2": (D, 4 * D)}.get(t, (D, D))
            mods[f"transformer_blocks.{i}.{t}"] = (torch.randn(r, k, generator=g).to(BF), torch.randn(n, r, generator=g).to(BF), alpha)
    return lora.LoraAdapter(mods)


def _mark(m, chosen, ff):
    """The state ``quantize_attention(linears=chosen)`` / ``quantize_ff()`` leave, without their launches."""
    from ltxmi import attn_mx8, ff_mx8
    chosen = attn_mx8.resolve(chosen)
    for b in m.transformer_blocks:
        for owner in ("attn1", "attn2"):
            which = {attn_mx8.PARTS[n][1] for n in chosen if attn_mx8.PARTS[n][0] == owner}
            if which:
                getattr(b, owner).__dict__["_mx8"] = attn_mx8.AttnState("proj" in which, "out" in which)
        if ff:
            b.ff.__dict__["_mx8"] = ff_mx8.FFState()
    if chosen:
        m.__dict__["_mx8_attn_linears"] = chosen
    return chosen


def _slots(m, i=0):
    b = m.transformer_blocks[i]
    return {(o, n): s for o in ("attn1", "attn2", "ff") for n, s in (getattr(b, o).__dict__.get("_lora") or {}).items()}


SUBSETS = [s for r in range(0, 5) for s in itertools.combinations(MX_SLOT, r)]


@pytest.mark.parametrize("ff", [False, True], ids=["bf16-ff", "mx8-ff"])
@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(s) or "none")
def test_which_slots_become_mx8_pairs(subset, ff):
    from ltxmi import lora
    m = _model(heads=4, dh=64, layers=LAYERS)
    _mark(m, subset, ff)
    m.attach_lora(_adapter(m, 16), mx8=True)
    want_mx = {MX_SLOT[n] for n in subset} | ({("ff", "ff1"), ("ff", "ff2")} if ff else set())
    for i in range(LAYERS):
        slots = _slots(m, i)
        assert set(slots) == set(ALL_SLOTS)
        for key, s in slots.items():
            assert isinstance(s, lora.LoraSlotMx8 if key in want_mx else lora.LoraSlot), (key, type(s).__name__)
            assert lora.runs_mx8(getattr(m.transformer_blocks[i], key[0]), key[1]) == (key in want_mx)
    assert ("attn2", "kv") not in want_mx                 # attn2.to_k / to_v stay on the bf16 pair


def test_stacking_padding_and_groups():
    from ltxmi import lora
    m = _model(heads=4, dh=64, layers=1)
    _mark(m, ("attn1.qkv", "attn2.to_out"), True)
    a16, a128 = _adapter(m, 16, seed=1), _adapter(m, 128, seed=2, alpha=64.0)
    m.attach_lora(a16, weight=0.5, name="a", mx8=True)
    m.attach_lora(a128, weight=2.0, name="b", mx8=True)
    slots = _slots(m)
    qkv, ff2, out1 = slots[("attn1", "qkv")], slots[("ff", "ff2")], slots[("attn1", "out")]
    # 16 + 128 = 144 -> 256 in MX-FP8 (a K-tile is 128), 192 in bf16 (64)
    assert qkv.down[0].shape == (3 * 256, D) and qkv.down[1].shape == (3 * 256, D // 32) and qkv.down[0].dtype == mc.E4M3
    assert qkv.up[0].shape == (3 * D, 256) and qkv.up[1].shape == (3 * D, 8) and qkv.group_cols == D
    assert ff2.down[0].shape == (256, 4 * D) and ff2.up[0].shape == (D, 256) and ff2.group_cols == 0
    assert out1.down.shape == (192, D) and out1.up.shape == (D, 192) and out1.down.dtype == BF
    # the stacked operands quantised as one: member g's rows are [down_a; down_b; zeros], the ups bf16(s up) side by side
    for g, t in enumerate(("attn1.to_q", "attn1.to_k", "attn1.to_v")):
        p = f"transformer_blocks.0.{t}"
        down = torch.cat([a16.modules[p][0], a128.modules[p][0], torch.zeros(112, D, dtype=BF)], 0)
        up = torch.cat([(a16.modules[p][1].float() * a16.scale(p, 0.5)).to(BF), (a128.modules[p][1].float() * a128.scale(p, 2.0)).to(BF),
                        torch.zeros(D, 112, dtype=BF)], 1)
        wq, ws = mc.quantize(down)
        assert torch.equal(qkv.down[0][g * 256:(g + 1) * 256].view(torch.uint8), wq.view(torch.uint8))
        assert torch.equal(qkv.down[1][g * 256:(g + 1) * 256], ws)
        uq, us = mc.quantize(up)
        assert torch.equal(qkv.up[0][g * D:(g + 1) * D].view(torch.uint8), uq.view(torch.uint8)) and torch.equal(qkv.up[1][g * D:(g + 1) * D], us)
        # the padding: scale byte 0, elements 0, exact zeros
        assert bool((qkv.down[0][g * 256 + 144:(g + 1) * 256].view(torch.uint8) == 0).all()) and bool((qkv.down[1][g * 256 + 144:(g + 1) * 256] == 0).all())
        assert bool((qkv.up[0].view(torch.uint8)[:, 144:] == 0).all()) and bool((qkv.up[1][:, 5:] == 0).all())
    assert a128.scale("transformer_blocks.0.attn1.to_q", 2.0) == 1.0
    # a member without an adapter contributes zero blocks
    m.detach_lora()
    m.attach_lora(_adapter(m, 16, only=("attn1.to_k",)), mx8=True)
    qkv = _slots(m)[("attn1", "qkv")]
    assert qkv.down[0].shape == (3 * 128, D)
    assert bool((qkv.down[0][:128].view(torch.uint8) == 0).all()) and bool((qkv.up[1][:D] == 0).all()) and bool((qkv.up[1][2 * D:] == 0).all())
    assert bool((qkv.up[1][D:2 * D, 0] != 0).any())


def test_a_packed_projection_needs_groups_of_256_columns():
    m = _model(heads=2, dh=64, layers=1)                 # D = 128: a tile of 256 columns would span two members
    _mark(m, ("attn1.qkv",), False)
    from ltxmi import lora
    g = torch.Generator().manual_seed(0)
    ad = lora.LoraAdapter({"transformer_blocks.0.attn1.to_q": (torch.randn(8, 128, generator=g).to(BF), torch.randn(128, 8, generator=g).to(BF), None)})
    with pytest.raises(NotImplementedError, match="multiple of 256"):
        m.attach_lora(ad, mx8=True)
    assert m.lora_names() == [] and not _slots(m)


def test_life_cycle_and_unquantize_rebuilds_bf16_slots():
    from ltxmi import lora
    m = _model(heads=4, dh=64, layers=1)
    _mark(m, tuple(MX_SLOT), True)
    ad = _adapter(m, 16, seed=3)
    m.attach_lora(ad, weight=1.0, name="a", mx8=True)
    ep = lora.epoch(m.transformer_blocks[0].ff)
    first = _slots(m)[("ff", "ff1")]
    m.set_lora_weights({"a": 0.5})
    second = _slots(m)[("ff", "ff1")]
    assert lora.epoch(m.transformer_blocks[0].ff) == ep + 1
    assert torch.equal(first.down[0].view(torch.uint8), second.down[0].view(torch.uint8))        # the strength lives in `up`
    assert torch.equal(first.up[0].view(torch.uint8), second.up[0].view(torch.uint8)) and not torch.equal(first.up[1], second.up[1])
    assert m.lora_names() == ["a"]
    # unquantize_ff(): the feed-forward's slots become bf16 ones, the attention's stay
    m.unquantize_ff()
    s = _slots(m)
    assert isinstance(s[("ff", "ff1")], lora.LoraSlot) and isinstance(s[("ff", "ff2")], lora.LoraSlot)
    assert isinstance(s[("attn1", "qkv")], lora.LoraSlotMx8) and s[("ff", "ff1")].down.shape == (64, D)
    m.unquantize_attention()
    assert all(isinstance(v, lora.LoraSlot) for v in _slots(m).values()) and not m.attention_quantized
    # ... and equal what attaching to the unquantised model gives
    fresh = _model(heads=4, dh=64, layers=1)
    fresh.attach_lora(ad, weight=0.5, name="a")
    for key, v in _slots(fresh).items():
        assert torch.equal(v.down, _slots(m)[key].down) and torch.equal(v.up, _slots(m)[key].up) and v.group_cols == _slots(m)[key].group_cols
    m.detach_lora()
    assert not _slots(m) and m.lora_names() == []
    # without adapters an unquantize rebuilds nothing
    _mark(m, ("attn1.qkv",), True)
    ep = lora.epoch(m)
    m.unquantize_ff()
    m.unquantize_attention()
    assert lora.epoch(m) == ep


def test_mx8_false_refuses_as_before_and_quantize_keeps_refusing():
    m = _model(heads=4, dh=64, layers=1)
    chosen = _mark(m, ("attn1.qkv", "attn2.to_out"), True)
    with pytest.raises(RuntimeError, match=r"attach_lora\(\): the feed-forward is quantised and the adapter names ff\.net\.0\.proj / "
                                           r"ff\.net\.2; unquantize_ff\(\) first"):
        m.attach_lora(_adapter(m, 16))
    with pytest.raises(RuntimeError, match=r"attach_lora\(\): the adapter names an attention linear that quantize_attention\(\) runs in "
                                           r"MX-FP8 \(attn1\.qkv, attn2\.to_out\); unquantize_attention\(\) first"):
        m.attach_lora(_adapter(m, 16, only=("attn1.to_k",)))
    m.attach_lora(_adapter(m, 16, only=("attn1.to_out.0", "attn2.to_k")))           # not quantised: bf16, as before
    assert m.lora_names() == ["lora0"]
    m.attach_lora(_adapter(m, 16, seed=4), name="x", mx8=True)
    with pytest.raises(RuntimeError, match=r"unquantize_ff\(\) first"):
        m.fuse_lora(_adapter(m, 16, only=("ff.net.2",)))
    # quantize_* over attached adapters keeps refusing: what it asks (``lora.has_slot``) sees an MX-FP8 slot as it sees a bf16 one,
    # before and after an unquantize (on a host model its device check comes first, so the question is put directly)
    from ltxmi import lora
    b = m.transformer_blocks[0]
    assert isinstance(b.ff.__dict__["_lora"]["ff1"], lora.LoraSlotMx8) and lora.has_slot(b.ff, "ff1") and lora.has_slot(b.attn1, "qkv")
    m.unquantize_ff()
    m.unquantize_attention()
    assert isinstance(b.ff.__dict__["_lora"]["ff1"], lora.LoraSlot) and lora.has_slot(b.ff, "ff1") and lora.has_slot(b.attn1, "qkv")


def test_keep_bf16_false_models_take_mx8_adapters():
    from ltxmi import lora
    m = _model(heads=4, dh=64, layers=1)
    _mark(m, tuple(MX_SLOT), True)
    b = m.transformer_blocks[0]
    held = lambda n, k: (torch.zeros(n, k, dtype=torch.uint8).view(mc.E4M3), torch.zeros(n, k // 32, dtype=torch.uint8))
    b.ff.__dict__["_mx8"].sealed = (held(4 * D, D), held(D, 4 * D))
    b.attn1.__dict__["_mx8"].sealed = {"proj": held(3 * D, D) + (None,), "out": held(D, D) + (None,)}
    b.attn2.__dict__["_mx8"].sealed = {"proj": held(D, D) + (None,), "out": held(D, D) + (None,)}
    for lin in (b.ff.net[0].proj, b.ff.net[2], b.attn1.to_q, b.attn1.to_k, b.attn1.to_v, b.attn1.to_out[0], b.attn2.to_q, b.attn2.to_out[0]):
        lin.weight.data = torch.empty(0, dtype=BF)
    assert lora.member_shapes(b.attn1, "qkv", ("to_q", "to_k", "to_v")) == [(D, D)] * 3
    assert lora.member_shapes(b.ff, "ff1", ("net.0.proj",)) == [(4 * D, D)]
    assert lora.member_shapes(b.attn2, "kv", ("to_k", "to_v")) == [(D, D)] * 2           # not freed: the parameters' shapes
    m.attach_lora(_adapter(m, 16), name="a", mx8=True)
    s = _slots(m)
    assert s[("attn1", "qkv")].down[0].shape == (3 * 128, D) and s[("ff", "ff2")].up[0].shape == (D, 128)
    assert isinstance(s[("attn2", "kv")], lora.LoraSlot)
    m.set_lora_weights({"a": 0.5})
    m.detach_lora()
    assert not _slots(m)
    # a shape that does not fit is refused with the held operand's shape
    bad = lora.LoraAdapter({"transformer_blocks.0.ff.net.2": (torch.zeros(4, D, dtype=BF), torch.zeros(D, 4, dtype=BF), None)})
    with pytest.raises(ValueError, match=r"ff\.net\.2.*but the linear is \(256, 1024\)"):
        m.attach_lora(bad, mx8=True)
    with pytest.raises(RuntimeError, match=r"unquantize_ff\(\) first"):
        m.attach_lora(_adapter(m, 16))


def test_pair_mx8_makes_the_down_gemm_and_hands_on_the_quantised_ups(monkeypatch):
    from ltxmi import lora, ops
    m = _model(heads=4, dh=64, layers=1)
    _mark(m, ("attn1.qkv",), True)
    b = m.transformer_blocks[0]
    calls = []
    monkeypatch.setattr(ops, "gemm_mx8", lambda *a, **k: (calls.append((a, k)), ("T", "Ts"))[1])
    xq = (object(), object())
    assert lora.pair_mx8(b.attn1, "qkv", xq) == {} and lora.pair_mx8(b.ff, "ff1", xq) == {} and not calls
    m.attach_lora(_adapter(m, 16), mx8=True)
    s = b.attn1.__dict__["_lora"]["qkv"]
    kw = lora.pair_mx8(b.attn1, "qkv", xq)
    assert kw == dict(a2=("T", "Ts"), w2=s.up, a2_group_cols=D)
    (a, k), = calls
    assert a[:2] == xq and a[2] is s.down[0] and a[3] is s.down[1] and k == dict(mx_out=True)
    assert lora.pair_mx8(b.ff, "ff2", xq)["a2_group_cols"] == 0
