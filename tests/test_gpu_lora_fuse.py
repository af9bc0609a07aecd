"""LoRA adapters fused into the weights on a real MI355X: ``lora.merged_weight`` on the GEMM kernels (the per-element bound of
tests/lora_fuse_cpu_cases.py against float64, the rounding witnesses, the in-place form), and ``Transformer3DModel.fuse_lora`` /
``set_fused_lora_weights`` / ``unfuse_lora`` on the cases of tests/test_gpu_lora.py: bit-identity with a model LOADED on the
merged weights -- with a forward before the fuse, so that packs and text K/V caches of the base weights exist and must not be
served -- and ``assert_parity`` against the truth and the eager yardstick the unmerged adapters are held to."""
import pytest
import torch

import lora_fuse_cpu_cases as fuse_cases
import mixed_oracle
import test_gpu_lora as unmerged
from test_gpu_model import BF, DEV, assert_parity, build_model, dit_case, rel, run_oracles

pytestmark = pytest.mark.gpu

_forward = unmerged._forward
_YARD = {}


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    unmerged._2B.clear()
    _YARD.clear()


def _fuse_both(c, m=None):
    for (ad, w), name in zip(c["adapters"], ("r16", "r64")):
        (m or c["m"]).fuse_lora(ad, weight=w, name=name)


def _weights(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _loaded_on_merged(cfg, base_w, adapters):
    """A second model whose state dict carries the ``merged_weight`` results."""
    return build_model(cfg, fuse_cases.merged_state_dict(base_w, adapters))


# ------------------------------------------------------------------------------------------------- the merge of one linear
@pytest.mark.parametrize("n_out,k_in,ranks,kernels", [
    (300, 260, (64,), (0,)),                         # ragged M and N tiles
    (2048, 128, (128,), (0,)),                       # patchify-like: a narrow N
    (8192, 2048, (16, 64, 100), (1, 2)),             # three adapters, 180 padded to 192; the 256-row kernels
])
def test_merged_weight_is_within_the_bound_of_one_rounding(n_out, k_in, ranks, kernels):
    from ltxmi import lora, ops
    base, entries = fuse_cases.drawn_operands(n_out, k_in, ranks, seed=n_out + k_in, device=DEV)
    R, k8 = (sum(ranks) + 63) // 64 * 64, (k_in + 7) // 8 * 8
    e = lambda *s: torch.empty(*s, dtype=BF)
    assert ops.gemm_kernel_id(e(n_out, R), e(k8, R), None, e(n_out, k8), ops.EPI_GATE_RESIDUAL, e(n_out, k8)) in kernels
    got = lora.merged_weight(base, entries)
    ratio, off = fuse_cases.bound_ratio(got, base, entries)
    print(f"merged_weight {(n_out, k_in, sum(ranks))}: largest |got - truth| / bound {ratio:.3f}, not correctly rounded {off:.1e}")
    assert ratio <= 1.0, ratio
    # the keep_base=False form: ``out`` is the residual
    alias = base.clone()
    assert lora.merged_weight(alias, entries, out=alias) is alias
    assert torch.equal(alias, got), "the in-place merge differs from the merge into a buffer of its own"


def test_rounding_witnesses():
    """One rounding, from an fp32 sum that includes the base -- where rounding the product first, or merging the two rank
    components one after the other, gives 1.0: by ``merged_weight``, and by two adapters fused separately on one linear."""
    from ltxmi import lora
    base, down, up = fuse_cases.witness_operands(device=DEV)
    got = lora.merged_weight(base, [(down, up, 1.0)])
    assert bool((got.float() == fuse_cases.WITNESS).all()), got.float().unique()
    cfg, sd32, x, enc, mask, ts, frac = dit_case(2, 64, 1, (1, 2, 2), 1, 8)
    m = build_model(cfg, sd32)
    w = m.transformer_blocks[0].attn1.to_q.weight
    with torch.no_grad():
        w.fill_(1.0)
    a, b = fuse_cases.witness_adapters("transformer_blocks.0.attn1.to_q")
    m.fuse_lora(a, name="a")
    assert bool((w == 1).all()), "1 + 2^-8 is a tie and rounds to even"
    m.fuse_lora(b, name="b")
    assert bool((w.float() == fuse_cases.WITNESS).all()), w.float().unique()
    m.unfuse_lora()
    assert bool((w == 1).all())


# ------------------------------------------------------------------------------------------------- the model, 2B widths
def _yardsticks():
    """(truth, eager) exactly as test_gpu_lora.py::test_2b_width_block_with_two_adapters builds them, and the mixed pair of
    ::test_2b_width_block_mixed_precision; computed once."""
    if not _YARD:
        c = unmerged._case_2b()
        x, enc, mask, ts, frac, grid = c["inputs"]
        merged32 = unmerged._merged32(c["sd32"], c["adapters"])
        _YARD["truth"] = run_oracles(c["cfg"], merged32, x, enc, mask, ts, frac, grid, truth_device=DEV, eager_device=DEV, **c["okw"])[0]
        _YARD["truth_mixed"] = mixed_oracle.run(merged32, c["cfg"], x, enc, mask, ts, frac, grid, torch.float32, DEV, **c["okw"])
        with pytest.MonkeyPatch.context() as mp:
            unmerged._unmerged_linear(c["adapters"], mp)
            _YARD["eager"] = run_oracles(c["cfg"], c["sd32"], x, enc, mask, ts, frac, grid, truth_device=DEV, eager_device=DEV,
                                         **c["okw"])[1]
            _YARD["eager_mixed"] = mixed_oracle.run(c["sd32"], c["cfg"], x, enc, mask, ts, frac, grid, BF, DEV, **c["okw"])
    return _YARD


def test_2b_fused_forward_is_the_forward_of_a_model_loaded_on_merged_weights():
    c = unmerged._case_2b()                              # (its base forwards have run: packs and text K/V caches exist)
    m, inputs = c["m"], c["inputs"]
    assert m.transformer_blocks[0].attn2.derived_slots() and m.transformer_blocks[0].attn1.derived_slots()
    base_w = _weights(m)
    params = {k: (p, p.data_ptr(), p._version) for k, p in m.named_parameters()}
    _fuse_both(c)
    try:
        for k, q in m.named_parameters():
            p, ptr, ver = params[k]
            assert q is p and q.data_ptr() == ptr, k
            if k.endswith(".weight") and k[:-7] in c["adapters"][0][0].modules:
                assert q._version > ver, f"{k}: the version counter did not move"
        assert m.fused_lora_names() == ["r16", "r64"] and m.lora_names() == []
        assert m.transformer_blocks[0].attn1.__dict__.get("_lora") is None
        assert set(m.__dict__["_lora_fused"].base) == set(c["adapters"][0][0].modules)
        assert m.state_dict().keys() == base_w.keys()
        out = _forward(m, *inputs, **c["mkw"])
        out_mixed = _forward(m, *inputs, mixed=True, **c["mkw"])
    finally:
        m.unfuse_lora()
    assert rel(out, c["base"]) > 5e-2 and rel(out_mixed, c["base_mixed"]) > 5e-2, "the fuse did nothing: stale packs or text K/V"
    m2 = _loaded_on_merged(c["cfg"], base_w, c["adapters"])
    assert torch.equal(_forward(m2, *inputs, **c["mkw"]), out)
    assert torch.equal(_forward(m2, *inputs, mixed=True, **c["mkw"]), out_mixed)
    # unfuse_lora() has restored the weights and the output bits
    assert all(torch.equal(v, base_w[k]) for k, v in m.state_dict().items())
    assert "_lora_fused" not in m.__dict__
    assert torch.equal(_forward(m, *inputs, **c["mkw"]), c["base"]), "unfuse_lora() does not restore the output"
    assert torch.equal(_forward(m, *inputs, mixed=True, **c["mkw"]), c["base_mixed"])


def test_2b_fused_parity():
    c = unmerged._case_2b()
    m, inputs, y = c["m"], c["inputs"], _yardsticks()
    _fuse_both(c)
    try:
        out = _forward(m, *inputs, **c["mkw"])
        out_mixed = _forward(m, *inputs, mixed=True, **c["mkw"])
    finally:
        m.unfuse_lora()
    assert_parity(out, y["truth"], y["eager"], "2B width, 1 block, N 624, adapters r16 + r64 fused")
    assert rel(out[2], out[1]) > 1e-3                                                # the STG row is perturbed
    assert_parity(out_mixed, y["truth_mixed"], y["eager_mixed"], "mixed 2B width, 1 block, N 624, adapters r16 + r64 fused")


def test_2b_set_fused_lora_weights_is_a_fresh_fuse():
    c = unmerged._case_2b()
    m, inputs = c["m"], c["inputs"]
    _fuse_both(c)
    try:
        fresh_w, fresh = _weights(m), _forward(m, *inputs, **c["mkw"])
        m.set_fused_lora_weights({"r16": 1.25, "r64": 0.5})
        other = _forward(m, *inputs, **c["mkw"])
        assert rel(other, fresh) > 1e-2, "set_fused_lora_weights: stale packs or text K/V"
        m.set_fused_lora_weights({"r16": 0.5, "r64": 2.0})
        assert all(torch.equal(v, fresh_w[k]) for k, v in m.state_dict().items())
        assert torch.equal(_forward(m, *inputs, **c["mkw"]), fresh)
        m.unfuse_lora("r16")
        only64 = _forward(m, *inputs, **c["mkw"])
        only64_w = _weights(m)
    finally:
        m.unfuse_lora()
    assert torch.equal(_forward(m, *inputs, **c["mkw"]), c["base"])
    # keep_base=False, on a model of its own (there is no way back): in place, the bits of the merge from a kept base
    ad, w = c["adapters"][1]
    m3 = build_model(c["cfg"], _weights(m))
    assert torch.equal(_forward(m3, *inputs, **c["mkw"]), c["base"])
    m3.fuse_lora(ad, weight=w, name="r64", keep_base=False)
    assert not m3.__dict__["_lora_fused"].base
    assert all(torch.equal(v, only64_w[k]) for k, v in m3.state_dict().items())
    assert torch.equal(_forward(m3, *inputs, **c["mkw"]), only64)
    with pytest.raises(RuntimeError, match="keep_base=False"):
        m3.unfuse_lora()


def test_2b_non_block_linears():
    """An adapter that also names caption_projection.linear_1 and proj_out: against the fp32 oracle on the merged weights,
    with the oracle's bf16 rendering on those weights as the yardstick."""
    from ltxmi import loading
    c = unmerged._case_2b()
    m, (x, enc, mask, ts, frac, grid) = c["m"], c["inputs"]
    sd = dict(fuse_cases.make_adapter_sd(c["cfg"], 16, seed=5),
              **fuse_cases.other_adapter_sd(m, ("caption_projection.linear_1", "proj_out"), 16, seed=8))
    ad = loading.load_lora(sd)
    with pytest.raises(ValueError, match="caption_projection.linear_1, proj_out"):
        m.attach_lora(ad)
    block_only = [(loading.load_lora(fuse_cases.make_adapter_sd(c["cfg"], 16, seed=5)), 1.0)]
    truth, eager = run_oracles(c["cfg"], unmerged._merged32(c["sd32"], [(ad, 1.0)]), x, enc, mask, ts, frac, grid, truth_device=DEV,
                               eager_device=DEV, **c["okw"])
    truth_block_only = run_oracles(c["cfg"], unmerged._merged32(c["sd32"], block_only), x, enc, mask, ts, frac, grid,
                                   truth_device=DEV, eager_device=DEV, **c["okw"])[0]
    assert rel(truth, truth_block_only) > 5e-2, "the two linears outside the block are too weak to test anything"
    m.fuse_lora(ad, name="all")
    try:
        out = _forward(m, x, enc, mask, ts, frac, grid, **c["mkw"])
    finally:
        m.unfuse_lora()
    assert_parity(out, truth, eager, "2B width, 1 block, adapter on the block, caption_projection.linear_1 and proj_out, fused")
    assert torch.equal(_forward(m, x, enc, mask, ts, frac, grid, **c["mkw"]), c["base"])


# ------------------------------------------------------------------------------------------------- the model, 13B widths
def test_13b_width_block_fused():
    """One block at the 13B widths (32 x 128, FF 16384), N = 1040, B 2, as test_gpu_lora.py sets it up: the 16384-wide merges."""
    grid, B, T = (5, 13, 16), 2, 128
    cfg, sd32, x, enc, mask, ts, frac = dit_case(32, 128, 1, grid, B, T, caption=4096, seed=26)
    adapters = unmerged._adapters(cfg, [(16, 5, None, 0.5), (128, 6, 64.0, 2.0)])
    m = build_model(cfg, sd32)
    base = _forward(m, x, enc, mask, ts, frac, grid)
    base_w = _weights(m)
    for ad, w in adapters:
        m.fuse_lora(ad, weight=w)
    assert m.fused_lora_names() == ["lora0", "lora1"]
    out = _forward(m, x, enc, mask, ts, frac, grid)
    assert out.shape == (2, 1040, 128) and rel(out, base) > 5e-2
    m2 = _loaded_on_merged(cfg, base_w, adapters)
    assert torch.equal(_forward(m2, x, enc, mask, ts, frac, grid), out)
    del m2
    m.unfuse_lora()
    assert all(torch.equal(v, base_w[k]) for k, v in m.state_dict().items())
    assert torch.equal(_forward(m, x, enc, mask, ts, frac, grid), base)
