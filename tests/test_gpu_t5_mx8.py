"""``T5EncoderModel.quantize`` on a real MI355X (the configs ``tiny`` and ``xxl_one_block`` of tests/test_gpu_t5.py).

  (a) composition   the quantised encoder's output is bit-identical to the same forward written HERE from the ops that existed
                    before and have tests of their own: rmsnorm_weight -> quantize_mx8 -> gemm_mx8 -> attention_relbias ->
                    quantize_mx8 -> gemm_mx8 + residual -> rmsnorm_weight -> quantize_mx8 -> gemm_mx8 -> gated_gelu ->
                    quantize_mx8 -> gemm_mx8 + residual.  So the fused row passes, the skinny GEMM and the model's plumbing add
                    nothing of their own.  For the full set and every single linear; the gemm_mx8_skinny launches are counted, and
                    above the skinny entry's row limit the same linears run on gemm_mx8 with the same bits;
  (b) float64       truth: the patched restatement tests/t5_mx8_double.py in float64 (the format is part of the function).
                    Yardstick: the same patched restatement run by torch in bf16 on the CPU.  Max-abs and rms of the GPU output
                    at most 2 x the yardstick's, the factor of tests/test_gpu_t5.py.  Weights init_state_dict(stream=30,
                    qk_gain=0.5): at that file's gain of 2 the attention is near one-hot and the format alone moves an output of
                    rms 1 by rms 0.25, so nothing could be told.  On ``tiny`` and on a 4-block, d_model-512 config: the float64
                    restatement of a block at XXL width takes the CPU longer than a test may, and (a) covers that width;
  (c) cost          printed, not a gate: the quantised output against the UNPATCHED float64 truth, beside the bf16 model's error
                    and the format's own cost (patched against unpatched truth);
  (d) life cycle    unquantize() restores the bf16 bits; keep_bf16=False gives the same bits from freed weights and the three
                    calls raise; an in-place weight edit quantises again; two quantised forwards are equal; .to() is followed;
                    LTXVideoPipeline.encode_prompt runs through a quantised encoder."""
import pytest
import torch

import t5_double as td
import t5_mx8_double as tq
from fake_t5 import FakeTokenizer
from test_gpu_t5 import MODEL_CASES, _inputs, _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
MID = dict(td.TINY, d_model=512, d_ff=1024, num_heads=8, num_layers=4)          # the 4-block config of (b) and (c)
SUBSETS = [tq.LINEARS] + [(n,) for n in tq.LINEARS]


def _weights(cfg, seed=0):
    return {k: v.to(BF) for k, v in td.init_state_dict(cfg, seed=seed, stream=30.0, qk_gain=0.5).items()}


def _composed(model, ids, mask, chosen):
    """The quantised forward from ops.rmsnorm_weight / quantize_mx8 / gemm_mx8 / gemm / attention_relbias / gated_gelu alone."""
    from ltxmi import ops
    cfg = model.config
    B, L = ids.shape
    eps, R = cfg.layer_norm_epsilon, ops.EPI_GATE_RESIDUAL

    def linear(name, x, w, **kw):
        if name in chosen:
            return ops.gemm_mx8(*ops.quantize_mx8(x), *ops.quantize_mx8(w), **kw)
        return ops.gemm(x, w, **kw)

    key_bias = torch.zeros((B, L), dtype=torch.float32, device=DEV).masked_fill_(mask == 0, float("-inf"))
    x = ops.embedding(ids, model.shared.weight).view(B * L, cfg.d_model)
    rel, center = model.rel_bias(L)
    for block in model.encoder.block:
        att, ff = block.layer[0].SelfAttention, block.layer[1].DenseReluDense
        h = ops.rmsnorm_weight(x, block.layer[0].layer_norm.weight, eps)
        qkv = linear("qkv", h, torch.cat([att.q.weight, att.k.weight, att.v.weight]).contiguous()).view(B, L, 3, att.n_heads, att.d_kv)
        ctx = ops.attention_relbias(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], rel_bias=rel, rel_center=center, key_bias=key_bias,
                                    softmax_scale=1.0).view(B * L, att.inner_dim)
        linear("o", ctx, att.o.weight, out=x, epilogue=R, residual=x)
        h = ops.rmsnorm_weight(x, block.layer[1].layer_norm.weight, eps)
        g = ops.gated_gelu(linear("wi", h, torch.cat([ff.wi_0.weight, ff.wi_1.weight]).contiguous()))
        linear("wo", g, ff.wo.weight, out=x, epilogue=R, residual=x)
    return ops.rmsnorm_weight(x, model.encoder.final_layer_norm.weight, eps).view(B, L, cfg.d_model)


class _Count:
    """Counts the calls of an ops function while it stands in for it."""

    def __init__(self, monkeypatch, name):
        from ltxmi import ops
        self.calls, fn = 0, getattr(ops, name)

        def wrapper(*a, **k):
            self.calls += 1
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapper)


# ------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: c[0])
def test_quantised_encoder_is_the_composition_of_the_tested_ops(case, monkeypatch):
    name, cfg, _, L, valid = case
    model = _model(cfg, _weights(cfg))
    ids, mask = (t.to(DEV) for t in _inputs(cfg, L, valid))
    skinny, big = _Count(monkeypatch, "gemm_mx8_skinny"), _Count(monkeypatch, "gemm_mx8")
    with torch.no_grad():
        for chosen in SUBSETS:
            model.quantize(linears=chosen)
            skinny.calls = big.calls = 0
            got = model(ids, attention_mask=mask)[0]
            assert (skinny.calls, big.calls) == (len(chosen) * cfg["num_layers"], 0), chosen     # per block: one per chosen linear
            model.unquantize()
            want = _composed(model, ids, mask, chosen)
            assert got.dtype == BF and torch.isfinite(got.float()).all()
            assert torch.equal(got, want), (name, chosen, int((got != want).sum()))


def test_above_the_row_limit_the_same_linears_run_on_gemm_mx8(monkeypatch):
    from ltxmi import ops
    cfg = td.TINY
    model = _model(cfg, _weights(cfg))
    L = ops.MXT_MAX_ROWS // 2 + 4                                  # 2 x 260 = 520 rows
    ids, mask = (t.to(DEV) for t in _inputs(cfg, L, (L, L - 37)))
    skinny, big = _Count(monkeypatch, "gemm_mx8_skinny"), _Count(monkeypatch, "gemm_mx8")
    with torch.no_grad():
        model.quantize(linears=tq.LINEARS)
        got = model(ids, attention_mask=mask)[0]
        assert (skinny.calls, big.calls) == (0, 4 * cfg["num_layers"])
        model.unquantize()
        assert torch.equal(got, _composed(model, ids, mask, tq.LINEARS))


# ------------------------------------------------------------------------------------------------- (b), (c)
@pytest.mark.parametrize("case", [("tiny", td.TINY, 24, (24, 1)), ("four_blocks_d512", MID, 48, (48, 19))], ids=lambda c: c[0])
def test_quantised_encoder_against_float64_with_the_cpu_bf16_run_as_yardstick(case):
    name, cfg, L, valid = case
    sd_bf = _weights(cfg)
    sd64 = {k: v.double() for k, v in sd_bf.items()}
    ids, mask = _inputs(cfg, L, valid)
    truth = tq.encoder_forward(sd64, cfg, ids, mask)
    cpu_max, cpu_rms = td.errors(tq.encoder_forward(sd_bf, cfg, ids, mask), truth)
    model = _model(cfg, sd_bf)
    plain_gpu = model(ids.to(DEV), attention_mask=mask.to(DEV))[0]
    model.quantize(linears=tq.LINEARS)
    got = model(ids.to(DEV), attention_mask=mask.to(DEV))[0]
    assert torch.isfinite(got.float()).all()
    gpu_max, gpu_rms = td.errors(got, truth)
    print(f"t5 mx8 {name}: |truth| max {float(truth.abs().max()):.3g}; max abs GPU {gpu_max:.4g} / CPU bf16 {cpu_max:.4g}; "
          f"rms GPU {gpu_rms:.4g} / CPU bf16 {cpu_rms:.4g}")
    # (c) the precision cost, not a gate: against the function without the format
    unpatched = td.encoder_forward(sd64, cfg, ids, mask)
    q, b, f = td.errors(got, unpatched), td.errors(plain_gpu, unpatched), td.errors(truth, unpatched)
    print(f"t5 mx8 {name}: against the unpatched float64 truth (|truth| rms {float(unpatched.pow(2).mean().sqrt()):.3g}): quantised model "
          f"max {q[0]:.4g} rms {q[1]:.4g}; bf16 model max {b[0]:.4g} rms {b[1]:.4g}; the format alone max {f[0]:.4g} rms {f[1]:.4g}")
    assert gpu_max <= 2.0 * cpu_max and gpu_rms <= 2.0 * cpu_rms


# ------------------------------------------------------------------------------------------------- (d)
def test_life_cycle():
    from ltxmi import loading
    cfg = td.TINY
    sd_bf = _weights(cfg)
    ids, mask = (t.to(DEV) for t in _inputs(cfg, 24, (24, 9)))
    model = _model(cfg, sd_bf)
    plain = model(ids, attention_mask=mask)[0]
    model.quantize()
    q1 = model(ids, attention_mask=mask)[0]
    assert not torch.equal(q1, plain)
    assert torch.equal(model(ids, attention_mask=mask)[0], q1), "two quantised forwards differ"
    # an in-place edit of a weight quantises again (and the edit is seen: the output moves), the edit undone gives q1 back
    w = model.encoder.block[1].layer[1].DenseReluDense.wo.weight
    keep = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    assert not torch.equal(model(ids, attention_mask=mask)[0], q1)
    with torch.no_grad():
        w.copy_(keep)
    assert torch.equal(model(ids, attention_mask=mask)[0], q1)
    # .to() is followed: the cache is keyed on the parameters' storage
    model.to("cpu").to(DEV)
    assert model.quantized and torch.equal(model(ids, attention_mask=mask)[0], q1)
    model.unquantize()
    assert torch.equal(model(ids, attention_mask=mask)[0], plain), "unquantize() does not restore the bf16 output"
    # keep_bf16=False: the same bits from freed weights, through the loader's switch as well
    model.quantize(keep_bf16=False)
    for block in model.encoder.block:
        att, ff = block.layer[0].SelfAttention, block.layer[1].DenseReluDense
        assert all(lin.weight.numel() == 0 for lin in (att.q, att.k, att.v, att.o, ff.wi_0, ff.wi_1, ff.wo))
        assert not att.derived_slots() and not ff.derived_slots()          # the stacked bf16 operands went with them
    assert model.shared.weight.numel() and model.encoder.final_layer_norm.weight.numel()
    assert torch.equal(model(ids, attention_mask=mask)[0], q1)
    model.to("cpu").to(DEV)                                                # the held weights follow the device
    assert torch.equal(model(ids, attention_mask=mask)[0], q1)
    for call in (model.unquantize, model.state_dict, lambda: model.load_state_dict(sd_bf)):
        with pytest.raises(RuntimeError, match=r"keep_bf16=False\) freed"):
            call()
    loaded = loading.load_t5_encoder(sd_bf, dict(cfg), device=DEV, mx8=True)
    assert loaded.quantized and torch.equal(loaded(ids, attention_mask=mask)[0], q1)


def test_pipeline_encodes_prompts_through_a_quantised_encoder():
    import ltxmi
    cfg = dict(td.TINY, vocab_size=256)
    enc = _model(cfg, _weights(cfg, seed=4))
    tok = FakeTokenizer()
    t = tok(["a red fox jumps over the fence"], padding="max_length", max_length=32, truncation=True, add_special_tokens=True,
            return_tensors="pt")
    plain = enc(t.input_ids.to(DEV), attention_mask=t.attention_mask.to(DEV))[0]
    enc.quantize()
    pipe = ltxmi.LTXVideoPipeline(tokenizer=tok, text_encoder=enc)
    pe, pm, ne, nm = pipe.encode_prompt("a red fox jumps over the fence", True, negative_prompt="blurry, low quality", device=DEV,
                                        text_encoder_max_tokens=32)
    want = enc(t.input_ids.to(DEV), attention_mask=t.attention_mask.to(DEV))[0]
    assert pe.dtype == BF and tuple(pe.shape) == (1, 32, 128) and torch.equal(pe, want) and not torch.equal(pe, plain)
    assert torch.equal(pm.cpu(), t.attention_mask) and tuple(ne.shape) == (1, 32, 128) and torch.isfinite(ne.float()).all()
