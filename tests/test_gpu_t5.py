"""ltxmi.T5EncoderModel on the GPU against the float64 restatement of tests/t5_double.py.

No tolerance is invented: the same restatement run by torch on the CPU in bfloat16 rounds where Hugging Face's eager bf16
forward rounds, on the same bf16 weights and inputs, and its error against float64 is the yardstick.  The GPU model is a bf16
pipeline with the same rounding points or fewer (fp32 scores, residual adds on the GEMM accumulator), so its max-abs and rms
error may be at most twice the yardstick's; a wrong bias sign, mask or residual lands orders of magnitude above, which the
flipped-bias run shows.  Measured pairs (GPU / CPU-bf16, max abs and rms): profiles/t5_encoder.md."""
import pytest
import torch

import t5_double as td
from fake_t5 import FakeTokenizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16

# name, config, weights (stream scale, logit gain), tokens, valid tokens per batch row
MODEL_CASES = [
    ("tiny", td.TINY, (30.0, 2.0), 24, (24, 1)),
    ("xxl_one_block", td.XXL_ONE, (30.0, 2.0), 256, (200, 77)),
]


def _inputs(cfg, L, valid, seed=2):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, cfg["vocab_size"], (len(valid), L), generator=g)
    mask = torch.zeros(len(valid), L, dtype=torch.long)
    for b, n in enumerate(valid):
        mask[b, :n] = 1
        ids[b, n:] = 0
    return ids, mask


def _model(cfg, sd_bf):
    from ltxmi import loading
    m = loading.load_t5_encoder(sd_bf, dict(cfg), device=DEV)
    assert m.unexpected_keys == []
    return m


@pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: c[0])
def test_encoder_against_float64_with_the_cpu_bf16_run_as_yardstick(case):
    name, cfg, (stream, gain), L, valid = case
    sd_bf = {k: v.to(BF) for k, v in td.init_state_dict(cfg, seed=0, stream=stream, qk_gain=gain).items()}
    ids, mask = _inputs(cfg, L, valid)
    truth = td.encoder_forward({k: v.double() for k, v in sd_bf.items()}, cfg, ids, mask)
    cpu_max, cpu_rms = td.errors(td.encoder_forward(sd_bf, cfg, ids, mask), truth)
    model = _model(cfg, sd_bf)
    out = model(ids.to(DEV), attention_mask=mask.to(DEV))
    got = out[0]
    assert got is out.last_hidden_state and got.dtype == BF and tuple(got.shape) == (len(valid), L, cfg["d_model"])
    assert torch.isfinite(got.float()).all()
    gpu_max, gpu_rms = td.errors(got, truth)
    print(f"t5 {name}: |truth| max {float(truth.abs().max()):.3g}; max abs GPU {gpu_max:.4g} / CPU bf16 {cpu_max:.4g}; "
          f"rms GPU {gpu_rms:.4g} / CPU bf16 {cpu_rms:.4g}")
    assert gpu_max <= 2.0 * cpu_max and gpu_rms <= 2.0 * cpu_rms
    # the same call again is the same bits (packed weights and the bias operand come from their caches)
    assert torch.equal(model(ids.to(DEV), attention_mask=mask.to(DEV))[0], got)
    # the bias with the sign of (key - query) flipped: operand[h, centre + d] <-> operand[h, centre - d]
    rel, center = model.rel_bias(L)
    table = model.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
    model.derived("rel_bias").put((table,), (L,), (rel.flip(-1).contiguous(), center))
    bad = model(ids.to(DEV), attention_mask=mask.to(DEV))[0]
    model.invalidate_packed()
    bad_max, bad_rms = td.errors(bad, truth)
    print(f"t5 {name}: flipped bias max abs {bad_max:.4g}, rms {bad_rms:.4g}")
    assert bad_max > 2.0 * cpu_max and bad_rms > 2.0 * cpu_rms
    # ... and the flipped run is the restatement with the wrong sign, to the same yardstick
    wrong = td.encoder_forward({k: v.double() for k, v in sd_bf.items()}, cfg, ids, mask, negate_offset=True)
    wrong_cpu = td.errors(td.encoder_forward(sd_bf, cfg, ids, mask, negate_offset=True), wrong)
    wrong_gpu = td.errors(bad, wrong)
    assert wrong_gpu[0] <= 2.0 * wrong_cpu[0] and wrong_gpu[1] <= 2.0 * wrong_cpu[1], (wrong_gpu, wrong_cpu)


def test_pipeline_encodes_prompts_through_the_encoder():
    import ltxmi
    cfg = dict(td.TINY, vocab_size=256)
    sd_bf = {k: v.to(BF) for k, v in td.init_state_dict(cfg, seed=4, stream=10.0).items()}
    enc = _model(cfg, sd_bf)
    assert enc.dtype == BF and enc.device.type == "cuda" and next(enc.parameters()).is_cuda
    tok = FakeTokenizer()
    pipe = ltxmi.LTXVideoPipeline(tokenizer=tok, text_encoder=enc)
    pe, pm, ne, nm = pipe.encode_prompt("a red fox jumps over the fence", True, negative_prompt="blurry, low quality", device=DEV,
                                        text_encoder_max_tokens=32)
    for text, e, m in (("a red fox jumps over the fence", pe, pm), ("blurry, low quality", ne, nm)):
        t = tok([text], padding="max_length", max_length=32, truncation=True, add_special_tokens=True, return_tensors="pt")
        want = enc(t.input_ids.to(DEV), attention_mask=t.attention_mask.to(DEV))[0]
        assert e.dtype == BF and tuple(e.shape) == (1, 32, 128) and e.is_cuda
        assert torch.equal(e, want) and torch.equal(m.cpu(), t.attention_mask)
        assert 0 < int(t.attention_mask.sum()) < 32
    # no mask: every token takes part (what HF does with attention_mask=None)
    ids = torch.randint(1, 256, (2, 17))
    full = enc(ids.to(DEV))[0]
    assert torch.equal(full, enc(ids.to(DEV), attention_mask=torch.ones(2, 17, dtype=torch.long, device=DEV))[0])
