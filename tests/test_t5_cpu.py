"""The T5 encoder's host side, without a GPU: the float64 restatement pinned to Hugging Face and to a golden, the bucket map,
the rel_bias operand, state-dict loading, the refusals, the hand-over from encode_prompt, and the attention bound of
tests/t5_cases.py pinned on the CPU (the emulated kernel inside, the wrong-sign oracle outside)."""
import json
import os

import pytest
import torch

import t5_cases as tc
import t5_double as td
from fake_t5 import FakeTokenizer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _double(sd):
    return {k: v.double() for k, v in sd.items()}


@pytest.fixture(scope="module")
def tiny_truth():
    sd = td.init_state_dict(td.TINY, seed=0)
    ids, mask = td.tiny_inputs()
    return sd, ids, mask, td.encoder_forward(_double(sd), td.TINY, ids, mask)


# fp32 against float64 over two blocks of K <= 256 sums: a few 1e-7 relative per operation, some tens of operations deep
FP32_REL = 1e-4


def test_restatement_equals_hf_fp32(tiny_truth):
    transformers = pytest.importorskip("transformers")
    sd, ids, mask, truth = tiny_truth
    cfg = transformers.T5Config(**td.TINY, dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
    model = transformers.T5EncoderModel(cfg).eval()
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"encoder.embed_tokens.weight"}
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask)[0]
    assert tuple(out.shape) == (2, 24, 128)
    err, _ = td.errors(out, truth)
    assert err <= FP32_REL * float(truth.abs().max()), (err, float(truth.abs().max()))


def test_restatement_equals_golden(tiny_truth):
    from safetensors.torch import load_file
    sd, ids, mask, truth = tiny_truth
    g = load_file(os.path.join(GOLDEN, "t5_tiny.safetensors"))
    assert torch.equal(g["input_ids"], ids) and torch.equal(g["attention_mask"], mask)
    assert int(mask[1].sum()) == 1                      # the second row is padded to a single valid token
    err, _ = td.errors(g["last_hidden_state"], truth)
    assert err <= FP32_REL * float(truth.abs().max()), err
    # ... and the restatement is sensitive to what the GPU tests rely on it for: the sign of the offset
    wrong = td.encoder_forward(_double(sd), td.TINY, ids, mask, negate_offset=True)
    assert td.errors(wrong[0], truth[0])[0] > 100 * FP32_REL * float(truth.abs().max())


def test_bucket_map_every_offset():
    from ltxmi import t5
    with open(os.path.join(GOLDEN, "t5_buckets.json")) as f:
        g = json.load(f)
    d = torch.arange(g["lo"], g["hi"] + 1)
    assert (g["lo"], g["hi"], len(g["buckets"])) == (-511, 511, 1023)
    ours = t5.relative_position_bucket(d, g["num_buckets"], g["max_distance"]).tolist()
    assert ours == g["buckets"]
    assert [td.bucket(int(x), g["num_buckets"], g["max_distance"]) for x in d] == g["buckets"]
    # the shape of the map: exact below num_buckets / 4, positive offsets in the upper half, saturating at max_distance
    assert ours[511 - 7:511 + 8] == [7, 6, 5, 4, 3, 2, 1, 0, 17, 18, 19, 20, 21, 22, 23]
    assert ours[0] == 15 and ours[-1] == 31 and ours[511 + 128] == 31 and ours[511 - 128] == 15


def test_bucket_map_equals_hf_function():
    pytest.importorskip("transformers")
    from transformers.models.t5.modeling_t5 import T5Attention
    from ltxmi import t5
    d = torch.arange(-511, 512)
    for nb, md in ((32, 128), (16, 64), (32, 256)):
        assert T5Attention._relative_position_bucket(d, True, nb, md).tolist() == t5.relative_position_bucket(d, nb, md).tolist()


def test_rel_bias_operand():
    from ltxmi import t5
    g = torch.Generator().manual_seed(5)
    for Lq, Lk, H in ((24, 24, 2), (1, 1, 1), (100, 200, 3), (512, 512, 2)):
        w = torch.randn(32, H, generator=g).to(torch.bfloat16)
        rel, center = t5.build_rel_bias(w, Lq, Lk, 32, 128)
        assert rel.dtype == torch.float32 and tuple(rel.shape) == (H, Lq + Lk - 1) and center == Lq - 1 and rel.is_contiguous()
        want = td.position_bias(w.float(), Lq, Lk, 32, 128)                   # [H, Lq, Lk] = table[bucket(j - i), h]
        i, j = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :]
        assert torch.equal(rel[:, center + (j - i)], want)


def _tiny_model():
    import ltxmi
    return ltxmi.T5EncoderModel(dict(td.TINY))


def test_state_dict_names_strict_alias_and_extras():
    from ltxmi import loading
    model = _tiny_model()
    assert sorted(model.state_dict()) == sorted(td.state_dict_names(td.TINY))
    sd = td.init_state_dict(td.TINY, seed=0)
    model.load_state_dict(sd, strict=True)
    assert torch.equal(model.shared.weight, sd["shared.weight"])
    # HF saves the tied embedding under both names, some exports only under the encoder's
    both = dict(sd, **{"encoder.embed_tokens.weight": sd["shared.weight"]})
    _tiny_model().load_state_dict(both, strict=True)
    only_alias = {k: v for k, v in both.items() if k != "shared.weight"}
    m2 = _tiny_model()
    m2.load_state_dict(only_alias, strict=True)
    assert torch.equal(m2.shared.weight, sd["shared.weight"])
    with pytest.raises(RuntimeError, match="decoder.block.0"):
        _tiny_model().load_state_dict(dict(sd, **{"decoder.block.0.layer.0.SelfAttention.q.weight": torch.zeros(2, 2)}), strict=True)
    # the loader: casts to bf16, strips a prefix, reports what names nothing in the encoder, insists on every encoder tensor
    extra = dict({"text_encoder." + k: v for k, v in only_alias.items()},
                 **{"decoder.block.0.layer.0.SelfAttention.q.weight": torch.zeros(2, 2), "lm_head.weight": torch.zeros(2, 2)})
    m3 = loading.load_t5_encoder(extra, dict(td.TINY), device="cpu")
    assert m3.unexpected_keys == ["decoder.block.0.layer.0.SelfAttention.q.weight", "lm_head.weight"]
    assert m3.dtype == torch.bfloat16 and not m3.training
    assert torch.equal(m3.encoder.block[1].layer[1].DenseReluDense.wo.weight,
                       sd["encoder.block.1.layer.1.DenseReluDense.wo.weight"].to(torch.bfloat16))
    # the stacked GEMM operands are built by the loader and the members are views of them: no second copy
    att, ff = m3.encoder.block[1].layer[0].SelfAttention, m3.encoder.block[1].layer[1].DenseReluDense
    qkv, wi = att._pack("qkv", [att.q, att.k, att.v]), ff._pack("wi", [ff.wi_0, ff.wi_1])
    assert qkv.data_ptr() == att.q.weight.data_ptr() and att.v.weight.data_ptr() == qkv[256:].data_ptr()
    assert wi.data_ptr() == ff.wi_0.weight.data_ptr() and ff.wi_1.weight.data_ptr() == wi[256:].data_ptr()
    assert torch.equal(qkv, torch.cat([sd[f"encoder.block.1.layer.0.SelfAttention.{c}.weight"] for c in "qkv"]).to(torch.bfloat16))
    assert sorted(m3.state_dict()) == sorted(td.state_dict_names(td.TINY))
    with pytest.raises(KeyError, match="final_layer_norm"):
        loading.load_t5_encoder({k: v for k, v in sd.items() if "final_layer_norm" not in k}, dict(td.TINY), device="cpu")


def test_loader_reads_a_config_file_and_a_safetensors_file(tmp_path):
    from safetensors.torch import save_file
    from ltxmi import loading
    sd = {k: v.to(torch.bfloat16).contiguous() for k, v in td.init_state_dict(td.TINY, seed=3).items()}
    save_file(sd, str(tmp_path / "t5.safetensors"))
    cfg = dict(td.TINY, architectures=["T5EncoderModel"], dense_act_fn="gelu_new", num_decoder_layers=2)   # a T5_config.json has more
    (tmp_path / "T5_config.json").write_text(json.dumps(cfg))
    m = loading.load_t5_encoder(tmp_path / "t5.safetensors", str(tmp_path / "T5_config.json"), device="cpu")
    assert m.unexpected_keys == [] and m.config.to_dict() == dict(td.TINY, is_decoder=False)
    assert torch.equal(m.shared.weight, sd["shared.weight"])
    with pytest.raises(ValueError, match="safetensors"):
        loading.load_t5_encoder(tmp_path / "t5.bin", cfg)


def test_refusals():
    import ltxmi
    for over, word in ((dict(feed_forward_proj="relu"), "feed_forward_proj"), (dict(feed_forward_proj="gated-silu"), "feed_forward_proj"),
                       (dict(d_kv=128), "d_kv"), (dict(is_decoder=True), "is_decoder")):
        with pytest.raises(NotImplementedError, match=f"{word}.*is not on this path"):
            ltxmi.T5EncoderModel(dict(td.TINY, **over))
    with pytest.raises(ValueError, match="missing"):
        ltxmi.T5EncoderModel(dict(d_model=128))
    m = _tiny_model().to(torch.bfloat16)
    ids = torch.zeros(1, 8, dtype=torch.long)
    for kw in (dict(output_attentions=True), dict(head_mask=torch.ones(2, 2)), dict(inputs_embeds=torch.zeros(1, 8, 128)),
               dict(decoder_input_ids=ids), dict(past_key_values=()), dict(use_cache=True), dict(encoder_hidden_states=ids),
               dict(output_hidden_states=True)):
        with pytest.raises(NotImplementedError, match=f"{next(iter(kw))} is not on this path"):
            m(ids, **kw)
    with pytest.raises(NotImplementedError, match="inputs_embeds is not on this path"):
        m(None, inputs_embeds=None)
    with pytest.raises(NotImplementedError, match="513 tokens is not on this path"):
        m(torch.zeros(1, 513, dtype=torch.long))
    # what HF callers pass as "off" is accepted up to the first launch, which refuses CPU tensors (no fallback path)
    with pytest.raises(TypeError, match="CUDA"):
        m(ids, attention_mask=torch.ones(1, 8), output_attentions=False, head_mask=None, return_dict=True)
    with pytest.raises(TypeError, match="bfloat16"):
        _tiny_model()(ids)


def test_encode_prompt_hands_over_to_the_encoder():
    """With a stub forward (no device here): encode_prompt returns what a direct call on the tokenizer's output returns,
    and finds dtype / device / parameters() on the model as it does on HF's."""
    import ltxmi

    class Stub(ltxmi.T5EncoderModel):
        calls = []

        def forward(self, input_ids=None, attention_mask=None, **kw):
            Stub.calls.append((input_ids.clone(), attention_mask.clone()))
            x = self.shared.weight[input_ids] * attention_mask[..., None].to(self.dtype)
            return ltxmi.t5.T5EncoderOutput(x)

    enc = Stub(dict(td.TINY, vocab_size=256)).to(torch.bfloat16)
    assert enc.dtype == torch.bfloat16 and enc.device.type == "cpu" and next(enc.parameters()).dtype == torch.bfloat16
    tok = FakeTokenizer()
    pipe = ltxmi.LTXVideoPipeline(tokenizer=tok, text_encoder=enc)
    pe, pm, ne, nm = pipe.encode_prompt("a red fox", True, negative_prompt="blurry", device="cpu", text_encoder_max_tokens=16)
    for text, e, m in (("a red fox", pe, pm), ("blurry", ne, nm)):
        t = tok([text], padding="max_length", max_length=16, truncation=True, add_special_tokens=True, return_tensors="pt")
        want = enc(t.input_ids, attention_mask=t.attention_mask)[0]
        assert e.dtype == torch.bfloat16 and tuple(e.shape) == (1, 16, 128)
        assert torch.equal(e, want) and torch.equal(m, t.attention_mask)
    assert len(Stub.calls) == 4


# ------------------------------------------------------------------------------------------ the attention bound, on the CPU
@pytest.fixture(scope="module")
def attn_truths():
    out = {}
    for case in tc.CASES:
        inp = tc.make_inputs(case)
        q, k, v = tc.views(inp["packed"], case[3], case[4])
        out[case[0]] = (inp, q, k, v, tc.truth(q, k, v, inp["rel"], inp["center"], inp["key_bias"]))
    return out


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_attention_bound_holds_the_emulated_kernel_and_rejects_the_wrong_sign(case, attn_truths):
    inp, q, k, v, (o, a) = attn_truths[case[0]]
    name, B, H, Lq, Lk, value, valid = case
    assert q.stride(1) == 3 * H * 64 and q.data_ptr() != k.data_ptr()          # slices of one packed buffer
    assert float((torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double())).abs().max()) > 200 or Lq == 1
    emu = tc.emulate(q, k, v, inp["rel"], inp["center"], inp["key_bias"])
    assert torch.isfinite(emu.float()).all()
    assert tc.worst_excess(emu, o, a) <= 1.0
    if value is not None:
        # a removed key carries no weight whatever its V holds; -10000 on top of logits of a few hundred is the same thing
        keep_truth = tc.truth(q, k, v, inp["rel"], inp["center"], torch.where(inp["keep"], 0.0, -float("inf")))[0]
        assert float((keep_truth - o).abs().max()) <= 1e-12
    if Lq > 1:
        wrong = tc.truth(q, k, v, inp["rel"], inp["center"], inp["key_bias"], negate_offset=True)[0]
        assert tc.worst_excess(wrong, o, a) > 10.0
        shifted = tc.truth(q, k, v, inp["rel"], inp["center"] + 1, inp["key_bias"])[0]
        assert tc.worst_excess(shifted, o, a) > 10.0
        if H > 1:
            mixed = tc.truth(q, k, v, inp["rel"].roll(1, 0), inp["center"], inp["key_bias"])[0]
            assert tc.worst_excess(mixed, o, a) > 10.0
