"""``Transformer3DModel.quantize_attention`` without a device: the ``linears`` choice, what is refused before any launch, the
sequence-parallel processors' refusal hook, and that a model that was never quantised carries nothing of it
(tests/test_gpu_attn_mx8_model.py holds the rest on the MI355X)."""
import pytest
import torch

from test_mx8_model_cpu import _model


def test_the_linears_choice():
    from ltxmi import attn_mx8
    assert attn_mx8.LINEARS == ("attn1.qkv", "attn1.to_out", "attn2.to_q", "attn2.to_out")
    assert attn_mx8.resolve(None) == attn_mx8.DEFAULT_LINEARS and set(attn_mx8.DEFAULT_LINEARS) <= set(attn_mx8.LINEARS)
    # any iterable, in any order, comes back in the order of LINEARS; a linear left out of the default stays selectable
    assert attn_mx8.resolve(iter(["attn2.to_out", "attn1.qkv"])) == ("attn1.qkv", "attn2.to_out")
    for n in attn_mx8.LINEARS:
        assert attn_mx8.resolve([n]) == (n,)
    assert attn_mx8.resolve(()) == ()
    assert set(attn_mx8.PARTS) == set(attn_mx8.LORA_SLOTS) == set(attn_mx8.LINEARS)
    # attn2.to_k / to_v are no choice: they run once per generation and stay bf16
    for bad in ("attn2.to_k", "attn2.kv", "ff.net.2", "attn1.to_q"):
        with pytest.raises(ValueError, match="unknown linear '" + bad.replace(".", r"\.") + "'"):
            attn_mx8.resolve(["attn1.qkv", bad])


def test_a_fresh_model_is_not_quantised_and_host_weights_are_refused():
    m = _model()
    assert m.attention_quantized is False
    assert all("_mx8" not in a.__dict__ for b in m.transformer_blocks for a in (b.attn1, b.attn2))
    m.unquantize_attention()                            # nothing to undo: no error
    keys = set(m.state_dict())
    with pytest.raises(TypeError, match=r"quantize_attention.*transformer_blocks\.0\.attn1\.qkv\.weight.*CUDA bfloat16"):
        m.quantize_attention()
    with pytest.raises(TypeError, match=r"transformer_blocks\.0\.attn2\.to_out\.weight"):
        m.quantize_attention(linears=["attn2.to_out"])
    with pytest.raises(ValueError, match="unknown linear"):
        m.quantize_attention(linears=["attn3.to_q"])
    assert not m.attention_quantized and set(m.state_dict()) == keys          # refused before anything was marked
    assert all("_mx8" not in a.__dict__ for b in m.transformer_blocks for a in (b.attn1, b.attn2))
    m.quantize_attention(linears=())                    # the empty choice quantises nothing
    assert not m.attention_quantized


def test_widths_the_kernel_does_not_take_are_refused():
    m = _model(heads=1, dh=64, layers=1)                # D = 64: in_features is no multiple of 128
    with pytest.raises(ValueError, match=r"transformer_blocks\.0\.attn1\.qkv.*% 128"):
        m.quantize_attention()
    with pytest.raises(ValueError, match=r"transformer_blocks\.0\.attn2\.to_q.*% 128"):
        m.quantize_attention(linears=("attn2.to_q", "attn2.to_out"))
    assert not m.attention_quantized


def test_sequence_parallel_processors_carry_the_refusal_hook():
    from ltxmi import distributed
    from ltxmi.attention import AttnProcessor2_0
    for proc in (distributed.UlyssesAttnProcessor(), distributed.RingAttnProcessor()):
        with pytest.raises(NotImplementedError, match=type(proc).__name__ + r".*quantize_attention\(\).*unquantize_attention\(\) first"):
            proc.refuse_quantized_attention()
    assert not hasattr(AttnProcessor2_0(), "refuse_quantized_attention")
    # a model that runs them is refused by quantize_attention, before the weights are looked at
    m = _model()
    distributed.enable_sequence_parallel(m)
    with pytest.raises(NotImplementedError, match=r"quantize_attention\(\).*UlyssesAttnProcessor"):
        m.quantize_attention()
    distributed.disable_sequence_parallel(m)


def test_refusals_name_the_call():
    """The messages of the quantised and of the keep_bf16=False state, driven through the state object alone (no device)."""
    from ltxmi import attn_mx8, lora
    m = _model()
    chosen = ("attn1.qkv", "attn2.to_out")
    for b in m.transformer_blocks:
        b.attn1.__dict__["_mx8"] = attn_mx8.AttnState(True, False)
        b.attn2.__dict__["_mx8"] = attn_mx8.AttnState(False, True)
    m.__dict__["_mx8_attn_linears"] = chosen
    assert m.attention_quantized
    with pytest.raises(RuntimeError, match="quantised already"):
        m.quantize_attention()
    z = lambda n, k: (torch.zeros(4, k, dtype=torch.bfloat16), torch.zeros(n, 4, dtype=torch.bfloat16), None)
    named = lambda p: lora.LoraAdapter({"transformer_blocks.0." + p: z(128, 128)})
    for path in ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn2.to_out.0"):
        for call in (lambda: m.attach_lora(named(path)), lambda: m.fuse_lora(named(path))):
            with pytest.raises(RuntimeError, match=r"attn1\.qkv, attn2\.to_out.*unquantize_attention\(\) first"):
                call()
    for path in ("attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "ff.net.0.proj"):       # not chosen: not refused here
        m._refuse_attn_quantized(["transformer_blocks.1." + path], "attach_lora")
    m.state_dict()                                      # keep_bf16=True: allowed
    for b in m.transformer_blocks:
        b.attn1.__dict__["_mx8"].sealed = {"proj": (None, None, None)}
    for call, word in ((m.unquantize_attention, "unquantize_attention"), (m.state_dict, "state_dict"),
                       (lambda: m.load_state_dict({}), "load_state_dict")):
        with pytest.raises(RuntimeError, match=word + r"\(\).*keep_bf16=False"):
            call()
