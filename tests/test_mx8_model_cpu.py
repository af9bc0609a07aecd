"""``Transformer3DModel.quantize_ff`` without a device: what it refuses before any launch, and that a model that was never
quantised carries nothing of it (tests/test_gpu_mx8_model.py holds the rest on the MI355X)."""
import pytest
import torch


def _model(heads=2, dh=64, layers=2):
    import ltxmi
    from oracle import dit
    cfg = dict(dit.default_2b_config(), num_attention_heads=heads, attention_head_dim=dh, num_layers=layers,
               cross_attention_dim=heads * dh, caption_channels=128)
    return ltxmi.Transformer3DModel(**cfg).to(torch.bfloat16).eval()


def test_a_fresh_model_is_not_quantised_and_host_weights_are_refused():
    m = _model()
    assert m.ff_quantized is False
    assert all("_mx8" not in b.ff.__dict__ for b in m.transformer_blocks)
    m.unquantize_ff()                                   # nothing to undo: no error
    keys = set(m.state_dict())
    with pytest.raises(TypeError, match=r"quantize_ff.*CUDA bfloat16"):
        m.quantize_ff()
    assert not m.ff_quantized and set(m.state_dict()) == keys          # refused before anything was marked


def test_widths_the_kernel_does_not_take_are_refused():
    m = _model(heads=1, dh=64, layers=1)                # D = 64: in_features of FF1 is no multiple of 128
    with pytest.raises(ValueError, match=r"ff\.net\.0\.proj.*% 128"):
        m.quantize_ff()
    assert not m.ff_quantized


def test_refusals_name_the_call():
    """The messages of the keep_bf16=False state, driven through the state object alone (no device needed)."""
    from ltxmi import ff_mx8
    m = _model()
    for b in m.transformer_blocks:
        st = b.ff.__dict__["_mx8"] = ff_mx8.FFState()
        st.sealed = ((None, None), (None, None))
    assert m.ff_quantized
    for call, word in ((m.unquantize_ff, "unquantize_ff"), (m.state_dict, "state_dict"), (lambda: m.load_state_dict({}), "load_state_dict")):
        with pytest.raises(RuntimeError, match=word + r"\(\).*keep_bf16=False"):
            call()
    with pytest.raises(RuntimeError, match="quantised already"):
        m.quantize_ff()
    from ltxmi import lora
    ad = lora.LoraAdapter({"transformer_blocks.0.ff.net.2": (torch.zeros(4, 512, dtype=torch.bfloat16), torch.zeros(128, 4, dtype=torch.bfloat16), None)})
    for call in (lambda: m.attach_lora(ad), lambda: m.fuse_lora(ad)):
        with pytest.raises(RuntimeError, match=r"unquantize_ff\(\) first"):
            call()
