"""The quantised T5 encoder on the CPU: the patched restatement tests/t5_mx8_double.py against tests/t5_double.py, and what of
``T5EncoderModel.quantize`` needs no device -- the names, the refusals and the life cycle of the per-module state."""
import inspect

import pytest
import torch

import mx8_cases as mc
import t5_double as td
import t5_mx8_double as tq

BF = torch.bfloat16


def _weights(cfg=td.TINY, seed=0):
    return {k: v.to(BF) for k, v in td.init_state_dict(cfg, seed=seed, stream=30.0, qk_gain=0.5).items()}


@pytest.mark.parametrize("dt", [torch.float64, BF], ids=["float64", "bfloat16"])
def test_with_no_linear_chosen_the_restatement_is_t5_double(dt):
    sd = {k: v.to(dt) for k, v in _weights().items()}
    ids, mask = td.tiny_inputs()
    assert torch.equal(tq.encoder_forward(sd, td.TINY, ids, mask, linears=()), td.encoder_forward(sd, td.TINY, ids, mask))


def test_qdq_is_the_format_restatement():
    x = mc.quant_input("row_scales", 37, 256)
    assert torch.equal(tq.qdq(x), mc.dequantize(*mc.quantize(x), BF))
    assert torch.equal(tq.qdq(x.double()), mc.dequantize(*mc.quantize(x)))
    w = mc.witness_rows(64)
    assert torch.equal(tq.qdq(w).double(), mc.dequantize(*mc.quantize(w)))
    assert tq.qdq(x.reshape(37, 2, 128)).shape == (37, 2, 128)


def test_every_chosen_linear_moves_the_output_and_the_format_costs_what_was_measured():
    """Float64 throughout, so only the format is seen: each linear alone moves the output, the four together by an rms of
    0.06 - 0.09 of an output of rms 1 (measured 0.074 - 0.077 on this config, seeds 0 - 2): two rounded operands cost about 5 % per
    projection, and the stream adds them up."""
    sd = {k: v.double() for k, v in _weights().items()}
    ids, mask = td.tiny_inputs()
    plain = td.encoder_forward(sd, td.TINY, ids, mask)
    for name in tq.LINEARS:
        one = tq.encoder_forward(sd, td.TINY, ids, mask, linears=(name,))
        assert torch.isfinite(one).all() and td.errors(one, plain)[1] > 1e-3, name
    cost = td.errors(tq.encoder_forward(sd, td.TINY, ids, mask), plain)
    print(f"format cost on tiny: max abs {cost[0]:.3g}, rms {cost[1]:.3g}; |plain| rms {float(plain.pow(2).mean().sqrt()):.3g}")
    assert 0.03 < cost[1] < 0.15


def _model(cfg=td.TINY, dtype=BF):
    import ltxmi
    m = ltxmi.T5EncoderModel(dict(cfg))
    m.load_state_dict(td.init_state_dict(cfg, seed=0))
    return m.to(dtype).eval()


def _state(mod):
    return mod.__dict__.get("_mx8")


def test_quantize_life_cycle_without_a_device():
    from ltxmi import t5_mx8
    m = _model()
    att, ff = m.encoder.block[1].layer[0].SelfAttention, m.encoder.block[1].layer[1].DenseReluDense
    keys = list(m.state_dict())
    assert m.quantized is False and m.quantized_linears == () and _state(att) is None and _state(ff) is None
    assert m.quantize() is m
    assert m.quantized is True and m.quantized_linears == t5_mx8.DEFAULT_LINEARS
    assert set(t5_mx8.DEFAULT_LINEARS) <= set(t5_mx8.LINEARS) == {"qkv", "o", "wi", "wo"}
    assert _state(att).chosen == frozenset(t5_mx8.DEFAULT_LINEARS) & {"qkv", "o"} and _state(att).sealed is None
    assert _state(ff).chosen == frozenset(t5_mx8.DEFAULT_LINEARS) & {"wi", "wo"}
    assert list(m.state_dict()) == keys                           # keep_bf16=True: the parameters are all there
    with pytest.raises(RuntimeError, match="quantised already"):
        m.quantize()
    assert m.unquantize() is m
    assert m.quantized is False and _state(att) is None and _state(ff) is None
    m.unquantize()                                                # nothing to undo is no error
    # any subset, in any order; a module without a chosen linear carries no state
    m.quantize(linears=("wo", "qkv"))
    assert m.quantized_linears == ("qkv", "wo") and _state(att).chosen == {"qkv"} and _state(ff).chosen == {"wo"}
    m.unquantize()
    m.quantize(linears=["o"])
    assert _state(att).chosen == {"o"} and _state(ff) is None
    m.unquantize()
    m.quantize(linears=())
    assert m.quantized is False and _state(att) is None
    with pytest.raises(ValueError, match="unknown linear 'wi_0'"):
        m.quantize(linears=("qkv", "wi_0"))
    assert m.quantized is False
    # .to() keeps the state (the cache behind it is keyed on the parameters' storage)
    m.quantize()
    m.to(torch.bfloat16)
    assert m.quantized and _state(att) is not None


def test_quantize_refuses_shapes_and_dtypes_the_gemm_cannot_take():
    m = _model(dict(td.TINY, d_model=192))                         # K = 192 for qkv and wi; o and wo have K = 128 / 256
    with pytest.raises(ValueError, match=r"SelfAttention\.qkv is \(128, 192\).*in_features % 128"):
        m.quantize()
    assert m.quantized is False and _state(m.encoder.block[0].layer[0].SelfAttention) is None      # nothing was set
    with pytest.raises(ValueError, match=r"DenseReluDense\.wi is"):
        m.quantize(linears=("wi", "wo"))
    m.quantize(linears=("o", "wo"))                               # N = 192 is a multiple of 32
    m.unquantize()
    m = _model(dict(td.TINY, d_ff=160))
    with pytest.raises(ValueError, match=r"DenseReluDense\.wo is \(128, 160\)"):
        m.quantize(linears=("wo",))
    m.quantize(linears=("qkv", "o", "wi"))
    with pytest.raises(TypeError, match="bfloat16"):
        _model(dtype=torch.float32).quantize()
    with pytest.raises(TypeError, match="quantised on the GPU"):
        _model().quantize(keep_bf16=False)


def test_the_loader_takes_mx8_and_defaults_to_bf16():
    from ltxmi import loading
    p = inspect.signature(loading.load_t5_encoder).parameters
    assert list(p)[:4] == ["path_or_state_dict", "config", "device", "dtype"] and p["mx8"].default is False
    m = loading.load_t5_encoder(_weights(), dict(td.TINY), device="cpu")
    assert m.quantized is False
    with pytest.raises(TypeError, match="quantised on the GPU"):
        loading.load_t5_encoder(_weights(), dict(td.TINY), device="cpu", mx8=True)
