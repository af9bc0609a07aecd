"""The mixed-precision host logic on the CPU doubles of ``ltxmi.ops`` -- run by tests/test_mixed_cpu.py in a process of its
own (``python tests/mixed_cpu_cases.py <case>``), because installing the doubles swaps functions of the ``ltxmi.ops`` module
for the whole process.  TEST INFRASTRUCTURE ONLY."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BF = torch.bfloat16
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_g16():
    from safetensors.torch import load_file
    with open(os.path.join(GOLDEN, "g16_mixed.json")) as f:
        meta = json.load(f)
    return load_file(os.path.join(GOLDEN, "g16_mixed.safetensors")), meta


def g16_state_dict(t, meta, layers):
    """fp32 copy of the weights of an L-layer case: block i = stored block i % stored_blocks (tools/make_golden_mixed.py)."""
    sd = {k[3:]: v.float() for k, v in t.items() if k.startswith("sd.")}
    out = {k: v for k, v in sd.items() if not k.startswith("transformer_blocks.")}
    for i in range(layers):
        src = f"transformer_blocks.{i % meta['stored_blocks']}."
        out.update({f"transformer_blocks.{i}." + k[len(src):]: v for k, v in sd.items() if k.startswith(src)})
    return out


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


class Holder:
    _interrupt = False


def _product_model(cfg, sd32):
    import ltxmi
    m = ltxmi.Transformer3DModel(**cfg)
    m.load_state_dict(sd32)
    return m.to(BF).eval()


def _g16_forward(m, t, meta, case, mixed):
    import ltxmi
    f, h, w = meta["grid"]
    kw = {}
    if case["strategy"] is not None:
        kw = dict(skip_layer_mask=m.create_skip_layer_mask(1, 3, 2, meta["skip_blocks"]),
                  skip_layer_strategy=getattr(ltxmi.SkipLayerStrategy, case["strategy"]))
    x = t["x"].clone() if mixed else t["x"].to(BF)
    with torch.no_grad():
        return m(x, freqs_cis=m.precompute_freqs_cis(t["indices_grid"]), encoder_hidden_states=t["enc"].to(BF),
                 encoder_attention_mask=t["mask"], timestep=t["ts_tok"] if case["per_token"] else t["ts"],
                 latent_shape=(f, h, w), ltxv_model=Holder(), mixed=mixed, return_dict=False, **kw)[0]


def case_model():
    """Transformer3DModel.forward(mixed=True) on the doubles against tests/mixed_oracle.py and the reference's own mixed
    output (G16): both timestep forms, all four strategies, the 8-layer case.  The doubles round where the kernels round, so
    the product's mixed rendering is held to the conditions the bf16 twin is held to (test_g5_transformer_bf16_twin)."""
    import cpu_ops_double_mixed
    cpu_ops_double_mixed.install()
    import mixed_oracle
    from oracle import dit
    t, meta = load_g16()
    strategies = {"AttentionValues": dit.ATTENTION_VALUES, "AttentionSkip": dit.ATTENTION_SKIP, "Residual": dit.RESIDUAL,
                  "TransformerBlock": dit.TRANSFORMER_BLOCK}
    for case in meta["cases"]:
        cfg = dict(meta["cfg"], num_layers=case["layers"])
        sd32 = g16_state_dict(t, meta, case["layers"])
        out = _g16_forward(_product_model(cfg, sd32), t, meta, case, True)
        assert out.dtype == BF, out.dtype
        kw = {}
        if case["strategy"] is not None:
            kw = dict(skip_layer_mask=dit.create_skip_layer_mask(case["layers"], 1, 3, 2, meta["skip_blocks"], torch.float32),
                      skip_layer_strategy=strategies[case["strategy"]])
        truth, oracle = mixed_oracle.oracles(sd32, cfg, t["x"], t["enc"], t["mask"], t["ts_tok"] if case["per_token"] else t["ts"],
                                             t["indices_grid"], tuple(meta["grid"]), **kw)
        ref = t[case["name"] + ".mixed"]
        e_ours, e_orc, e_ref = rel(out, truth), rel(oracle, truth), rel(ref, truth)
        print(f"{case['name']}: rel L2 vs fp32: product on the doubles {e_ours:.3e}, mixed oracle {e_orc:.3e}, reference "
              f"{e_ref:.3e}; product vs oracle {rel(out, oracle):.3e}, vs reference {rel(out, ref):.3e}")
        assert rel(out, oracle) < 1e-2 and rel(out, ref) < 1e-2, case["name"]
        assert e_ours < 2 * e_orc + 1e-3 and e_ours < 2 * e_ref + 1e-3, (case["name"], e_ours, e_orc, e_ref)
        if case["strategy"] in ("AttentionValues", "AttentionSkip", "TransformerBlock"):
            assert rel(out[2], out[1]) > 1e-3, case["name"]            # the perturbation acted


def case_rounding_points():
    """Where the block rounds: ``BasicTransformerBlock._forward_stream32`` hands the stream to the row kernels as
    norm1 -> gate(round_product=1, bf16 copy) -> gate(no gate) -> norm2 -> gate(round_product=0), all on ONE fp32 buffer; the
    GEMMs and attention see bf16 only.  (An L2 comparison at 3e-3 cannot tell a moved rounding point; the call record can.)"""
    import cpu_ops_double_mixed
    ops = cpu_ops_double_mixed.install()
    t, meta = load_g16()
    case = next(c for c in meta["cases"] if c["name"] == "L2.sample")
    m = _product_model(dict(meta["cfg"], num_layers=2), g16_state_dict(t, meta, 2))
    calls = []
    real = {n: getattr(ops, n) for n in ("norm_modulate_f32in", "gate_residual_f32_", "norm_modulate", "gemm", "attention")}

    def norm_f32in(x, out, *a, **k):
        calls.append(("norm", x.dtype, out.dtype, x.data_ptr()))
        return real["norm_modulate_f32in"](x, out, *a, **k)

    def gate(h, y, gate_table=None, gate_temb=None, rows_per_group=1, round_product=0, h_bf16=None):
        calls.append(("gate", None if gate_table is None else int(round_product), h_bf16 is not None, h.dtype, y.dtype, h.data_ptr()))
        return real["gate_residual_f32_"](h, y, gate_table, gate_temb, rows_per_group, round_product, h_bf16)

    def bf16_only(name):
        def fn(*a, **k):
            assert all(x.dtype == BF for x in a[:3] if torch.is_tensor(x)), name
            assert k.get("epilogue", 0) != ops.EPI_GATE_RESIDUAL, "a fused residual epilogue on the mixed path"
            return real[name](*a, **k)
        return fn

    def no_bf16_norm(*a, **k):
        raise AssertionError("the bf16 norm kernel ran on the mixed path")

    ops.norm_modulate_f32in, ops.gate_residual_f32_, ops.norm_modulate = norm_f32in, gate, no_bf16_norm
    ops.gemm, ops.attention = bf16_only("gemm"), bf16_only("attention")
    out = _g16_forward(m, t, meta, case, True)
    assert out.dtype == BF
    stream = calls[0][-1]
    per_block = [("norm", torch.float32, BF, stream), ("gate", 1, True, torch.float32, BF, stream),
                 ("gate", None, False, torch.float32, BF, stream), ("norm", torch.float32, BF, stream),
                 ("gate", 0, False, torch.float32, BF, stream)]
    assert calls == per_block * 2 + [("norm", torch.float32, BF, stream)], calls


def case_bf16_untouched():
    """The bf16 path on the double gives the same bits before the new doubles are installed and after a mixed forward ran
    on the same module."""
    import cpu_ops_double
    ops = cpu_ops_double.install()
    t, meta = load_g16()
    case = next(c for c in meta["cases"] if c["name"] == "L4.AttentionValues")
    cfg = dict(meta["cfg"], num_layers=4)
    m = _product_model(cfg, g16_state_dict(t, meta, 4))
    assert ops.norm_modulate_f32in.__module__ == "ltxmi.ops"            # the new doubles are not installed yet
    before = _g16_forward(m, t, meta, case, False)
    import cpu_ops_double_mixed
    cpu_ops_double_mixed.install()
    mixed = _g16_forward(m, t, meta, case, True)
    after = _g16_forward(m, t, meta, case, False)
    assert before.dtype == after.dtype == mixed.dtype == BF
    assert torch.equal(before, after)
    assert not torch.equal(mixed, after)


def case_pipeline():
    """LTXVideoPipeline.__call__(mixed_precision=True, output_type="latent") on the tiny model."""
    import cpu_ops_double_mixed
    cpu_ops_double_mixed.install()
    import ltxmi
    from oracle import dit
    cfg = dict(dit.default_2b_config(), num_attention_heads=2, attention_head_dim=64, num_layers=2, cross_attention_dim=128,
               caption_channels=128)
    m = _product_model(cfg, {k: v.to(BF).float() for k, v in dit.init_state_dict(cfg, seed=5).items()})
    g = torch.Generator().manual_seed(9)
    T = 12
    pos, neg = torch.randn(1, T, 128, generator=g).to(BF), torch.randn(1, T, 128, generator=g).to(BF)
    pmask, nmask = torch.ones(1, T), torch.ones(1, T)
    pmask[:, 8:] = 0
    nmask[:, 3:] = 0
    noise = torch.randn(1, 2 * 2 * 4, 128, generator=g)
    args = dict(height=64, width=128, num_frames=9, frame_rate=25.0, prompt_embeds=pos, prompt_attention_mask=pmask,
                negative_prompt_embeds=neg, negative_prompt_attention_mask=nmask, num_inference_steps=2, guidance_scale=3.0,
                stg_scale=1.0, rescaling_scale=0.7, skip_block_list=[1], skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues,
                latents=noise, output_type="latent", is_video=True, joint_pass=True, return_dict=False)
    pipe = ltxmi.LTXVideoPipeline(transformer=m, scheduler=ltxmi.RectifiedFlowScheduler(shifting="SD3", target_shift_terminal=0.1))
    calls = []
    forward = m.forward

    def recording(model_in, **kw):
        calls.append((model_in.dtype, kw.get("mixed")))
        out = forward(model_in, **kw)
        assert out[0].dtype == BF
        return out

    m.forward = recording
    plain = pipe(**args)[0]
    assert plain.dtype == BF and calls == [(BF, False)] * 2, (plain.dtype, calls)       # :1062: prompt_embeds' dtype
    del calls[:]
    out = pipe(mixed_precision=True, **args)[0]
    assert out.dtype == torch.float32 and out.shape == (1, 128, 2, 2, 4), (out.dtype, out.shape)      # :1061
    assert calls == [(BF, True)] * 2, calls
    assert torch.isfinite(out).all() and 0 < rel(out, plain) < 0.1, rel(out, plain)
    same = pipe(mixed_precision=True, latents_dtype=torch.float32, **args)[0]
    assert torch.equal(same, out)
    for bad in (BF, torch.float16):
        try:
            pipe(mixed_precision=True, latents_dtype=bad, **args)
        except ValueError as e:
            assert "mixed_precision" in str(e)
        else:
            raise AssertionError(f"latents_dtype={bad} with mixed_precision=True was accepted")
    # the multi-scale wrapper hands the flag through like every other keyword
    seen = {}

    class Recorder:
        vae = None
        vae_scale_factor = 32

        def __call__(self, *a, **kw):
            seen.setdefault("mixed_precision", []).append(kw.get("mixed_precision"))
            return None

    ms = ltxmi.LTXMultiScalePipeline(Recorder(), None)
    assert ms(0.5, {}, {}, output_type="latent", height=64, width=128, prompt_embeds=pos, mixed_precision=True) is None
    assert seen["mixed_precision"] == [True]


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]]()
    print("ok")
