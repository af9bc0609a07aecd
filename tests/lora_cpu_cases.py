"""LoRA adapters through the host logic on the CPU doubles of ``ltxmi.ops`` -- run by tests/test_lora_cpu.py in a process of its
own (``python tests/lora_cpu_cases.py <case>``), because installing the doubles swaps functions of the ``ltxmi.ops`` module for
the whole process.  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BF = torch.bfloat16
F64 = torch.float64


class Holder:
    _interrupt = False


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def make_adapter_sd(cfg, rank, seed, targets=None, alpha=None, blocks=None, prefix="", spelling="A", scale=0.5):
    """A LoRA state dict for a model of ``cfg``: bf16 down [r, in] ~ in^-1/2, up [out, r] ~ scale r^-1/2 on ``targets`` (default: the
    ten linears of every block)."""
    from ltxmi import lora
    D = cfg["num_attention_heads"] * cfg["attention_head_dim"]
    Dc = cfg["cross_attention_dim"]
    dims = {"attn1.to_q": (D, D), "attn1.to_k": (D, D), "attn1.to_v": (D, D), "attn1.to_out.0": (D, D),
            "attn2.to_q": (D, D), "attn2.to_k": (D, Dc), "attn2.to_v": (D, Dc), "attn2.to_out.0": (D, D),
            "ff.net.0.proj": (4 * D, D), "ff.net.2": (D, 4 * D)}
    g = torch.Generator().manual_seed(seed)
    down_name, up_name = ("lora_A", "lora_B") if spelling == "A" else ("lora_down", "lora_up")
    sd = {}
    for i in (range(cfg["num_layers"]) if blocks is None else blocks):
        for t in (lora.BLOCK_TARGETS if targets is None else targets):
            n_out, n_in = dims[t]
            path = f"{prefix}transformer_blocks.{i}.{t}"
            sd[f"{path}.{down_name}.weight"] = (torch.randn(rank, n_in, generator=g) * n_in ** -0.5).to(BF)
            sd[f"{path}.{up_name}.weight"] = (torch.randn(n_out, rank, generator=g) * scale * rank ** -0.5).to(BF)
            if alpha is not None:
                sd[f"{path}.alpha"] = torch.tensor(float(alpha))
    return sd


def merged(sd, adapters):
    """float64 weights W + s B A for ``adapters`` = [(LoraAdapter, weight)]: the truth of the unmerged formula."""
    out = {k: v.to(F64) for k, v in sd.items()}
    for adapter, weight in adapters:
        for path, (down, up, _) in adapter.modules.items():
            out[path + ".weight"] = out[path + ".weight"] + adapter.scale(path, weight) * (up.to(F64) @ down.to(F64))
    return out


def setup(num_layers=2, seed=0):
    """smoke()'s tiny DiT on the doubles: (ltxmi, cfg, bf16-valued fp32 state dict, model, forward(model) -> out, oracle(sd64) -> truth)."""
    import cpu_ops_double_lora
    cpu_ops_double_lora.install()
    import ltxmi
    from oracle import dit, sched
    cfg = dict(dit.default_2b_config(), num_attention_heads=2, attention_head_dim=64, num_layers=num_layers,
               cross_attention_dim=128, caption_channels=128)
    sd = {k: v.to(BF).float() for k, v in dit.init_state_dict(cfg, seed=seed).items()}
    f, h, w, B, T = 2, 4, 6, 3, 16
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, f * h * w, 128, generator=g).to(BF)
    enc = torch.randn(B, T, 128, generator=g).to(BF)
    mask = torch.ones(B, T)
    mask[:, 10:] = 0
    ts = torch.full((B, 1), 0.7)
    frac = sched.fractional_coords(f, h, w, 1, 25.0)
    m = ltxmi.Transformer3DModel(**cfg)
    m.load_state_dict(sd)
    m = m.to(BF).eval()

    def forward(model=m, mixed=False, enc_t=enc):
        with torch.no_grad():
            return model(x.float() if mixed else x.clone(), freqs_cis=model.precompute_freqs_cis(frac), encoder_hidden_states=enc_t,
                         encoder_attention_mask=mask, timestep=ts, skip_layer_mask=model.create_skip_layer_mask(1, 3, 2, [1]),
                         skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues, latent_shape=(f, h, w),
                         ltxv_model=Holder(), mixed=mixed, return_dict=False)[0]

    def oracle(sd64):
        skip = dit.create_skip_layer_mask(num_layers, 1, 3, 2, [1], F64)
        return dit.transformer3d_forward(sd64, cfg, x.to(F64), dit.precompute_freqs_cis(frac, cfg, F64), enc.to(F64), ts.to(F64),
                                         encoder_attention_mask=mask.to(F64), latent_shape=(f, h, w), skip_layer_mask=skip,
                                         skip_layer_strategy=dit.ATTENTION_VALUES)

    return ltxmi, cfg, sd, m, forward, oracle


def case_attach_detach():
    """Detach restores bit-identical outputs; an adapter with zero up matrices changes no value; the per-linear state exists
    only while an adapter is attached; the mixed-precision block takes the adapters too."""
    from ltxmi import loading
    ltxmi, cfg, sd, m, forward, _ = setup()
    base, base_mixed = forward(), forward(mixed=True)
    ad = loading.load_lora(make_adapter_sd(cfg, 16, seed=5))
    assert m.attach_lora(ad, name="a") == [] and m.lora_names() == ["a"]
    slots = m.transformer_blocks[0].attn1.__dict__["_lora"]
    assert set(slots) == {"qkv", "out"} and slots["qkv"].down.shape == (3 * 64, 128) and slots["qkv"].up.shape == (3 * 128, 64)
    assert slots["qkv"].group_cols == 128 and slots["out"].group_cols == 0
    with_a, with_a_mixed = forward(), forward(mixed=True)
    assert rel(with_a, base) > 1e-2 and rel(with_a_mixed, base_mixed) > 1e-2, "the adapter did nothing"
    assert rel(with_a_mixed, with_a) < 2e-2
    m.detach_lora("a")
    assert m.lora_names() == [] and all(b.attn1.__dict__["_lora"] is None and b.ff.__dict__["_lora"] is None for b in m.transformer_blocks)
    assert torch.equal(forward(), base) and torch.equal(forward(mixed=True), base_mixed)
    zero_sd = {k: (torch.zeros_like(v) if ".lora_B." in k else v) for k, v in make_adapter_sd(cfg, 16, seed=5).items()}
    m.attach_lora(loading.load_lora(zero_sd))
    assert m.transformer_blocks[1].ff.__dict__["_lora"]["ff1"].down.abs().max() > 0
    assert torch.equal(forward(), base) and torch.equal(forward(mixed=True), base_mixed), "zero up matrices changed a value"
    m.detach_lora()
    assert torch.equal(forward(), base)
    # a partial adapter: one member of a packed projection, one block
    part = loading.load_lora(make_adapter_sd(cfg, 16, seed=6, targets=("attn1.to_k", "attn2.to_v"), blocks=[1]))
    m.attach_lora(part)
    assert m.transformer_blocks[0].attn1.__dict__["_lora"] is None
    s = m.transformer_blocks[1].attn1.__dict__["_lora"]["qkv"]
    assert float(s.up[:128].abs().max()) == 0 and float(s.up[128:256].abs().max()) > 0 and float(s.down[:64].abs().max()) == 0
    assert rel(forward(), base) > 1e-4


def case_arithmetic():
    """Two adapters at weights (0.5, 2.0) equal their single concatenated adapter (down stacked along r, up side by side with the
    weights folded in) bit for bit; rank 16 pads to 64; alpha / r scales."""
    from ltxmi import loading, lora
    ltxmi, cfg, sd, m, forward, _ = setup()
    sd_a, sd_b = make_adapter_sd(cfg, 16, seed=5), make_adapter_sd(cfg, 64, seed=6, alpha=32.0)
    a, b = loading.load_lora(sd_a), loading.load_lora(sd_b)
    assert a.scale("transformer_blocks.0.attn1.to_q", 0.5) == 0.5 and b.scale("transformer_blocks.0.attn1.to_q", 2.0) == 1.0
    m.attach_lora(a, weight=0.5, name="a")
    m.attach_lora(b, weight=2.0, name="b")
    s = m.transformer_blocks[0].ff.__dict__["_lora"]["ff2"]
    assert s.down.shape == (128, 512) and s.up.shape == (128, 128)          # 16 + 64 = 80 -> 128
    assert float(s.down[80:].abs().max()) == 0 and float(s.up[:, 80:].abs().max()) == 0
    two = forward()
    m.detach_lora()
    cat = {}
    for path in a.modules:
        (da, ua, _), (db, ub, _) = a.modules[path], b.modules[path]
        # the concatenated adapter carries bf16(s_i B_i), which is what the two adapters' state holds
        cat[path + ".lora_A.weight"] = torch.cat([da, db], 0)
        cat[path + ".lora_B.weight"] = torch.cat([(ua.float() * 0.5).to(BF), (ub.float() * 1.0).to(BF)], 1)
    m.attach_lora(loading.load_lora(cat), name="cat")
    assert torch.equal(forward(), two)
    m.set_lora_weights({"cat": 0.0})
    base = forward()
    m.detach_lora()
    assert torch.equal(forward(), base)
    # rank 16 alone pads to 64
    m.attach_lora(a)
    s = m.transformer_blocks[0].attn2.__dict__["_lora"]
    assert s["q"].down.shape == (64, 128) and s["kv"].down.shape == (128, 128) and s["kv"].up.shape == (256, 64)
    assert lora.RANK_PAD == 64


def case_oracle():
    """A two-block model with adapters on all ten linears against oracle/dit.py run in float64 on MERGED weights W + s B A: the
    bound is the one the tiny bf16 DiT is held to against its fp32 oracle (2e-2 relative L2, __graft_entry__.smoke), and the
    adapters may not cost more than twice the error of the same model without them."""
    from ltxmi import loading
    ltxmi, cfg, sd, m, forward, oracle = setup()
    e_base = rel(forward(), oracle(merged(sd, [])))
    a, b = loading.load_lora(make_adapter_sd(cfg, 16, seed=5)), loading.load_lora(make_adapter_sd(cfg, 64, seed=6, alpha=32.0))
    m.attach_lora(a, weight=0.5)
    m.attach_lora(b, weight=2.0)
    out = forward()
    truth = oracle(merged(sd, [(a, 0.5), (b, 2.0)]))
    e = rel(out, truth)
    moved = rel(truth, oracle(merged(sd, [])))
    print(f"rel L2 vs float64 merged oracle: with adapters {e:.3e}, without {e_base:.3e}; the adapters move the output by {moved:.3e}")
    assert moved > 5e-2, "the adapters are too weak to test anything"
    assert e < 2e-2 and e < 2 * e_base + 1e-3, (e, e_base)
    e_mixed = rel(forward(mixed=True), truth)
    print(f"mixed=True: {e_mixed:.3e}")
    assert e_mixed < 2e-2


def case_caches():
    """The per-layer text K/V caches key on weights and the prompt tensor; an adapter on to_k / to_v changes the projection
    without touching either.  A changed set_lora_weights between two forwards with the SAME prompt tensor must change the
    cross-attention output; the stacked text K/V projection steps aside while such an adapter is attached."""
    from ltxmi import loading, ops
    ltxmi, cfg, sd, m, forward, _ = setup()
    assert ops.STEP_INVARIANT_CACHING
    base = forward()
    kv = loading.load_lora(make_adapter_sd(cfg, 16, seed=7, targets=("attn2.to_k", "attn2.to_v"), scale=2.0))
    m.attach_lora(kv, name="kv")
    one = forward()
    assert rel(one, base) > 1e-3, "attach: the cached text K/V of the base weights was served"
    assert torch.equal(forward(), one)
    m.set_lora_weights({"kv": 3.0})
    three = forward()
    assert rel(three, one) > 1e-3, "set_lora_weights: a stale text K/V cache was served"
    m.set_lora_weights({"kv": 0.0})
    assert torch.equal(forward(), base), "weight 0 is not the base model: a stale text K/V cache was served"
    m.set_lora_weights({"kv": 1.0})
    assert torch.equal(forward(), one)
    m.detach_lora()
    assert torch.equal(forward(), base), "detach: a stale text K/V cache was served"
    # without step-invariant caching a joint pass uses the stacked projection: not with an adapter on a to_k / to_v
    ops.set_step_invariant_caching(False)
    try:
        m.derived("stacked_kv").clear()
        base2 = forward()
        assert torch.equal(base2, base)
        m.attach_lora(kv, name="kv")
        assert torch.equal(forward(), one)
        m.detach_lora()
    finally:
        ops.set_step_invariant_caching(True)


CASES = {"attach_detach": case_attach_detach, "arithmetic": case_arithmetic, "oracle": case_oracle, "caches": case_caches}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
