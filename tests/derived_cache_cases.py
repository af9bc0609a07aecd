"""The two step-invariant cache sites (caption projection, per-layer text K/V) through the model's host logic on the CPU
doubles of ``ltxmi.ops`` -- run by tests/test_derived_cache.py in a process of its own (``python tests/derived_cache_cases.py
<case>``), because installing the doubles swaps functions of the ``ltxmi.ops`` module for the whole process.
TEST INFRASTRUCTURE ONLY."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BF = torch.bfloat16


def setup(double="cpu_ops_double"):
    """test_host_logic's tiny DiT (4 heads of 64, 3 layers, B = 3, N = 24, 12 text tokens) on the doubles:
    (ops, cfg, model, forward() -> out, calls) where ``calls`` counts the caption projections and the text K/V GEMMs."""
    ops = __import__(double).install()
    import ltxmi
    from oracle import dit, sched
    cfg = dict(dit.default_2b_config(), num_attention_heads=4, attention_head_dim=64, num_layers=3, cross_attention_dim=256,
               caption_channels=128)
    sd = {k: v.to(BF).float() for k, v in dit.init_state_dict(cfg, seed=3).items()}
    f, h, w = 2, 3, 4
    N, B, T = f * h * w, 3, 12
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, N, 128, generator=g).to(BF)
    enc = torch.randn(B, T, 128, generator=g).to(BF)
    mask = torch.ones(B, T)
    mask[:, 8:] = 0
    m = ltxmi.Transformer3DModel(**cfg)
    m.load_state_dict(sd)
    m = m.to(BF).eval()
    fc = m.precompute_freqs_cis(sched.fractional_coords(f, h, w, 1, 25.0))
    calls = {"caption": 0, "text_kv": 0}

    caption_forward = m.caption_projection.forward

    def counted_caption(*a, **k):
        calls["caption"] += 1
        return caption_forward(*a, **k)
    m.caption_projection.forward = counted_caption

    gemm = ops.gemm

    def counted_gemm(a, w, *rest, **k):
        if a.shape[0] == B * T and w.shape[0] == 2 * 256:          # [B T, Dc] against a [to_k; to_v]: a text K/V projection
            calls["text_kv"] += 1
        return gemm(a, w, *rest, **k)
    ops.gemm = counted_gemm

    def forward():
        with torch.no_grad():
            return m(x.clone(), freqs_cis=fc, encoder_hidden_states=enc, encoder_attention_mask=mask,
                     timestep=torch.full((B, 1), 0.7), latent_shape=(f, h, w), return_dict=False)[0]
    return ops, cfg, m, forward, calls


def case_caption_bias():
    """Same prompt tensor: one projection for two forwards; an in-place edit of linear_1.bias projects again and changes the
    output (the key once held the two weights only)."""
    ops, cfg, m, forward, calls = setup()
    first = forward()
    assert torch.equal(forward(), first) and calls["caption"] == 1
    with torch.no_grad():
        m.caption_projection.linear_1.bias.add_(1.0)
    edited = forward()
    assert calls["caption"] == 2
    assert not torch.equal(edited, first)
    assert torch.equal(forward(), edited) and calls["caption"] == 2


def case_k_norm_weight():
    """The text K/V: once per layer for two forwards; an in-place edit of one layer's k_norm.weight rebuilds that layer's."""
    ops, cfg, m, forward, calls = setup()
    layers = cfg["num_layers"]
    first = forward()
    assert torch.equal(forward(), first) and calls["text_kv"] == layers
    with torch.no_grad():
        m.transformer_blocks[1].attn2.k_norm.weight.mul_(1.5)
    edited = forward()
    assert calls["text_kv"] == layers + 1
    assert not torch.equal(edited, first)
    assert torch.equal(forward(), edited) and calls["text_kv"] == layers + 1


def case_caching_off():
    """set_step_invariant_caching(False): every forward does the work and nothing is stored."""
    ops, cfg, m, forward, calls = setup()
    ops.set_step_invariant_caching(False)
    ops.STACKED_TEXT_KV = False                        # the per-layer projections, so that the text K/V site itself is asked
    first = forward()
    assert torch.equal(forward(), first)
    assert calls == {"caption": 2, "text_kv": 2 * cfg["num_layers"]}
    assert "caption" not in m.derived_slots()
    assert all("text_kv" not in b.attn2.derived_slots() for b in m.transformer_blocks)
    ops.set_step_invariant_caching(True)
    assert torch.equal(forward(), first) and torch.equal(forward(), first)
    assert calls == {"caption": 3, "text_kv": 3 * cfg["num_layers"]}
    assert "caption" in m.derived_slots() and all("text_kv" in b.attn2.derived_slots() for b in m.transformer_blocks)


def case_lora_epoch():
    """An adapter on to_k: set_lora_weights touches no weight, yet the text K/V are rebuilt (the adapter epoch is in the key)."""
    from lora_cpu_cases import make_adapter_sd
    from ltxmi import loading
    ops, cfg, m, forward, calls = setup("cpu_ops_double_lora")
    layers = cfg["num_layers"]
    m.attach_lora(loading.load_lora(make_adapter_sd(cfg, 16, seed=7, targets=("attn2.to_k",), scale=2.0)), name="k")
    one = forward()
    assert torch.equal(forward(), one) and calls["text_kv"] == layers
    m.set_lora_weights({"k": 3.0})
    three = forward()
    assert calls["text_kv"] == 2 * layers and not torch.equal(three, one)
    assert torch.equal(forward(), three) and calls["text_kv"] == 2 * layers and calls["caption"] == 1


CASES = {"caption_bias": case_caption_bias, "k_norm_weight": case_k_norm_weight, "caching_off": case_caching_off,
         "lora_epoch": case_lora_epoch}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
