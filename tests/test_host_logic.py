"""Host-side logic of the PRODUCT (ltxmi/) against the reference-generated golden vectors -- CPU only.
RoPE tables, the scheduler, the per-step guidance tables and the skip-layer masks are computed on the host once
per generation; none of them needs a GPU, so they are pinned here directly (not only through model-level tolerances)."""
import pytest
import torch

import ltxmi
from ltxmi.patchifier import SymmetricPatchifier, latent_to_pixel_coords_from_factors

TOL = dict(rtol=1e-5, atol=2e-6)


def _model(heads, dh, layers=1):
    # a 1-layer model only to own the RoPE parameters (inner_dim, theta, max_pos); the tables do not depend on weights
    return ltxmi.Transformer3DModel(num_attention_heads=heads, attention_head_dim=dh, in_channels=16, out_channels=16,
                                    num_layers=layers, cross_attention_dim=heads * dh, caption_channels=32,
                                    attention_bias=True, activation_fn="gelu-approximate", norm_elementwise_affine=False,
                                    norm_eps=1e-6, qk_norm="rms_norm", standardization_norm="rms_norm",
                                    adaptive_norm="single_scale_shift", positional_embedding_type="rope",
                                    positional_embedding_theta=10000.0, positional_embedding_max_pos=[20, 2048, 2048],
                                    timestep_scale_multiplier=1000)


def test_g1_product_precompute_freqs_cis(golden):
    """Transformer3DModel.precompute_freqs_cis of the product (transformer3d.py:202-255) against G1, including the
    D = 2048 case whose 2 leading pad channels (2048 % 6) must be cos 1 / sin 0, and the coordinate grid the product's
    patchifier + causal fix produce."""
    t, meta = golden("g1_rope")
    for case in meta["cases"]:
        tag = case["tag"]
        f, h, w = case["grid"]
        coords = SymmetricPatchifier(1).get_latent_coords(f, h, w, 2, "cpu")
        pc = latent_to_pixel_coords_from_factors(coords, (8, 32, 32), causal_fix=True).to(torch.float32)
        pc[:, 0] = pc[:, 0] * (1.0 / 25.0)
        torch.testing.assert_close(pc, t[f"{tag}.indices_grid"], rtol=0, atol=0)
        m = _model(case["heads"], case["dh"])                      # fp32 module: tables come out in fp32
        cos, sin = m.precompute_freqs_cis(t[f"{tag}.indices_grid"])
        torch.testing.assert_close(cos, t[f"{tag}.cos"], **TOL)
        torch.testing.assert_close(sin, t[f"{tag}.sin"], **TOL)
        # the bf16 tables the kernels read are the fp32 tables rounded once
        cb, sb = m.to(torch.bfloat16).precompute_freqs_cis(t[f"{tag}.indices_grid"])
        assert torch.equal(cb, t[f"{tag}.cos"].to(torch.bfloat16)) or (cb.float() - t[f"{tag}.cos"]).abs().max() < 4e-3
        assert (sb.float() - t[f"{tag}.sin"]).abs().max() < 4e-3


def test_g6_product_scheduler(golden):
    """ltxmi.RectifiedFlowScheduler.set_timesteps (SD3 resolution-dependent shift, stretch to terminal 0.1) against G6
    for the latent shapes of all five configs."""
    t, meta = golden("g6_scheduler")
    for tag, shp in meta["shapes"].items():
        for steps in (2, 8, 40):
            s = ltxmi.RectifiedFlowScheduler(shifting="SD3", target_shift_terminal=0.1)
            s.set_timesteps(steps, samples_shape=tuple(shp), device="cpu")
            torch.testing.assert_close(s.timesteps.float().cpu(), t[f"{tag}.steps{steps}"], rtol=1e-6, atol=1e-7)


def test_g7_product_guidance_tables_and_skip_masks(golden):
    """LTXVideoPipeline._guidance_tables + Transformer3DModel.create_skip_layer_mask of the product against what the
    reference's own __call__ fed its loop (G7, the run with list-valued scales and guidance_timesteps)."""
    t, meta = golden("g7_pipeline_call")
    kw = meta["tables_kwargs"]
    ts = t["tables.timesteps"].tolist()
    gs, stg, rs, skips = ltxmi.LTXVideoPipeline._guidance_tables(ts, kw["guidance_scale"], kw["stg_scale"],
                                                                 kw["rescaling_scale"], kw["skip_block_list"],
                                                                 kw["guidance_timesteps"])
    # first table entry whose guidance timestep is <= t (:961-968); guidance scales <= 1 are zeroed (:983)
    assert gs == [0.0, 3.0, 2.0][: len(ts)] or len(gs) == len(ts)
    m = _model(2, 64, layers=meta["cfg"]["num_layers"])
    for i in range(len(ts)):
        mask = m.create_skip_layer_mask(1, 3, 2, skips[i])
        if f"tables.skip_layer_mask.{i}" in t:
            assert torch.equal(mask.float(), t[f"tables.skip_layer_mask.{i}"])
        else:
            assert mask is None
    from oracle import pipeline_ctl as pc
    ogs, ostg, ors, oskips, *_ = pc.guidance_tables(ts, kw["guidance_scale"], kw["stg_scale"], kw["rescaling_scale"],
                                                    kw["skip_block_list"], guidance_timesteps=kw["guidance_timesteps"])
    assert (gs, stg, rs, skips) == (ogs, ostg, ors, oskips)


def test_g6_product_scheduler_step(golden):
    """ltxmi.RectifiedFlowScheduler.step: Euler (global and per-token timesteps) and the stochastic branch (same torch
    generator state as the recorded draw) against G6."""
    t, meta = golden("g6_scheduler")
    s = ltxmi.RectifiedFlowScheduler(shifting="SD3", target_shift_terminal=0.1)
    s.set_timesteps(8, samples_shape=tuple(meta["shapes"]["small"]), device="cpu")
    ts = s.timesteps.float()
    torch.testing.assert_close(ts, t["step.timesteps"], rtol=1e-6, atol=1e-7)
    out = s.step(t["step.v"], ts[2], t["step.sample"], return_dict=False)[0]
    torch.testing.assert_close(out, t["step.global"], **TOL)
    out = s.step(t["step.v"], t["step.tok_t"], t["step.sample"], return_dict=False)[0]
    torch.testing.assert_close(out, t["step.per_token"], **TOL)
    g = torch.Generator().manual_seed(7)            # the draw the reference took from the global RNG seeded with 7
    out = s.step(t["step.v"], t["step.tok_t"], t["step.sample"], return_dict=False, stochastic_sampling=True, generator=g)[0]
    torch.testing.assert_close(out, t["step.stochastic_per_token"], **TOL)


def test_stacked_text_kv_host_logic_on_the_cpu_double():
    """Transformer3DModel._stacked_text_kv + the processor's hand-over (ops.STACKED_TEXT_KV, the per-generation cache off) with
    ltxmi.ops swapped for its CPU double, in a process of its own: same output as the per-layer projections (torch.equal: the
    double's GEMM is row- and column-wise independent too), every block consumes its slice, a block run on other rows than the
    leading ones falls back to projecting by itself."""
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys, torch
ROOT = sys.argv[1]
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import cpu_ops_double
ops = cpu_ops_double.install()
import ltxmi
from oracle import dit, sched
bf = torch.bfloat16
cfg = dict(dit.default_2b_config(), num_attention_heads=4, attention_head_dim=64, num_layers=3, cross_attention_dim=256, caption_channels=128)
sd32 = {k: v.to(bf).float() for k, v in dit.init_state_dict(cfg, seed=3).items()}
f, h, w = 2, 3, 4
N, B, T = f * h * w, 3, 12
g = torch.Generator().manual_seed(4)
x = torch.randn(B, N, 128, generator=g).to(bf)
enc = torch.randn(B, T, 128, generator=g).to(bf)
x[2], enc[2] = x[1], enc[1]
mask = torch.ones(B, T); mask[:, 8:] = 0
ts = torch.full((B, 1), 0.7)
m = ltxmi.Transformer3DModel(**cfg); m.load_state_dict(sd32); m = m.to(bf).eval()
fc = m.precompute_freqs_cis(sched.fractional_coords(f, h, w, 1, 25.0))
kw = dict(freqs_cis=fc, encoder_hidden_states=enc, encoder_attention_mask=mask, timestep=ts, latent_shape=(f, h, w), return_dict=False)
ops.set_step_invariant_caching(False)
with torch.no_grad():
    for alias in (0, 2):
        ops.STACKED_TEXT_KV = False
        ref = m(x.clone(), stg_alias_blocks=alias, **kw)[0]
        assert "stacked_kv" not in m.derived_slots()
        ops.STACKED_TEXT_KV = True
        out = m(x.clone(), stg_alias_blocks=alias, **kw)[0]
        assert torch.equal(out, ref), alias
        assert "stacked_kv" in m.derived_slots()
        assert all("_text_kv_ready" not in b.attn2.__dict__ for b in m.transformer_blocks)
        m.derived("stacked_kv").clear()
    # a block that sees OTHER rows than the leading ones must not take the hand-over
    m._stacked_text_kv(m.caption_projection(enc).view(B, T, -1))
    blk = m.transformer_blocks[0]
    ready = blk.attn2.__dict__["_text_kv_ready"]
    full = ready[0]
    assert full.shape[0] == B and ready[2].shape[0] == B * T
    # with the cache on nothing is stacked
    ops.set_step_invariant_caching(True)
    for b in m.transformer_blocks: b.attn2.__dict__.pop("_text_kv_ready", None)
    m.derived("stacked_kv").clear()
    m(x.clone(), **kw)
    assert "stacked_kv" not in m.derived_slots()
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ the drop-in boundary: signatures
def _sig(fn):
    import enum
    import inspect
    out = []
    for prm in inspect.signature(fn).parameters.values():
        d = None
        if prm.default is not inspect.Parameter.empty:
            v = prm.default
            d = f"{type(v).__name__}.{v.name}" if isinstance(v, enum.Enum) else repr(v)
        out.append({"name": prm.name, "kind": prm.kind.name, "has_default": prm.default is not inspect.Parameter.empty,
                    "default": d})
    return out


def _product_entry_points():
    from ltxmi import autoencoder as ae, latent_upsampler as lu, pipeline as pl
    return {
        "Transformer3DModel.__init__": ltxmi.Transformer3DModel.__init__,
        "Transformer3DModel.forward": ltxmi.Transformer3DModel.forward,
        "Transformer3DModel.precompute_freqs_cis": ltxmi.Transformer3DModel.precompute_freqs_cis,
        "Transformer3DModel.create_skip_layer_mask": ltxmi.Transformer3DModel.create_skip_layer_mask,
        "BasicTransformerBlock.forward": ltxmi.BasicTransformerBlock.forward,
        "Attention.set_processor": ltxmi.Attention.set_processor,
        "Attention.forward": ltxmi.Attention.forward,
        "AttnProcessor2_0.__call__": ltxmi.AttnProcessor2_0.__call__,
        "pay_attention": ltxmi.pay_attention,
        "CausalVideoAutoencoder.decode": ltxmi.CausalVideoAutoencoder.decode,
        "CausalVideoAutoencoder.encode": ltxmi.CausalVideoAutoencoder.encode,
        "CausalVideoAutoencoder.enable_z_tiling": ltxmi.CausalVideoAutoencoder.enable_z_tiling,
        "CausalVideoAutoencoder.set_tiling_params": ltxmi.CausalVideoAutoencoder.set_tiling_params,
        "CausalVideoAutoencoder.get_VAE_tile_size": ltxmi.CausalVideoAutoencoder.get_VAE_tile_size,
        "Decoder.forward": ae.Decoder.forward,
        "CausalConv3d.forward": ae.CausalConv3d.forward,
        "vae_decode": ltxmi.vae_decode,
        "vae_encode": ltxmi.vae_encode,
        "un_normalize_latents": ae.un_normalize_latents,
        "normalize_latents": ae.normalize_latents,
        "SymmetricPatchifier.patchify": SymmetricPatchifier.patchify,
        "SymmetricPatchifier.unpatchify": SymmetricPatchifier.unpatchify,
        "RectifiedFlowScheduler.__init__": ltxmi.RectifiedFlowScheduler.__init__,
        "RectifiedFlowScheduler.set_timesteps": ltxmi.RectifiedFlowScheduler.set_timesteps,
        "RectifiedFlowScheduler.step": ltxmi.RectifiedFlowScheduler.step,
        "RectifiedFlowScheduler.add_noise": ltxmi.RectifiedFlowScheduler.add_noise,
        "RectifiedFlowScheduler.scale_model_input": ltxmi.RectifiedFlowScheduler.scale_model_input,
        "LTXVideoPipeline.__init__": ltxmi.LTXVideoPipeline.__init__,
        "LTXVideoPipeline.__call__": ltxmi.LTXVideoPipeline.__call__,
        "LTXVideoPipeline.encode_prompt": ltxmi.LTXVideoPipeline.encode_prompt,
        "LTXVideoPipeline.check_inputs": ltxmi.LTXVideoPipeline.check_inputs,
        "LTXVideoPipeline.prepare_latents": ltxmi.LTXVideoPipeline.prepare_latents,
        "LTXVideoPipeline.prepare_conditioning": ltxmi.LTXVideoPipeline.prepare_conditioning,
        "LTXVideoPipeline.resize_tensor": ltxmi.LTXVideoPipeline.resize_tensor,
        "LTXMultiScalePipeline.__init__": ltxmi.LTXMultiScalePipeline.__init__,
        "LTXMultiScalePipeline.__call__": ltxmi.LTXMultiScalePipeline.__call__,
        "LTXMultiScalePipeline._upsample_latents": ltxmi.LTXMultiScalePipeline._upsample_latents,
        "retrieve_timesteps": pl.retrieve_timesteps,
        "adain_filter_latent": ltxmi.adain_filter_latent,
        "ConditioningItem": ltxmi.ConditioningItem,
        "LatentUpsampler.__init__": ltxmi.LatentUpsampler.__init__,
        "LatentUpsampler.forward": ltxmi.LatentUpsampler.forward,
    }


# where the product is deliberately MORE permissive than the reference (a default where the reference requires the
# argument); nothing else may differ
_LENIENT_DEFAULTS = {
    "LTXVideoPipeline.__init__": {"tokenizer", "text_encoder", "vae", "transformer", "scheduler", "patchifier",
                                  "prompt_enhancer_image_caption_model", "prompt_enhancer_image_caption_processor",
                                  "prompt_enhancer_llm_model", "prompt_enhancer_llm_tokenizer"},
}


def _compare_signature(name, ref, ours):
    problems = []
    variadic = ("VAR_POSITIONAL", "VAR_KEYWORD")
    ref_named = [p for p in ref if p["kind"] not in variadic]
    ours_named = [p for p in ours if p["kind"] not in variadic]
    for i, rp in enumerate(ref_named):
        if i >= len(ours_named):
            problems.append(f"missing parameter {rp['name']!r}")
            continue
        op = ours_named[i]
        if op["name"] != rp["name"]:
            problems.append(f"position {i}: {op['name']!r} where the reference has {rp['name']!r}")
            continue
        if op["kind"] != rp["kind"]:
            problems.append(f"{rp['name']}: kind {op['kind']} != {rp['kind']}")
        if rp["has_default"]:
            if not op["has_default"] or op["default"] != rp["default"]:
                problems.append(f"{rp['name']}: default {op['default']} != {rp['default']}")
        elif op["has_default"] and rp["name"] not in _LENIENT_DEFAULTS.get(name, ()):
            problems.append(f"{rp['name']}: has a default ({op['default']}) where the reference requires it")
    for op in ours_named[len(ref_named):]:                 # extras: optional, after everything the reference has
        if not op["has_default"]:
            problems.append(f"extra parameter {op['name']!r} without a default")
    for kind in variadic:
        if any(p["kind"] == kind for p in ref) and not any(p["kind"] == kind for p in ours):
            problems.append(f"the reference takes {kind} and the product does not")
    return problems


def test_entry_point_signatures_match_the_reference():
    """Every public entry point of SURVEY 8(b) has the reference's parameter names, order, kinds and defaults
    (tests/golden/signatures.json = inspect.signature of the reference's own objects, oracle/gen/make_golden.py
    ``signatures``); the product may only add optional parameters behind them."""
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "signatures.json")) as f:
        ref = json.load(f)
    ours = _product_entry_points()
    report = {}
    for name, fn in ours.items():
        problems = _compare_signature(name, ref[name], _sig(fn))
        if problems:
            report[name] = problems
    assert not report, "\n" + "\n".join(f"{k}: {v}" for k, v in report.items())
    # the Wan sequence-parallel entry points are NOT signature-compatible (they are bound methods of the Wan model, which
    # is out of scope): the names are reused for the LTX DiT, INTEGRATION.md says so -- keep that statement honest
    from ltxmi import distributed as sp
    assert [p["name"] for p in _sig(sp.usp_dit_forward)][:2] != [p["name"] for p in ref["wan.usp_dit_forward"]][:2]


# ------------------------------------------------------------------ the pipeline's prompt and conditioning glue (CPU)
# LTXVideoPipeline's host code is plain torch on small tensors: pinned here without the library, against the goldens the
# reference's own methods produced (G12, G15) and against the oracle where no golden exists.
def _prompt_pipeline(golden):
    from golden_cases import g15_case
    t, meta, _, _, _, tok, enc = g15_case(golden)
    return ltxmi.LTXVideoPipeline(tokenizer=tok, text_encoder=enc), t, meta["call"]


def test_g15_product_encode_prompt(golden):
    """encode_prompt called the way LTXMultiScalePipeline.__call__ calls it, against the tensors the reference's own
    encode_prompt produced under the same fake T5 (G15)."""
    pipe, t, call = _prompt_pipeline(golden)
    with torch.no_grad():
        got = pipe.encode_prompt(call["prompt"], True, negative_prompt=call["negative_prompt"], device="cpu",
                                 text_encoder_max_tokens=256)
    pos, pos_mask, neg, neg_mask = got
    assert pos.dtype == neg.dtype == pipe.text_encoder.dtype
    assert torch.equal(pos, t["prompt_embeds"]) and torch.equal(neg, t["negative_prompt_embeds"])
    assert torch.equal(pos_mask.float(), t["prompt_attention_mask"])
    assert torch.equal(neg_mask.float(), t["negative_prompt_attention_mask"])
    assert all(str(x.device) == "cpu" for x in got)


def test_encode_prompt_batches_repeats_and_refusals(golden):
    """Two prompts x two videos per prompt: rows come out prompt-major (p0, p0, p1, p1), the negative prompt is encoded once
    per prompt at the positive pair's token length, texts are stripped before tokenising (the mask sums are the byte counts
    + EOS of the STRIPPED texts).  The literals are what the parent commit returns."""
    pipe, _, _ = _prompt_pipeline(golden)
    with torch.no_grad():
        pos, pos_mask, neg, neg_mask = pipe.encode_prompt(["a cat ", "two dogs"], True, negative_prompt=" bad",
                                                          num_images_per_prompt=2, device="cpu", text_encoder_max_tokens=32)
    assert pos.shape == neg.shape == (4, 32, 128) and pos_mask.shape == neg_mask.shape == (4, 32)
    assert pos.dtype == neg.dtype == torch.float32 and pos_mask.dtype == neg_mask.dtype == torch.int64
    assert torch.equal(pos[0], pos[1]) and torch.equal(pos[2], pos[3]) and not torch.equal(pos[0], pos[2])
    assert all(torch.equal(neg[0], neg[i]) for i in (1, 2, 3))
    assert pos_mask.sum(1).tolist() == [6, 6, 9, 9] and neg_mask.sum(1).tolist() == [4, 4, 4, 4]
    with torch.no_grad():
        one = pipe.encode_prompt("two dogs", True, negative_prompt="bad", device="cpu", text_encoder_max_tokens=32)
        assert torch.equal(one[0][0], pos[2]) and torch.equal(one[1][0], pos_mask[2])
        assert torch.equal(one[2][0], neg[0]) and torch.equal(one[3][0], neg_mask[0])
        # no guidance: no negative pair, and the negative prompt is not encoded
        a, b, c, d = pipe.encode_prompt("two dogs", False, device="cpu", text_encoder_max_tokens=32)
    assert torch.equal(a, one[0]) and torch.equal(b, one[1]) and c is None and d is None

    # given embeddings, no T5: taken as they are, cast to the transformer's dtype (there is no text encoder), repeated per video
    bare = ltxmi.LTXVideoPipeline()
    a, b, c, d = bare.encode_prompt(None, True, num_images_per_prompt=2, device="cpu", prompt_embeds=pos[2:3],
                                    prompt_attention_mask=pos_mask[2:3], negative_prompt_embeds=neg[:1],
                                    negative_prompt_attention_mask=neg_mask[:1])
    assert torch.equal(a, pos[2:]) and torch.equal(b, pos_mask[2:]) and torch.equal(c, neg[:2]) and torch.equal(d, neg_mask[:2])
    import types
    bf16 = ltxmi.LTXVideoPipeline(transformer=types.SimpleNamespace(dtype=torch.bfloat16, device="cpu"))
    a, b, c, d = bf16.encode_prompt(None, False, prompt_embeds=pos[:1], prompt_attention_mask=pos_mask[:1])
    assert torch.equal(a, pos[:1].to(torch.bfloat16)) and torch.equal(b, pos_mask[:1]) and c is None and d is None

    with pytest.raises(RuntimeError):
        bare.encode_prompt("two dogs", False, device="cpu")
    with pytest.raises(RuntimeError):           # the positive pair is given, the negative prompt still needs the T5
        bare.encode_prompt(None, True, negative_prompt="bad", device="cpu", prompt_embeds=pos[:1],
                           prompt_attention_mask=pos_mask[:1])


def _check_inputs_rows():
    e, m = torch.zeros(1, 4, 8), torch.ones(1, 4)
    e2, m2 = torch.zeros(1, 5, 8), torch.ones(1, 5)
    ok = dict(prompt="p", height=64, width=96, negative_prompt=None)
    emb = dict(ok, prompt=None, prompt_embeds=e, prompt_attention_mask=m)
    both = dict(emb, negative_prompt_embeds=e, negative_prompt_attention_mask=m)
    return [
        # (arguments, exception or None, parameter names the message has to mention)
        (dict(ok, height=60), ValueError, ["height", "width"]),
        (dict(ok, width=100), ValueError, ["height", "width"]),
        (dict(ok, prompt_embeds=e, prompt_attention_mask=m), ValueError, ["prompt", "prompt_embeds"]),
        (dict(ok, prompt=None), ValueError, ["prompt", "prompt_embeds"]),
        (dict(ok, prompt=3), ValueError, ["prompt"]),
        (dict(ok, negative_prompt_embeds=e, negative_prompt_attention_mask=m), ValueError, ["prompt", "negative_prompt_embeds"]),
        (dict(both, negative_prompt="n"), ValueError, ["negative_prompt", "negative_prompt_embeds"]),
        (dict(emb, prompt_attention_mask=None), ValueError, ["prompt_attention_mask", "prompt_embeds"]),
        (dict(both, negative_prompt_attention_mask=None), ValueError,
         ["negative_prompt_attention_mask", "negative_prompt_embeds"]),
        (dict(both, negative_prompt_embeds=e2, negative_prompt_attention_mask=m2), ValueError,
         ["prompt_embeds", "negative_prompt_embeds"]),
        (dict(both, negative_prompt_attention_mask=m2), ValueError,
         ["prompt_attention_mask", "negative_prompt_attention_mask"]),
        (dict(ok, enhance_prompt=True), NotImplementedError, ["enhance_prompt"]),
        (dict(ok, negative_prompt="n"), None, []),
        (dict(both), None, []),
    ]


@pytest.mark.parametrize("kwargs,exc,names", _check_inputs_rows())
def test_check_inputs_refusals(kwargs, exc, names):
    """One row per refusal of check_inputs (ten ValueErrors, the first listed for height and for width; one
    NotImplementedError) and two accepted argument sets: the exception type, and that the message names what is wrong."""
    pipe = ltxmi.LTXVideoPipeline()
    if exc is None:
        assert pipe.check_inputs(**kwargs) is None
        return
    with pytest.raises(exc) as info:
        pipe.check_inputs(**kwargs)
    assert type(info.value) is exc
    for name in names:
        assert name in str(info.value), (name, str(info.value))


def test_g12_product_latent_spatial_position(golden):
    """_get_latent_spatial_position against G12: a 64x64 item at x = 32 of a 160x128 frame, vertically centred, touches no
    border, so one latent row / column goes on every side and the origin moves by one latent."""
    import types
    t, meta = golden("g12_conditioning")
    stub = types.SimpleNamespace(vae_scale_factor=32)
    item = ltxmi.ConditioningItem(torch.zeros(1, 3, 1, 64, 64), 0, 1.0, media_x=32, media_y=None)
    out, lx, ly = ltxmi.LTXVideoPipeline._get_latent_spatial_position(stub, t["place.in"], item, 128, 160, True)
    assert [lx, ly] == meta["place"] and torch.equal(out, t["place.out"])
    out, lx, ly = ltxmi.LTXVideoPipeline._get_latent_spatial_position(stub, t["place.in"], item, 128, 160, False)
    assert (lx, ly) == (1, 1) and torch.equal(out, t["place.in"])


@pytest.mark.parametrize("mode", ["concat", "soft", "drop", "bogus"])
@pytest.mark.parametrize("f_l,prefix", [(2, 2), (4, 2), (3, 1), (1, 1), (5, 3)])
def test_non_first_conditioning_sequence_matches_oracle(mode, f_l, prefix):
    """A frame sequence that does not start the video: its latent frames past the prefix are blended into the grid, the
    prefix is kept as extra tokens ("concat"), blended softly ("soft") or dropped.  Against the oracle's restatement; its
    "concat" path is pinned to the reference by G12 (test_g12_conditioning), "soft" and "drop" have no golden."""
    from oracle import conditioning as oc
    g = torch.Generator().manual_seed(100 * f_l + prefix)
    grid, lat = torch.randn(1, 8, 9, 2, 3, generator=g), torch.randn(1, 8, f_l, 2, 3, generator=g)
    mask = torch.rand(1, 9, 2, 3, generator=g)
    args = dict(num_prefix_latent_frames=prefix, prefix_latents_mode=mode, prefix_soft_conditioning_strength=0.15)
    ours = ltxmi.LTXVideoPipeline._handle_non_first_conditioning_sequence
    for strength in (0.9, 0.1):                 # 0.1: below the soft prefix strength, which is then capped by it
        if mode == "bogus":
            with pytest.raises(ValueError):
                ours(grid.clone(), mask.clone(), lat.clone(), 16, strength, **args)
            continue
        want = oc.handle_non_first_conditioning_sequence(grid.clone(), mask.clone(), lat.clone(), 16, strength, **args)
        mine_grid, mine_mask = grid.clone(), mask.clone()
        got = ours(mine_grid, mine_mask, lat.clone(), 16, strength, **args)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(mine_grid, want[0]) and torch.equal(mine_mask, want[1])          # written in place
        assert (got[2] is None and want[2] is None) or torch.equal(got[2], want[2])
        assert (got[2] is None) == (mode != "concat")
        assert torch.equal(mine_grid, grid) == (f_l == prefix and (mode != "soft" or prefix == 1))     # something was written


class _TorchWithRecordedDraws:
    """``torch`` as ltxmi.pipeline sees it, with ``randn`` handing out recorded draws in order."""

    def __init__(self, draws):
        self.draws, self.used = draws, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def randn(self, shape, **kwargs):
        draw = self.draws[self.used]
        assert tuple(shape) == tuple(draw.shape), (self.used, tuple(shape), tuple(draw.shape))
        self.used += 1
        return draw.clone()


def test_g12_product_prepare_conditioning(golden, monkeypatch):
    """prepare_conditioning end to end on the CPU against what the reference's own method returned (G12): a first-frame
    image, a 17-frame sequence at frame 8 (its two prefix latent frames become extra tokens) and a single frame at 24.
    The encoder is the oracle's on G11-b's weights (pinned to the reference by G11), the noise is the recorded draws."""
    import types
    from golden_cases import sub
    from ltxmi import pipeline as pl
    from oracle import vae_encoder as ve
    t, meta = golden("g12_conditioning")
    tb, _ = golden("g11_encoder_b")
    cfg, sd = meta["cfg"], sub(tb, "sd.")
    assert torch.equal(sd["encoder.conv_out.conv.weight"], t["weights_check"])
    sd["per_channel_statistics.std-of-means"] = t["per_channel_statistics.std-of-means"]
    sd["per_channel_statistics.mean-of-means"] = t["per_channel_statistics.mean-of-means"]
    vae = types.SimpleNamespace(dtype=torch.float32, device=torch.device("cpu"))
    pipe = ltxmi.LTXVideoPipeline(
        vae=vae, transformer=types.SimpleNamespace(config=types.SimpleNamespace(causal_temporal_positioning=True)))
    encoded = []

    def encode(media, the_vae, **kwargs):
        assert the_vae is vae and kwargs["vae_per_channel_normalize"] is True
        encoded.append(tuple(media.shape))
        return ve.vae_encode(sd, cfg, media)

    fake_torch = _TorchWithRecordedDraws([t[f"noise.{i}"] for i in range(meta["n_prepare_draws"])])
    monkeypatch.setattr(pl, "vae_encode", encode)
    monkeypatch.setattr(pl, "torch", fake_torch)
    items = [ltxmi.ConditioningItem(t["img"], 0, 1.0), ltxmi.ConditioningItem(t["seq"], 8, 0.9),
             ltxmi.ConditioningItem(t["single"], 24, 0.7)]
    lat, pc, mask, n_extra = pipe.prepare_conditioning(items, t["init_latents"].clone(), meta["F"], meta["H"], meta["W"],
                                                       vae_per_channel_normalize=True)
    assert n_extra == meta["n_extra"] and fake_torch.used == meta["n_prepare_draws"]
    assert encoded == [tuple(t[k].shape) for k in ("img", "seq", "single")]
    torch.testing.assert_close(lat, t["latents"], rtol=1e-4, atol=1e-5)
    assert torch.equal(pc, t["pixel_coords"]) and torch.equal(mask, t["mask"])
    lat0, pc0, mask0, n0 = pipe.prepare_conditioning(None, t["init_latents"].clone(), meta["F"], meta["H"], meta["W"])
    assert mask0 is None and n0 == 0 and fake_torch.used == meta["n_prepare_draws"]
    assert torch.equal(lat0, t["plain.latents"]) and torch.equal(pc0, t["plain.pixel_coords"])
