"""Several videos per ``LTXVideoPipeline.__call__``: the host logic on the CPU.

The step kernels are the CPU doubles of tests/cpu_ops_double.py and tests/cpu_ops_double_batched.py; the transformer is a
stub whose output for a row is an elementwise function of that row's inputs alone (its latents, the mean of its prompt row
over the valid tokens, its timestep, the number of blocks its skip-mask column switches off), so exact equality between
video j of a batched call and the single call made with video j's inputs is meaningful here.  The stub records what it is
called with: the row order, the skip-layer masks, ``stg_alias_rows``."""
import types

import pytest
import torch

import cpu_ops_double_batched
import ltxmi
from ltxmi import pipeline as pl
from ltxmi.autoencoder import randn_rows

BF = torch.bfloat16
C, LAYERS, T, DC = 8, 4, 6, 16
H, W, FRAMES = 64, 96, 17
GRID = (3, 2, 3)
N = GRID[0] * GRID[1] * GRID[2]


class StubTransformer:
    """Rows are independent: out[r] = 0.5 x[r] + 0.25 mean(prompt[r]) + 0.125 timestep[r] - 0.3 (blocks skipped for row r)."""
    dtype, device = BF, torch.device("cpu")

    def __init__(self):
        self.config = types.SimpleNamespace(in_channels=C, causal_temporal_positioning=True)
        self.transformer_blocks = [None] * LAYERS
        self.calls = []

    def precompute_freqs_cis(self, frac):
        self.frac = frac
        return (frac, frac)

    create_skip_layer_mask = ltxmi.Transformer3DModel.create_skip_layer_mask

    def __call__(self, x, freqs_cis=None, encoder_hidden_states=None, encoder_attention_mask=None, timestep=None,
                 stg_alias_blocks=0, stg_alias_rows=1, skip_layer_mask=None, **kw):
        rows = x.shape[0]
        assert encoder_hidden_states.shape[0] == encoder_attention_mask.shape[0] == timestep.shape[0] == rows
        assert freqs_cis[0].shape[0] == 1                               # one table for all rows
        m = encoder_attention_mask.float()
        prompt = (encoder_hidden_states.float() * m.unsqueeze(-1)).sum((1, 2)) / (m.sum(1) * DC)
        skipped = torch.zeros(rows) if skip_layer_mask is None else (1 - skip_layer_mask.float()).sum(0)
        self.calls.append(dict(rows=rows, embeds=encoder_hidden_states.clone(), mask=encoder_attention_mask.clone(),
                               timestep=timestep.clone(), x=x.clone(), alias_blocks=stg_alias_blocks, alias_rows=stg_alias_rows,
                               skip=None if skip_layer_mask is None else skip_layer_mask.float().clone(),
                               joint_pass=kw.get("joint_pass")))
        out = (0.5 * x.float() + 0.25 * prompt.view(rows, 1, 1) + 0.125 * timestep.float().reshape(rows, -1, 1)
               - 0.3 * skipped.view(rows, 1, 1))
        return (out.to(BF),)


def fake_vae_encode(media, vae, split_size=1, vae_per_channel_normalize=False, generator=None, sample_posterior=True,
                    num_samples=None):
    """(m, 3, f, H, W) -> (m or num_samples, C, f_l, H / 32, W / 32): pooled pixels times a channel ramp, plus a posterior
    draw through the product's ``randn_rows`` (a generator list: one draw per video)."""
    m, _, f, h, w = media.shape
    pooled = torch.nn.functional.adaptive_avg_pool3d(media.float(), ((f - 1) // 8 + 1, h // 32, w // 32)).mean(1, keepdim=True)
    lat = pooled * torch.linspace(0.5, 2.0, C).view(1, C, 1, 1, 1)
    if num_samples is not None and lat.shape[0] == 1:
        lat = lat.expand(num_samples, *lat.shape[1:])
    if sample_posterior:
        lat = lat + 0.1 * randn_rows(lat.shape, generator, lat.device, torch.float32)
    return lat


@pytest.fixture
def pipe(monkeypatch):
    cpu_ops_double_batched.install(monkeypatch)
    monkeypatch.setattr(pl, "vae_encode", fake_vae_encode)
    return ltxmi.LTXVideoPipeline(transformer=StubTransformer(), vae=types.SimpleNamespace(dtype=torch.float32, device="cpu"),
                                  scheduler=ltxmi.RectifiedFlowScheduler(shifting="SD3", target_shift_terminal=0.1))


def prompts(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    pos, neg = torch.randn(n, T, DC, generator=g).to(BF), torch.randn(n, T, DC, generator=g).to(BF)
    pmask, nmask = torch.ones(n, T), torch.ones(n, T)
    for j in range(n):
        pmask[j, 3 + j % 3:] = 0
        nmask[j, 2 + j % 2:] = 0
    return dict(prompt_embeds=pos, prompt_attention_mask=pmask, negative_prompt_embeds=neg, negative_prompt_attention_mask=nmask)


def rows_of(p, rows):
    return {k: v[rows] for k, v in p.items()}


def gens(seeds):
    return [torch.Generator().manual_seed(s) for s in seeds]


BASE = dict(height=H, width=W, num_frames=FRAMES, frame_rate=25.0, output_type="latent", is_video=True, joint_pass=True,
            latents_dtype=torch.float32, skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues)
DISTILLED = dict(num_inference_steps=3, guidance_scale=1.0, stg_scale=0.0, rescaling_scale=1.0)
GUIDED = dict(num_inference_steps=3, guidance_scale=3.0, stg_scale=1.0, rescaling_scale=0.7, skip_block_list=[1, 2])
# step 0: no guidance at all; steps 1, 2: CFG + STG + rescale -- dead-row elimination changes the chunk count between steps
TABLES = dict(num_inference_steps=3, guidance_scale=[1, 3], stg_scale=[0, 1], rescaling_scale=[1, 0.7],
              skip_block_list=[[], [2]], guidance_timesteps=[1.0, 0.95])


def run(pipe, **kw):
    pipe.transformer.calls = []
    out = pipe(**{**BASE, **kw})
    return out, pipe.transformer.calls


def assert_videos_equal_single_calls(pipe, per_video_prompts, seeds, settings, per_video=None, **shared):
    """The batched call (generator list) against one call per video (its prompt rows, its generator, ``per_video[j]``)."""
    b = len(seeds)
    batched, calls = run(pipe, **per_video_prompts, generator=gens(seeds), **settings, **shared,
                         **({} if per_video is None else per_video["batched"]))
    assert batched.shape == (b, C, *GRID)
    for j in range(b):
        extra = {} if per_video is None else per_video["single"][j]
        single, _ = run(pipe, **rows_of(per_video_prompts, slice(j, j + 1)), generator=gens(seeds[j:j + 1])[0], **settings,
                        **shared, **extra)
        assert single.shape == (1, C, *GRID)
        assert torch.equal(batched[j:j + 1], single), f"video {j} differs from its single call"
    assert all(not torch.equal(batched[0], batched[j]) for j in range(1, b))
    return batched, calls


def test_two_prompts(pipe):
    p = prompts(2)
    _, calls = assert_videos_equal_single_calls(pipe, p, [11, 12], DISTILLED)
    assert [c["rows"] for c in calls] == [2, 2, 2]                      # B_eff = b: no guidance rows
    assert all(torch.equal(c["embeds"], p["prompt_embeds"]) and c["skip"] is None for c in calls)


def test_num_images_per_prompt_repeats_the_prompt_rows(pipe):
    p1, p2 = prompts(1), prompts(2)
    batched, calls = run(pipe, **p1, num_images_per_prompt=2, generator=gens([21, 22]), **DISTILLED)
    assert batched.shape == (2, C, *GRID) and calls[0]["rows"] == 2
    assert torch.equal(calls[0]["embeds"], p1["prompt_embeds"].repeat_interleave(2, 0))
    for j, seed in enumerate([21, 22]):
        single, _ = run(pipe, **p1, generator=gens([seed])[0], **DISTILLED)
        assert torch.equal(batched[j:j + 1], single)
    # two prompts x two images: prompt-major (p0, p0, p1, p1), as encode_prompt repeats text
    batched, calls = run(pipe, **p2, num_images_per_prompt=2, generator=gens([31, 32, 33, 34]), **GUIDED)
    assert batched.shape == (4, C, *GRID) and calls[0]["rows"] == 12
    order = [0, 0, 1, 1]
    want = torch.cat([p2["negative_prompt_embeds"][order], p2["prompt_embeds"][order], p2["prompt_embeds"][order]])
    assert torch.equal(calls[0]["embeds"], want)
    for j, seed in enumerate([31, 32, 33, 34]):
        single, _ = run(pipe, **rows_of(p2, slice(order[j], order[j] + 1)), generator=gens([seed])[0], **GUIDED)
        assert torch.equal(batched[j:j + 1], single), j
    with pytest.raises(ValueError, match="num_images_per_prompt"):
        run(pipe, **p1, num_images_per_prompt=0, **DISTILLED)


@pytest.mark.parametrize("b", [2, 3])
def test_guidance_tables_row_order_masks_and_alias_rows(pipe, b):
    p = prompts(b)
    _, calls = assert_videos_equal_single_calls(pipe, p, list(range(40, 40 + b)), TABLES)
    assert [c["rows"] for c in calls] == [b, 3 * b, 3 * b]              # dead rows are not computed at step 0
    neg, pos = p["negative_prompt_embeds"], p["prompt_embeds"]
    assert torch.equal(calls[0]["embeds"], pos) and calls[0]["skip"] is None and calls[0]["alias_blocks"] == 0
    for c in calls[1:]:
        assert torch.equal(c["embeds"], torch.cat([neg, pos, pos]))     # [neg x b, pos x b, ptb x b]
        assert torch.equal(c["mask"], torch.cat([p["negative_prompt_attention_mask"], p["prompt_attention_mask"],
                                                 p["prompt_attention_mask"]]))
        want = torch.ones(LAYERS, 3 * b)
        want[2, 2 * b:] = 0                                             # zeros on exactly the last b rows, at block 2 only
        assert torch.equal(c["skip"], want)
        assert c["alias_rows"] == b and c["alias_blocks"] == 2
        assert torch.equal(c["x"][:b], c["x"][b:2 * b]) and torch.equal(c["x"][:b], c["x"][2 * b:])
    # without the eliminations: all three chunks at every step, the mask on the last b rows, no aliasing -- the same bits
    on, _ = run(pipe, **p, generator=gens(range(40, 40 + b)), **TABLES)
    off, calls = run(pipe, **p, generator=gens(range(40, 40 + b)), **TABLES, dead_row_elimination=False, stg_row_dedup=False)
    assert [c["rows"] for c in calls] == [3 * b] * 3 and all(c["alias_blocks"] == 0 for c in calls)
    assert calls[0]["skip"] is None and torch.equal(calls[1]["skip"][2], torch.tensor([1.0] * 2 * b + [0.0] * b))
    assert torch.equal(on, off)


def test_one_video_takes_the_path_it_always_took(pipe):
    """b = 1: ``ops.guidance_step_`` (not the batched entry), the reference's skip-layer mask, no ``stg_alias_rows`` passed."""
    from ltxmi import ops
    used = []
    single_step = ops.guidance_step_
    ops.guidance_step_ = lambda *a, **k: (used.append("single"), single_step(*a, **k))[1]       # (the fixture restores it)
    batched_step = ops.guidance_step_batched_
    ops.guidance_step_batched_ = lambda *a, **k: (used.append("batched"), batched_step(*a, **k))[1]
    _, calls = run(pipe, **prompts(1), generator=gens([5])[0], **GUIDED)
    assert used == ["single"] * 3 and all(c["alias_rows"] == 1 and c["rows"] == 3 for c in calls)
    assert torch.equal(calls[0]["skip"], pipe.transformer.create_skip_layer_mask(1, 3, 2, [1, 2]).float())
    del used[:]
    run(pipe, **prompts(2), generator=gens([5, 6]), **GUIDED)
    assert used == ["batched"] * 3


@pytest.mark.parametrize("media_batch", ["shared", "per video"])
def test_conditioning_item_at_frame_0(pipe, media_batch):
    """An image at frame 0 (hard-conditioned first latent frame), image_cond_noise_scale > 0: the posterior draw, the initial
    noise and the per-step draw all come from video j's generator; cond_mask is [b, N] and the per-token timestep is
    min(t, 1 - mask), chunk-wise."""
    b = 2
    g = torch.Generator().manual_seed(60)
    media = torch.rand(b, 3, 1, H, W, generator=g) * 2 - 1
    if media_batch == "shared":
        per_video = dict(batched=dict(conditioning_items=[ltxmi.ConditioningItem(media[:1], 0, 1.0)]),
                         single=[dict(conditioning_items=[ltxmi.ConditioningItem(media[:1], 0, 1.0)])] * b)
    else:
        per_video = dict(batched=dict(conditioning_items=[ltxmi.ConditioningItem(media, 0, 1.0)]),
                         single=[dict(conditioning_items=[ltxmi.ConditioningItem(media[j:j + 1], 0, 1.0)]) for j in range(b)])
    _, calls = assert_videos_equal_single_calls(pipe, prompts(b), [61, 62], GUIDED, per_video, image_cond_noise_scale=0.15)
    hw = GRID[1] * GRID[2]
    for c in calls:
        ts = c["timestep"]
        assert ts.shape == (3 * b, N) and bool((ts[:, :hw] == 0).all()) and bool((ts[:, hw:] > 0).all())
        assert torch.equal(ts[:b], ts[b:2 * b]) and torch.equal(ts[:b], ts[2 * b:])
    first = calls[0]["x"]                                                # the conditioned frame differs per video (posterior draw)
    assert not torch.equal(first[0, :hw], first[1, :hw])
    with pytest.raises(ValueError, match="one per video, or one shared"):
        run(pipe, **prompts(3), **GUIDED, conditioning_items=[ltxmi.ConditioningItem(media, 0, 1.0)])


def test_item_with_extra_tokens_and_the_callback(pipe):
    """A single frame at pixel frame 8 becomes h w extra tokens in front, drawn per video; the callback gets video 0."""
    b = 2
    g = torch.Generator().manual_seed(70)
    frame = torch.rand(1, 3, 1, H, W, generator=g) * 2 - 1
    item = [ltxmi.ConditioningItem(frame, 8, 0.8)]
    seen = {"batched": [], "single": []}

    def callback_into(key):
        def callback(step, preview, start, **kw):
            if preview is not None:
                seen[key].append(preview.clone())
        return callback

    per_video = dict(batched=dict(callback=callback_into("batched")),
                     single=[dict(callback=callback_into("single")), {}])
    _, calls = assert_videos_equal_single_calls(pipe, prompts(b), [71, 72], GUIDED, per_video, conditioning_items=item)
    hw = GRID[1] * GRID[2]
    assert calls[0]["x"].shape == (3 * b, hw + N, C) and pipe.transformer.frac.shape == (1, 3, hw + N)
    assert not torch.equal(calls[0]["x"][0, :hw], calls[0]["x"][1, :hw])          # the extra tokens' noise is per video
    assert len(seen["batched"]) == len(seen["single"]) == 3
    for got, want in zip(seen["batched"], seen["single"]):
        assert got.shape == (C, *GRID) and torch.equal(got, want)


def test_given_latents_3d_and_5d_and_media_items(pipe):
    b = 2
    g = torch.Generator().manual_seed(80)
    tokens = torch.randn(b, N, C, generator=g)
    grid5 = torch.randn(b, C, *GRID, generator=g)
    p = prompts(b)
    out3, _ = run(pipe, **p, latents=tokens, **GUIDED)
    for j in range(b):
        assert torch.equal(out3[j:j + 1], run(pipe, **rows_of(p, slice(j, j + 1)), latents=tokens[j:j + 1], **GUIDED)[0])
    kw = dict(strength=0.9, **GUIDED)
    out5, _ = run(pipe, **p, latents=grid5, generator=gens([81, 82]), **kw)
    for j in range(b):
        single, _ = run(pipe, **rows_of(p, slice(j, j + 1)), latents=grid5[j:j + 1], generator=gens([81 + j])[0], **kw)
        assert torch.equal(out5[j:j + 1], single)
    with pytest.raises(AssertionError):
        run(pipe, **p, latents=tokens[:1], **GUIDED)
    # media_items shared by both videos: encoded once; its posterior is sampled from the global RNG (as the reference's
    # latent_dist.sample() is), so that RNG is set alike in front of every call
    video = torch.rand(1, 3, FRAMES, H, W, generator=g) * 2 - 1
    torch.manual_seed(85)
    outm, _ = run(pipe, **p, media_items=video, generator=gens([83, 84]), **kw)
    for j in range(b):
        torch.manual_seed(85)
        single, _ = run(pipe, **rows_of(p, slice(j, j + 1)), media_items=video, generator=gens([83 + j])[0], **kw)
        assert torch.equal(outm[j:j + 1], single)


def test_one_generator_draws_the_whole_batch_and_a_wrong_list_is_refused(pipe):
    p = prompts(2)
    a, _ = run(pipe, **p, generator=gens([90])[0], **DISTILLED)
    b_, _ = run(pipe, **p, generator=gens([90])[0], **DISTILLED)
    assert torch.equal(a, b_) and not torch.equal(a[0], a[1])
    for wrong in ([90], [90, 91, 92]):
        with pytest.raises(ValueError, match="generators for a batch of 2"):
            run(pipe, **p, generator=gens(wrong), **DISTILLED)
    one, _ = run(pipe, **prompts(1), generator=gens([90]), **DISTILLED)   # a list of one generator for one video
    assert torch.equal(one, run(pipe, **prompts(1), generator=gens([90])[0], **DISTILLED)[0])


def test_stochastic_sampling_steps_the_batch(pipe):
    torch.manual_seed(0)
    out, _ = run(pipe, **prompts(2), generator=gens([95, 96]), stochastic_sampling=True, **GUIDED)
    assert out.shape == (2, C, *GRID) and bool(torch.isfinite(out).all())


def test_sequence_parallelism_refuses_several_videos(pipe):
    pipe.transformer._sp_interrupt = types.SimpleNamespace(reset=lambda: None)
    with pytest.raises(NotImplementedError, match=r"2 videos.*sequence parallelism"):
        run(pipe, **prompts(2), **DISTILLED)
    out, _ = run(pipe, **prompts(1), generator=gens([1])[0], **DISTILLED)           # one video still runs
    assert out.shape == (1, C, *GRID)


def test_multiscale_encodes_a_prompt_list_once_per_image():
    """``LTXMultiScalePipeline.__call__``: a list ``prompt`` and ``num_images_per_prompt`` give prompts x images rows out of
    ``encode_prompt`` (prompt-major), and the passes are told one image per row: nothing is repeated twice."""
    from fake_t5 import FakeTextEncoder, FakeTokenizer
    enc = FakeTextEncoder(DC)
    vp = ltxmi.LTXVideoPipeline(tokenizer=FakeTokenizer(), text_encoder=enc,
                                transformer=types.SimpleNamespace(dtype=torch.float32, device="cpu"),
                                vae=types.SimpleNamespace())
    ms = ltxmi.LTXMultiScalePipeline(vp, None)
    seen = []
    ms._run_pass = lambda number, args, shared, overrides, **fixed: seen.append(shared)
    assert ms(0.5, {}, {}, prompt=["a red fox", "two dogs"], negative_prompt="blurry", num_images_per_prompt=2,
              output_type="latent", height=H, width=W, device="cpu") is None
    shared = seen[0]
    assert shared["num_images_per_prompt"] == 1 and "prompt" not in shared
    assert shared["prompt_embeds"].shape == shared["negative_prompt_embeds"].shape == (4, 256, DC)
    single = vp.encode_prompt(["a red fox", "two dogs"], True, negative_prompt="blurry", device="cpu")
    assert torch.equal(shared["prompt_embeds"], single[0].repeat_interleave(2, 0))
    assert torch.equal(shared["prompt_attention_mask"], single[1].repeat_interleave(2, 0))
    # embeddings handed in directly are left alone: the video pipeline repeats them itself
    del seen[:]
    ms(0.5, {}, {}, prompt_embeds=single[0], num_images_per_prompt=2, output_type="latent", height=H, width=W)
    assert seen[0]["num_images_per_prompt"] == 2 and seen[0]["prompt_embeds"].shape[0] == 2
