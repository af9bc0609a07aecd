"""Several videos per pipeline call on the MI355X: video j of a batched call must equal, bit for bit, the single call made
with video j's inputs (its prompt rows, its generator) -- the property ``dead_row_elimination`` and ``stg_row_dedup`` already
rest on: every kernel computes a batch row independently of the others, and the GEMMs accumulate over K in one order whatever
M picks.  Only the attention kernel id can differ with the row count, so every case first asserts that
``ops.attention_kernel_id`` is the same at every row count that occurs, for self- and cross-attention."""
import types

import pytest
import torch

from test_gpu_model import BF, DEV, build_model, build_vae, vae_case

pytestmark = pytest.mark.gpu

HEADS, DH, LAYERS, CAPTION, T = 2, 64, 3, 128, 32
H, W, FRAMES = 64, 96, 17
GRID = (3, 2, 3)
N = GRID[0] * GRID[1] * GRID[2]
SCHED = dict(shifting="SD3", target_shift_terminal=0.1)
# step 0 without guidance, then CFG + STG + rescale with block 1 skipped: B_eff goes b -> 3 b, block 0 is aliased (stg_row_dedup)
TABLES = dict(num_inference_steps=3, guidance_scale=[1, 3], stg_scale=[0, 1], rescaling_scale=[1, 0.7],
              skip_block_list=[[], [1]], guidance_timesteps=[1.0, 0.95])
DISTILLED = dict(num_inference_steps=3, guidance_scale=1.0, stg_scale=0.0, rescaling_scale=1.0)


@pytest.fixture(scope="module")
def model():
    from oracle import dit
    cfg = dict(dit.default_2b_config(), num_attention_heads=HEADS, attention_head_dim=DH, num_layers=LAYERS,
               cross_attention_dim=HEADS * DH, caption_channels=CAPTION, causal_temporal_positioning=True)
    return build_model(cfg, {k: v.to(BF).float() for k, v in dit.init_state_dict(cfg, seed=7).items()})


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(8)
    pos, neg = torch.randn(3, T, CAPTION, generator=g).to(BF), torch.randn(3, T, CAPTION, generator=g).to(BF)
    pmask, nmask = torch.ones(3, T), torch.ones(3, T)
    for j in range(3):
        pmask[j, 20 - 3 * j:] = 0
        nmask[j, 5 + j:] = 0
    return dict(prompt_embeds=pos.to(DEV), prompt_attention_mask=pmask.to(DEV), negative_prompt_embeds=neg.to(DEV),
                negative_prompt_attention_mask=nmask.to(DEV))


def assert_one_attention_kernel(tokens, b):
    """Self- and cross-attention are served by one kernel at every row count a call of b videos and its single calls use:
    1 .. 3 chunks of 1 or b rows, and the sub-batches stg_row_dedup runs (one chunk less)."""
    from ltxmi import ops
    rows = sorted({c * v for c in (1, 2, 3) for v in (1, b)})
    ids = {(ops.attention_kernel_id(r, HEADS, tokens, tokens, DH), ops.attention_kernel_id(r, HEADS, tokens, T, DH, True))
           for r in rows}
    assert len(ids) == 1, (tokens, rows, ids)


def pipeline(model, vae=None):
    import ltxmi
    return ltxmi.LTXVideoPipeline(transformer=model, scheduler=ltxmi.RectifiedFlowScheduler(**SCHED), vae=vae)


def gens(seeds):
    return [torch.Generator(device=DEV).manual_seed(s) for s in seeds]


def call(pipe, prompts, rows, generator, **kw):
    import ltxmi
    base = dict(height=H, width=W, num_frames=FRAMES, frame_rate=25.0, output_type="latent", is_video=True, joint_pass=True,
                skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues, latents_dtype=torch.float32)
    return pipe(**{**base, **{k: v[rows] for k, v in prompts.items()}, "generator": generator, **kw})


def assert_videos_equal_single_calls(pipe, prompts, b, seeds, run=call, **kw):
    batched = run(pipe, prompts, slice(0, b), gens(seeds), **kw)
    assert batched.shape[0] == b and bool(torch.isfinite(batched.float()).all())
    for j in range(b):
        single = run(pipe, prompts, slice(j, j + 1), gens(seeds[j:j + 1])[0], **kw)
        assert torch.equal(batched[j:j + 1], single), f"video {j} of {b} differs from its single call"
    assert not torch.equal(batched[0], batched[1])
    return batched


@pytest.mark.parametrize("b", [2, 3])
def test_distilled_settings(model, prompts, b):
    """Guidance 1, STG 0: B_eff = b, the rows that fill the chip are the other videos of the call."""
    assert_one_attention_kernel(N, b)
    out = assert_videos_equal_single_calls(pipeline(model), prompts, b, [11, 12, 13][:b], **DISTILLED)
    assert out.shape == (b, 128, *GRID)


@pytest.mark.parametrize("b", [2, 3])
@pytest.mark.parametrize("dedup,dead", [(True, True), (True, False), (False, True), (False, False)])
def test_cfg_stg_with_and_without_the_row_eliminations(model, prompts, b, dedup, dead):
    assert_one_attention_kernel(N, b)
    kw = dict(TABLES, stg_row_dedup=dedup, dead_row_elimination=dead)
    out = assert_videos_equal_single_calls(pipeline(model), prompts, b, [21, 22, 23][:b], **kw)
    if not (dedup and dead):                            # the eliminations themselves change no bit at b videos either
        plain = call(pipeline(model), prompts, slice(0, b), gens([21, 22, 23][:b]), **TABLES)
        assert torch.equal(out, plain)


def test_a_batch_of_identical_videos_is_the_single_video(model, prompts):
    """num_images_per_prompt = 2 with the same noise for both images: both rows are the one-video result."""
    assert_one_attention_kernel(N, 2)
    noise = torch.randn(1, N, 128, generator=torch.Generator().manual_seed(30)).to(DEV)
    pipe = pipeline(model)
    single = call(pipe, prompts, slice(0, 1), None, latents=noise, **TABLES)
    both = call(pipe, prompts, slice(0, 1), None, latents=noise.repeat(2, 1, 1), num_images_per_prompt=2, **TABLES)
    assert both.shape[0] == 2 and torch.equal(both[:1], single) and torch.equal(both[1:], single)


def test_image_to_video_with_conditioning_noise_and_a_generator_list(model, prompts):
    """A first-frame image shared by both videos (encoded once) and a later single frame (extra tokens): the posterior
    draws, the extra tokens' noise, the initial noise and the per-step image_cond_noise draws all come from video j's
    generator; the masked step and the per-token timesteps run per video."""
    import ltxmi
    b = 2
    assert_one_attention_kernel(N + GRID[1] * GRID[2], b)
    vcfg, vsd = vae_case("b", with_encoder=True)
    pipe = pipeline(model, build_vae(vcfg, vsd))
    g = torch.Generator().manual_seed(40)
    img, later = [(torch.rand(1, 3, 1, H, W, generator=g) * 2 - 1).to(BF).to(DEV) for _ in range(2)]
    items = [ltxmi.ConditioningItem(img, 0, 1.0), ltxmi.ConditioningItem(later, 8, 0.8)]
    kw = dict(num_inference_steps=3, guidance_scale=3.0, stg_scale=1.0, rescaling_scale=0.7, skip_block_list=[1],
              conditioning_items=items, image_cond_noise_scale=0.15)
    out = assert_videos_equal_single_calls(pipe, prompts, b, [41, 42], **kw)
    assert out.shape == (b, 128, *GRID)
    assert not torch.equal(out[0, :, 0], out[1, :, 0])          # the hard-conditioned frame: same image, other posterior draw


def test_mixed_precision(model, prompts):
    assert_one_attention_kernel(N, 2)
    out = assert_videos_equal_single_calls(pipeline(model), prompts, 2, [51, 52], mixed_precision=True,
                                           **{**TABLES, "latents_dtype": None})
    assert out.dtype == torch.float32


def test_multiscale_two_passes(model, prompts):
    """LTXMultiScalePipeline at b = 2 with a generator list: pass 1, the latent upsampler, AdaIN (planes = b c), the
    re-noising and pass 2 (joint_pass=False) all per video."""
    import ltxmi
    from oracle import upsampler as ou
    b = 2
    assert_one_attention_kernel(GRID[0] * 2 * 3, b)                  # pass 1: 64 x 96 px, latent 2 x 3
    assert_one_attention_kernel(GRID[0] * 4 * 6, b)                  # pass 2: twice that
    ucfg = dict(in_channels=128, mid_channels=64, num_blocks_per_stage=1, dims=3, spatial_upsample=True, temporal_upsample=False)
    ups = ltxmi.LatentUpsampler.from_config(ucfg)
    ups.load_state_dict({k: v.to(BF).float() for k, v in ou.init_state_dict(ucfg, seed=6).items()})
    ups = ups.to(device=DEV, dtype=BF).eval()
    g = torch.Generator().manual_seed(60)
    vae = types.SimpleNamespace(std_of_means=(0.5 + torch.rand(128, generator=g)).to(DEV),
                                mean_of_means=(0.2 * torch.randn(128, generator=g)).to(DEV))
    ms = ltxmi.LTXMultiScalePipeline(pipeline(model, vae), ups)
    first = dict(TABLES)
    second = dict(num_inference_steps=4, skip_initial_inference_steps=2, guidance_scale=1, stg_scale=0, rescaling_scale=1,
                  skip_block_list=None, guidance_timesteps=None)

    def run(_, prompts, rows, generator, **kw):
        return ms(0.5, first, second, height=128, width=192, num_frames=FRAMES, frame_rate=25.0, output_type="latent",
                  is_video=True, skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues, latents_dtype=torch.float32,
                  generator=generator, **{k: v[rows] for k, v in prompts.items()})

    out = assert_videos_equal_single_calls(None, prompts, b, [61, 62], run=run)
    assert out.shape == (b, 128, GRID[0], 4, 6)


def test_decode_to_pixels(model, prompts, monkeypatch):
    """output_type="pt" at b = 2 through a small VAE without timestep conditioning.  The decoder's convolutions are asked for
    their route (``ops.conv3d_route``, host arithmetic) at batch 1 and batch 2: the same for every one of them at this latent
    size, so the decoded videos must have the single calls' bits too."""
    from ltxmi import ops
    b = 2
    assert_one_attention_kernel(N, b)
    vcfg, vsd = vae_case("a")
    assert not vcfg.get("timestep_conditioning")
    pipe = pipeline(model, build_vae(vcfg, vsd))
    routes, conv3d = [], ops.conv3d

    def recording(*a, **kw):
        routes.append(ops.conv3d_route(*a, **kw))
        return conv3d(*a, **kw)

    monkeypatch.setattr(ops, "conv3d", recording)
    batched = call(pipe, prompts, slice(0, b), gens([71, 72]), output_type="pt", **DISTILLED)
    batched_routes = list(routes)
    assert batched.shape == (b, 3, FRAMES, H, W) and float(batched.min()) >= 0 and float(batched.max()) <= 1
    assert len(batched_routes) >= 10 and all(isinstance(r, dict) for r in batched_routes)
    for j in range(b):
        del routes[:]
        single = call(pipe, prompts, slice(j, j + 1), gens([71 + j])[0], output_type="pt", **DISTILLED)
        assert routes == batched_routes, "a decoder convolution takes another route at batch 2 than at batch 1"
        assert torch.equal(batched[j:j + 1], single), f"decoded video {j} differs from its single call"
