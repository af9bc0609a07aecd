"""ltxmi_guidance_step_batched_bf16 on the MI355X: video j of a batched step against the one-sample step on its slices
(bit for bit) and against the float64 truth of tests/batched_step_cases.py (the bound tests/pointwise_cases.py derives)."""
import pytest
import torch

import batched_step_cases as bc
import pointwise_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run_batched(setting, b, tokens, lat_dtype, masked, npred=None):
    """The batched step on a NaN-filled workspace; returns the latents [b, tokens, C] after it."""
    from ltxmi import ops
    np_host, lat, mask = bc.inputs(setting, b, tokens)
    npred = (np_host if npred is None else npred).to(DEV)
    lat = lat.to(lat_dtype).to(DEV).clone()
    workspace = torch.full((b * ops.GUIDANCE_WORKSPACE_FLOATS,), float("nan"), dtype=torch.float32, device=DEV)
    ops.guidance_step_batched_(npred, lat, bc.DT, *bc.SETTINGS[setting], workspace,
                               cond_mask=mask.to(DEV) if masked else None, t=bc.MASK_T)
    return lat


@pytest.mark.parametrize("setting,b,tokens", bc.cases(), ids=[f"{s}-b{b}-t{t}" for s, b, t in bc.cases()])
def test_batched_step_equals_the_single_steps_and_meets_the_truth(setting, b, tokens):
    from ltxmi import ops
    np_host, lat_host, mask_host = bc.inputs(setting, b, tokens)
    for lat_dtype in (torch.float32, torch.bfloat16):
        for masked in (True, False):
            what = f"{setting} b={b} tokens={tokens} {lat_dtype} masked={masked}"
            got = _run_batched(setting, b, tokens, lat_dtype, masked)                     # (c): NaN-filled workspace
            want = bc.truth(setting, b, tokens, lat_dtype, masked)
            for j in range(b):
                np_j, lat_j, mask_j = bc.video_slices(np_host, lat_host.to(lat_dtype), mask_host if masked else None, j)
                lat_j = lat_j.to(DEV)
                ws = torch.empty(ops.GUIDANCE_WORKSPACE_FLOATS, dtype=torch.float32, device=DEV)
                ops.guidance_step_(np_j.to(DEV), lat_j, bc.DT, *bc.SETTINGS[setting], ws,
                                   cond_mask=None if mask_j is None else mask_j.to(DEV), t=bc.MASK_T)
                assert torch.equal(got[j:j + 1], lat_j), f"{what}: video {j} differs from its one-sample step"   # (a)
                fig = pc.compare(got[j].cpu(), *want[j], what=f"{what} video {j}")                              # (b)
                print(f"{what} video {j}: worst element at {fig:.3f} of its bound")
            if masked:                                                    # held tokens keep their bits
                held = ~bc.moves(mask_host)
                assert torch.equal(got.cpu()[held], lat_host.to(lat_dtype)[held]), what


@pytest.mark.parametrize("setting", ["cfg+stg+rescale", "none"])
@pytest.mark.parametrize("tokens", bc.TOKENS)
def test_another_videos_noise_pred_does_not_reach_video_0(setting, tokens):
    """(d): video 1's noise_pred rows replaced (scaled by -7, plus 3) -- video 0's result keeps its bits, video 1's changes."""
    b = 2
    np_host = bc.inputs(setting, b, tokens)[0]
    other = np_host.clone()
    other[1::b] = (other[1::b].float() * -7 + 3).to(torch.bfloat16)
    for lat_dtype in (torch.float32, torch.bfloat16):
        first = _run_batched(setting, b, tokens, lat_dtype, True)
        second = _run_batched(setting, b, tokens, lat_dtype, True, npred=other)
        assert torch.equal(first[0], second[0])
        assert not torch.equal(first[1], second[1])


def test_batched_step_is_run_to_run_identical():
    runs = [_run_batched("cfg+stg+rescale", 5, bc.TOKENS_BIG, torch.float32, True) for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_python_entry_refusals():
    """ops.guidance_step_batched_ raises what ops.guidance_step_ raises: TypeError for a dtype, ValueError for a layout."""
    from ltxmi import ops
    np_host, lat, mask = bc.inputs("cfg+stg+rescale", 2, 3)
    npred, lat, mask = np_host.to(DEV), lat.to(DEV), mask.to(DEV)
    args = (bc.DT, *bc.SETTINGS["cfg+stg+rescale"])
    ws = torch.empty(2 * ops.GUIDANCE_WORKSPACE_FLOATS, dtype=torch.float32, device=DEV)
    with pytest.raises(TypeError):
        ops.guidance_step_batched_(npred.float(), lat.clone(), *args, ws)
    with pytest.raises(TypeError):
        ops.guidance_step_batched_(npred, lat.double(), *args, ws)
    with pytest.raises(ValueError):
        ops.guidance_step_batched_(npred, lat.clone().transpose(1, 2), *args, ws)
    with pytest.raises(ValueError):
        ops.guidance_step_batched_(npred[:5], lat.clone(), *args, ws)                    # 5 rows are no multiple of b = 2
    with pytest.raises(ValueError):
        ops.guidance_step_batched_(npred, lat.clone(), *args, ws[:ops.GUIDANCE_WORKSPACE_FLOATS])   # one video's workspace
    with pytest.raises(ValueError):
        ops.guidance_step_batched_(npred, lat.clone(), *args, ws, cond_mask=mask[:1])
    with pytest.raises(ValueError):
        ops.guidance_step_batched_(npred, lat.clone(), *args, ws, cond_mask=mask.double())


@pytest.mark.parametrize("lat_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("b,tokens,channels", [(2, 37, 1), (5, 4100, 128)])
def test_image_cond_noise_on_a_batch_equals_the_per_video_calls(lat_dtype, b, tokens, channels):
    """(e): ltxmi_image_cond_noise is flat over tokens x channels with a flat mask, so [b, N, C] with a [b, N] mask is served
    as it stands: every video equals its own call, the threshold masks of tests/pointwise_cases.py included."""
    from ltxmi import ops
    noise_scale, t = pc.COND_NOISE
    lat, init, noise = (pc.make_like("plain", (b, tokens, channels), seed=170 + k, dtype=lat_dtype) for k in range(3))
    mask = torch.cat([pc.threshold_mask(pc.cond_noise_threshold_masks(), tokens, seed=20 + j) for j in range(b)])
    got = ops.image_cond_noise_(lat.to(DEV).clone(), init.to(DEV), noise.to(DEV), mask.to(DEV), noise_scale, t)
    reset = False
    for j in range(b):
        one = ops.image_cond_noise_(lat[j:j + 1].to(DEV).clone(), init[j:j + 1].to(DEV).contiguous(),
                                    noise[j:j + 1].to(DEV).contiguous(), mask[j:j + 1].to(DEV).contiguous(), noise_scale, t)
        assert torch.equal(got[j:j + 1], one), j
        reset = reset or not torch.equal(one.cpu(), lat[j:j + 1])
    assert reset
