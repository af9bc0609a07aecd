"""The case table of the batched guidance + Euler step (tests/batched_step_cases.py) and the argument checks of its C
entry, without a GPU."""
import ctypes
import itertools

import pytest
import torch

import batched_step_cases as bc
import pointwise_cases as pc


def test_the_big_size_is_one_trip_of_the_capped_grid_plus_one_token():
    assert bc.CHANNELS * bc.TOKENS_BIG == bc.GRID_CAP_BLOCKS * bc.BLOCK_THREADS + bc.CHANNELS
    assert (bc.GRID_CAP_BLOCKS, bc.BLOCK_THREADS) == (256, 256)
    assert bc.TOKENS[0] * bc.CHANNELS == 3 * bc.CHANNELS and max(bc.BATCHES) <= len(bc.VIDEO)


def test_every_consistent_guidance_combination_is_in_the_table():
    combos = {(s[3], s[4], s[5]) for s in bc.SETTINGS.values()}
    assert combos == set(itertools.product([False, True], repeat=3))
    assert any(s[0] == 1.0 and s[3] for s in bc.SETTINGS.values())          # do_cfg at guidance scale 1: the branch is skipped


@pytest.mark.parametrize("setting", list(bc.SETTINGS))
def test_the_videos_of_a_case_differ_in_every_sum(setting):
    """float64: any two videos' alphas differ by more than 0.5 and their rescale factors by more than 0.1 (where the setting
    uses them), and every video's mask holds a token back and moves one."""
    b = max(bc.BATCHES)
    sc = bc.scalars(setting, b, bc.TOKENS_BIG)
    for (a0, f0), (a1, f1) in itertools.combinations(sc, 2):
        if bc.uses_alpha(setting):
            assert abs(a0 - a1) > 0.5, (setting, sc)
        if bc.uses_factor(setting):
            assert abs(f0 - f1) > 0.1, (setting, sc)
    if not bc.uses_factor(setting):
        assert all(f == 1.0 for _, f in sc)
    for tokens in bc.TOKENS:
        mv = bc.moves(bc.inputs(setting, b, tokens)[2])
        assert bool(mv.any(dim=1).all()) and bool((~mv).any(dim=1).all())
    # the tiny size: the first two videos already differ by as much
    (a0, f0), (a1, f1) = bc.scalars(setting, 2, bc.TOKENS[0])
    assert not bc.uses_alpha(setting) or abs(a0 - a1) > 0.5, (a0, a1)
    assert not bc.uses_factor(setting) or abs(f0 - f1) > 0.1, (f0, f1)


@pytest.mark.parametrize("setting", ["cfg+stg+rescale", "stg+rescale", "cfg"])
def test_a_step_that_shares_its_sums_between_videos_misses_the_bound(setting):
    """Teeth: the one-sample fp32 restatement per video passes the bound; the same arithmetic with video 0's noise_pred rows
    summed together with video 1's (one alpha, one pair of deviations for both) misses it by orders of magnitude."""
    b, tokens = 2, bc.TOKENS_BIG
    npred, lat, _ = bc.inputs(setting, b, tokens)
    want = bc.truth(setting, b, tokens, torch.float32, masked=False)
    got = bc.truth(setting, b, tokens, torch.float32, masked=False, dt=torch.float32)
    for j in range(b):
        assert pc.element_figure(got[j][0], *want[j])[0] <= 1
    nc = bc.num_conds(setting)
    pooled = npred.reshape(nc, b * tokens, bc.CHANNELS)                       # both videos as ONE sample
    shared, _ = pc.guidance_step_op(pooled, lat.reshape(1, b * tokens, bc.CHANNELS), bc.DT, *bc.SETTINGS[setting],
                                    dt=torch.float32)
    shared = shared.reshape(b, tokens, bc.CHANNELS)
    worst = max(pc.element_figure(shared[j], *want[j])[0] for j in range(b))
    assert worst > 100, worst


# ------------------------------------------------------------------------------------------------ refusals (no device)
def _refusal_rows():
    """(what, overrides of a valid argument set, text the message must hold)."""
    return [
        ("NULL noise_pred", dict(noise_pred=None), b"noise_pred"),
        ("NULL latents", dict(latents=None), b"latents"),
        ("NULL workspace", dict(workspace=None), b"workspace"),
        ("batch 0", dict(batch=0), b"batch"),
        ("batch -3", dict(batch=-3), b"batch"),
        ("n 1", dict(n=1), b"n="),
        ("n 0", dict(n=0), b"n="),
        ("two chunks for CFG + STG", dict(num_conds=2), b"num_conds"),
        ("three chunks for STG alone", dict(do_cfg=0), b"num_conds"),
        ("mask with channels 0", dict(channels=0), b"channels"),
        ("mask with n % channels != 0", dict(channels=5), b"channels"),
        ("workspace one float short", dict(workspace_floats=2 * 2048 - 1), b"workspace_floats"),
        ("workspace sized for one video", dict(workspace_floats=2048), b"workspace_floats"),
    ]


@pytest.mark.parametrize("what,override,needle", _refusal_rows(), ids=[r[0] for r in _refusal_rows()])
def test_batched_entry_refuses_before_any_launch(what, override, needle):
    """Every invalid argument set returns LTXMI_ERR_INVALID_ARG with a message that names the argument.  Every row fails a
    check, and the checks all stand in front of the launches, so nothing is launched on these (host) pointers."""
    from ltxmi import _lib, ops
    assert ops.GUIDANCE_WORKSPACE_FLOATS == 2048
    buf = ctypes.create_string_buffer(256)
    host = ctypes.c_void_p(ctypes.addressof(buf))
    args = dict(noise_pred=host, batch=2, n=12, num_conds=3, gs=3.0, stg=1.0, rs=0.7, do_cfg=1, do_stg=1, do_rescale=1,
                latents=host, latents_bf16=0, dt=0.1, cond_mask=host, channels=4, t=0.5, workspace=host,
                workspace_floats=2 * 2048, stream=None)
    args.update(override)
    status = _lib.lib.ltxmi_guidance_step_batched_bf16(*args.values())
    message = _lib.lib.ltxmi_last_error()
    assert status == -1, (what, status, message)
    assert b"ltxmi_guidance_step_batched_bf16" in message and needle in message, (what, message)

