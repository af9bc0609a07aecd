"""Cases and float64 truth of the batched guidance + Euler step (ltxmi_guidance_step_batched_bf16) -- TEST INFRASTRUCTURE
ONLY (plain module, no GPU).  Shared by tests/test_batched_step_cases.py (CPU) and tests/test_gpu_batched_step.py (MI355X).

LAYOUT.  noise_pred bf16 [num_conds * b, tokens, CHANNELS] in chunk order (uncond x b, text x b, perturbed x b), latents
[b, tokens, CHANNELS], cond_mask fp32 [b, tokens]: video j's one-sample inputs are noise_pred[j::b], latents[j:j + 1],
cond_mask[j:j + 1] (``video_slices``).

THE VIDEOS OF A CASE DIFFER, so that a kernel which shares any sum between videos misses the bound by orders of magnitude
(``VIDEO`` below; sigma_j = 2 scale_j is video j's spread):
  text_j      = scale_j x (a seeded draw of its own)
  uncond_j    = c_j text_j + 0.3 sigma_j noise       alpha_j = c_j / (c_j^2 + 0.09): 0.92, -1.47, 1.67, -0.49, 0.20
  perturbed_j = text_j + p_j sigma_j noise           p_j = 0.7, 1.2, 2.5, 0.1, 8: the ratio std(text) / std(out) moves with it
  mask_j      : token 0 held back (1.0), token 1 moved (0.0), the rest seeded picks of (0.0, 0.3, 1.0), other picks per video;
                at MASK_T = 0.63 a token moves iff 0.63 - 1e-6 < 1 - mask, and 1 - mask is 1.0, 0.7 or 0.0: nowhere near the
                threshold (that edge is tests/pointwise_cases.py's, on the same kernels).
tests/test_batched_step_cases.py asserts, in float64, that the alphas of any two videos of a case differ by more than 0.5
and their rescale factors by more than 0.1 wherever the setting uses them.

TRUTH AND BOUND.  Per video, ``pointwise_cases.guidance_step_op`` in float64 (the oracle's guidance, then the Euler update)
on that video's slices, with the held tokens left as they are; the bound is ``pointwise_cases.compare``: the whole-tensor
``check`` plus the per-element 2^-7 |truth| + SLACK mag that module derives for the one-sample step -- unchanged, no new
number.

SIZES.  tokens 3 (n = 3 CHANNELS: one ragged block) and TOKENS_BIG: n = 256 blocks x 256 threads + CHANNELS, just past one
full trip of the capped grid, so every thread of every video takes a second trip and all but CHANNELS of them find nothing
there."""
import torch

import pointwise_cases as pc

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64

CHANNELS = 4
GRID_CAP_BLOCKS, BLOCK_THREADS = pc.CAPS["guidance"][:2]                # 256 x 256: pointwise.hip's capped guidance grid
TOKENS_BIG = GRID_CAP_BLOCKS * BLOCK_THREADS // CHANNELS + 1            # n = 65536 + CHANNELS
TOKENS = [3, TOKENS_BIG]
BATCHES = [1, 2, 5]
DT, MASK_T = pc.GUIDANCE_DT, 0.63

# (guidance_scale, stg_scale, rescaling_scale, do_cfg, do_stg, do_rescale): every consistent combination of (CFG, STG), each
# without and with the rescale, and CFG + STG at guidance scale exactly 1 (do_cfg set, the CFG branch skipped)
SETTINGS = {
    "none": (0.0, 0.0, 1.0, False, False, False), "none+rescale": (0.0, 0.0, 0.7, False, False, True),
    "cfg": (3.0, 0.0, 1.0, True, False, False), "cfg+rescale": (3.0, 0.0, 0.7, True, False, True),
    "stg": (0.0, 1.0, 1.0, False, True, False), "stg+rescale": (0.0, 1.0, 0.7, False, True, True),
    "cfg+stg": (3.0, 1.0, 1.0, True, True, False), "cfg+stg+rescale": (3.0, 1.0, 0.7, True, True, True),
    "gs1+stg+rescale": (1.0, 1.0, 0.7, True, True, True),
}

# per video: (scale, c of uncond = c text + noise, p of perturbed = text + p sigma noise)
VIDEO = [(1.0, 1.0, 0.7), (3.0, -0.5, 1.2), (0.5, 0.3, 2.5), (2.0, -2.0, 0.1), (1.5, 5.0, 8.0)]
MASK_VALUES = (0.0, 0.3, 1.0)


def uses_alpha(setting):
    gs, _, _, do_cfg, _, _ = SETTINGS[setting]
    return do_cfg and gs not in (0.0, 1.0)


def uses_factor(setting):
    _, stg, _, _, do_stg, do_rescale = SETTINGS[setting]
    return do_stg and do_rescale and stg > 0


def num_conds(setting):
    return 1 + int(SETTINGS[setting][3]) + int(SETTINGS[setting][4])


_cache = {}


def inputs(setting, b, tokens):
    """(noise_pred bf16 [num_conds * b, tokens, CHANNELS], latents fp32 [b, tokens, CHANNELS] holding bf16 values,
    cond_mask fp32 [b, tokens]) of a case; built once and handed out as is: callers clone what they write."""
    key = (setting, b, tokens)
    if key not in _cache:
        _, _, _, do_cfg, do_stg, _ = SETTINGS[setting]
        unc, txt, ptb, lat, mask = [], [], [], [], []
        for j in range(b):
            scale, c, p = VIDEO[j]
            g = torch.Generator().manual_seed(7700 + 17 * j)
            shape, sigma = (tokens, CHANNELS), 2.0 * scale
            text = (torch.randn(shape, generator=g) * sigma).to(BF).float()
            unc.append((c * text + 0.3 * sigma * torch.randn(shape, generator=g)).to(BF))
            ptb.append((text + p * sigma * torch.randn(shape, generator=g)).to(BF))
            txt.append(text.to(BF))
            lat.append(torch.randn(shape, generator=g).to(BF).float())
            picks = torch.tensor(MASK_VALUES)[torch.randint(0, 3, (tokens,), generator=g)]
            picks[0], picks[1] = 1.0, 0.0
            mask.append(picks)
        chunks = ([unc] if do_cfg else []) + [txt] + ([ptb] if do_stg else [])
        npred = torch.stack([row for chunk in chunks for row in chunk]).contiguous()
        _cache[key] = (npred, torch.stack(lat).contiguous(), torch.stack(mask).contiguous())
    return _cache[key]


def video_slices(npred, lat, mask, j):
    """Video j's one-sample inputs (contiguous copies): noise_pred [num_conds, tokens, C], latents [1, tokens, C], mask [1, tokens]."""
    b = lat.shape[0]
    return npred[j::b].contiguous(), lat[j:j + 1].clone(), None if mask is None else mask[j:j + 1].contiguous()


def moves(mask):
    """Which tokens the step advances at MASK_T, decided in fp32 as the kernel and the reference decide it."""
    return torch.tensor(MASK_T, dtype=F32) - torch.tensor(1e-6, dtype=F32) < 1.0 - mask.to(F32)


def truth(setting, b, tokens, lat_dtype, masked, dt=F64):
    """Per video (value, mag) [tokens, CHANNELS] of the step in ``dt``: float64 = the truth.  ``lat_dtype`` only says which
    values the latents hold (bf16's either way: ``inputs`` rounds them)."""
    npred, lat, mask = inputs(setting, b, tokens)
    out = []
    for j in range(b):
        np_j, lat_j, mask_j = video_slices(npred, lat, mask, j)
        value, mag = pc.guidance_step_op(np_j, lat_j, DT, *SETTINGS[setting], dt=dt)
        value, mag, lat_j = value.reshape(tokens, CHANNELS), mag.reshape(tokens, CHANNELS), lat_j.to(dt).reshape(tokens, CHANNELS)
        if masked:
            mv = moves(mask_j).reshape(tokens, 1)
            value, mag = torch.where(mv, value, lat_j), torch.where(mv, mag, lat_j.abs())
        out.append((value, mag))
    return out


def scalars(setting, b, tokens):
    """Per video (alpha, rescale factor) in float64."""
    npred, lat, _ = inputs(setting, b, tokens)
    out = []
    for j in range(b):
        _, alpha, factor, _ = pc.guidance_parts(npred[j::b], *SETTINGS[setting], dt=F64)
        out.append((float(alpha), float(factor)))
    return out


def cases():
    return [(s, b, t) for s in SETTINGS for b in BATCHES for t in TOKENS]
