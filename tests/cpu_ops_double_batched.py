"""CPU stand-ins for the step kernels ``LTXVideoPipeline.__call__`` calls with several videos per call -- TEST
INFRASTRUCTURE ONLY, beside tests/cpu_ops_double.py (which stays as it is): ``ops.guidance_step_batched_`` and
``ops.image_cond_noise_``, with the kernels' argument meaning, so the pipeline's host logic (row order, masks, draws, the
per-video step) runs in the CPU container.  ``install(monkeypatch)`` swaps them in for one test."""
import torch

import cpu_ops_double


def guidance_step_batched_(noise_pred, latents, dt, guidance_scale, stg_scale, rescaling_scale, do_cfg, do_stg, do_rescale,
                           workspace, cond_mask=None, t=0.0):
    """noise_pred [num_conds * b, N, C] in chunk order, latents [b, N, C] in place, cond_mask [b, N]: video j is the
    one-sample double on noise_pred[j::b], latents[j], cond_mask[j] -- every sum per video, as the kernel's contract says."""
    b = latents.shape[0]
    assert noise_pred.shape[0] % b == 0 and noise_pred.shape[1:] == latents.shape[1:]
    assert workspace.numel() >= b * 2048
    for j in range(b):
        cpu_ops_double.guidance_step_(noise_pred[j::b], latents[j:j + 1], dt, guidance_scale, stg_scale, rescaling_scale,
                                      do_cfg, do_stg, do_rescale, workspace,
                                      cond_mask=None if cond_mask is None else cond_mask[j:j + 1], t=t)
    return latents


def image_cond_noise_(latents, init_latents, noise, cond_mask, noise_scale, t):
    """pipeline_ltx_video.py:606-629 as the kernel does it: tokens with mask > 1 - 1e-6 become init + noise_scale noise t^2."""
    assert latents.shape == init_latents.shape == noise.shape and cond_mask.shape == latents.shape[:2]
    need = (cond_mask > 1.0 - 1e-6).unsqueeze(-1)
    new = init_latents.float() + noise_scale * noise.float() * (t ** 2)
    latents.copy_(torch.where(need, new, latents.float()).to(latents.dtype))
    return latents


def install(monkeypatch):
    """The one-sample step of tests/cpu_ops_double.py and the two functions above, until the test ends."""
    from ltxmi import ops
    monkeypatch.setattr(ops, "guidance_step_", cpu_ops_double.guidance_step_)
    monkeypatch.setattr(ops, "guidance_step_batched_", guidance_step_batched_, raising=False)
    monkeypatch.setattr(ops, "image_cond_noise_", image_cond_noise_)
    return ops
