#!/usr/bin/env python3
"""What mixed precision costs on the config-2 step (768 x 512 x 97: N = 4992 tokens, B_eff 3, 28 layers), and what the two row
kernels of the fp32 residual stream reach.

One process, bench.py's StepRunner (same model, inputs and step body):
  step   ms per denoise step with mixed=False and mixed=True, the two alternating in rounds (device events around each round's
         steps, after a warm-up of both), median and spread over the rounds;
  rows   each new kernel on the step's own rows ([14976, 2048]) beside ltxmi_norm_modulate_bf16 on the same rows: device
         events around a run of --iters launches (2000: a window of about a tenth of a second), algorithmic bytes (from the
         shapes, below) over the time.  The launches rotate through 8 sets of buffers (0.7 .. 1.7 GB per kernel, several times the
         256 MB Infinity Cache), so a pass finds nothing of its own data cached; the run is repeated --rounds times to show its
         own spread.  The gate passes update ``h`` in place across the iterations (y is scaled by 0.01: h stays finite, checked).
Writes profiles/mixed_step.json (or --out) and prints it.

    python tools/mixed_step_time.py [--rounds 5] [--steps 6] [--iters 2000] [--out profiles/mixed_step.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import bench  # noqa: E402


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def row_kernel_bytes(rows, D, groups):
    """Algorithmic traffic of one pass (bytes): what the formula needs, each operand once."""
    tables = 2 * D * 2 + 2 * groups * D * 2
    return {
        "norm_modulate_bf16": rows * D * (2 + 2) + tables,                      # bf16 in, bf16 out
        "norm_modulate_f32in_bf16": rows * D * (4 + 2) + tables,                # fp32 in, bf16 out
        "gate_residual_f32 (attn1: rounded product, bf16 copy)": rows * D * (4 + 4 + 2 + 2) + tables // 2,
        "gate_residual_f32 (attn2: no gate)": rows * D * (4 + 4 + 2),
        "gate_residual_f32 (FF: fp32 product)": rows * D * (4 + 4 + 2) + tables // 2,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mixed_step_time.py measures on the GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    r = bench.StepRunner(dev)
    ops, m = r.ops, r.m
    ops.set_step_invariant_caching(False)                       # as bench.py's headline number: every step does all its work

    @torch.no_grad()
    def step(mixed):
        x = r.latents if mixed else r.latents.to(torch.bfloat16)          # :1061: fp32 latents go in as they are
        noise_pred = m(x.expand(bench.NUM_CONDS, -1, -1), freqs_cis=r.freqs, encoder_hidden_states=r.embeds,
                       encoder_attention_mask=r.mask, timestep=r.t_dev, skip_layer_mask=r.skip,
                       skip_layer_strategy=r.ltxmi.SkipLayerStrategy.AttentionValues, latent_shape=r.grid, ltxv_model=r.holder,
                       mixed=mixed, return_dict=False)[0]
        ops.guidance_step_(noise_pred, r.latents, r.dt, 3.0, 1.0, 0.7, True, True, True, r.ws)

    for mixed in (False, True, False, True):
        step(mixed)
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for _ in range(a.rounds):
        for mixed in (False, True):
            times[mixed].append(events_ms(lambda: step(mixed), a.steps))
    assert torch.isfinite(r.latents).all()

    def summary(xs):
        return dict(median_ms=round(statistics.median(xs), 3), min_ms=round(min(xs), 3), max_ms=round(max(xs), 3),
                    rounds_ms=[round(x, 3) for x in xs])

    result = dict(config="768x512x97: N 4992, B_eff 3, 28 layers, step-invariant caching off", steps_per_round=a.steps,
                  step=dict(bf16=summary(times[False]), mixed=summary(times[True])))
    result["step"]["mixed_minus_bf16_ms"] = round(result["step"]["mixed"]["median_ms"] - result["step"]["bf16"]["median_ms"], 3)

    # ---- the row kernels on the step's rows
    B, N, D = bench.NUM_CONDS, r.n_tok, bench.D
    rows = B * N
    g = torch.Generator(device=dev).manual_seed(5)
    SETS = 8
    hs = [torch.randn(rows, D, generator=g, device=dev) for _ in range(SETS)]
    xbs = [h.to(torch.bfloat16) for h in hs]
    ys = [torch.randn(rows, D, generator=g, device=dev).to(torch.bfloat16) * 0.01 for _ in range(SETS)]
    outs, hbs = [torch.empty_like(x) for x in xbs], [torch.empty_like(x) for x in xbs]
    table = (torch.randn(6, D, generator=g, device=dev) * 0.3).to(torch.bfloat16)
    temb = (torch.randn(B, 6 * D, generator=g, device=dev) * 0.3).to(torch.bfloat16)
    sc_e, sh_e, g_e = temb[:, D:2 * D], temb[:, :D], temb[:, 2 * D:3 * D]
    turn = [0]

    def rotating(fn):
        def call():
            i = turn[0] = (turn[0] + 1) % SETS
            fn(i)
        return call

    launches = {
        "norm_modulate_bf16": rotating(lambda i: ops.norm_modulate(xbs[i], outs[i], 1e-6, ops.NORM_RMS, table[1], sc_e, table[0], sh_e, N)),
        "norm_modulate_f32in_bf16": rotating(lambda i: ops.norm_modulate_f32in(hs[i], outs[i], 1e-6, ops.NORM_RMS, table[1], sc_e,
                                                                                table[0], sh_e, N)),
        "gate_residual_f32 (attn1: rounded product, bf16 copy)":
            rotating(lambda i: ops.gate_residual_f32_(hs[i], ys[i], table[2], g_e, N, round_product=1, h_bf16=hbs[i])),
        "gate_residual_f32 (attn2: no gate)": rotating(lambda i: ops.gate_residual_f32_(hs[i], ys[i])),
        "gate_residual_f32 (FF: fp32 product)": rotating(lambda i: ops.gate_residual_f32_(hs[i], ys[i], table[2], g_e, N, round_product=0)),
    }
    nbytes = row_kernel_bytes(rows, D, B)
    result["rows"] = dict(shape=[rows, D], iters=a.iters, buffer_sets=SETS, kernels={})
    for _ in range(2 * SETS):
        for fn in launches.values():
            fn()
    torch.cuda.synchronize()
    for name, fn in launches.items():
        runs = [events_ms(fn, a.iters) for _ in range(a.rounds)]
        us = statistics.median(runs) * 1e3
        result["rows"]["kernels"][name] = dict(
            bytes=nbytes[name], median_us=round(us, 2), min_us=round(min(runs) * 1e3, 2), max_us=round(max(runs) * 1e3, 2),
            tb_per_s=round(nbytes[name] / (us * 1e-6) / 1e12, 3),
            tb_per_s_range=[round(nbytes[name] / (max(runs) * 1e-3) / 1e12, 3), round(nbytes[name] / (min(runs) * 1e-3) / 1e12, 3)])
    ks = result["rows"]["kernels"]
    for name, k in ks.items():
        k["rate_over_norm_modulate_bf16"] = round(k["tb_per_s"] / ks["norm_modulate_bf16"]["tb_per_s"], 3)
    assert all(bool(torch.isfinite(h).all()) for h in hs)
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
