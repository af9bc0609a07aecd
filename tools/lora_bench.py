#!/usr/bin/env python3
"""What an unmerged LoRA adapter costs: the two-pair GEMM (ltxmi_gemm_pair2_bf16) beside the kernels of ltxmi_gemm_bf16 at the
shapes of a denoise step, and the config-2 step with rank-128 adapters on every block linear against the same step without.

One process on one box.  Per shape (M = 14976 = 3 x 4992 tokens; the 2B step's and the 13B widths' (N, K1); K2 = 128, three
groups for the packed QKV), after a warm-up of every launch, device events around a run of --iters launches, repeated --rounds
times with the four launches alternating inside a round; medians and the spread over the rounds:
  pair2       the two-pair call (the non-persistent two-pair kernel, id 4 at these shapes)
  down        the down GEMM that makes its A2 ([M, groups * K2] from [M, K1]) -- ltxmi_gemm_bf16
  base        ltxmi_gemm_bf16 on the same base shape as the product runs it (the persistent kernel): the yardstick
  base_tile   ltxmi_gemm_bf16 with algo = 256 on the same shape (the non-persistent 256x256 kernel): separates "second pair"
              from "not persistent"
FLOPs are the algorithm's, from the shapes: 2 M N K1 (+ 2 M N K2 for pair2; 2 M K1 groups K2 for down).
  step        bench.py's StepRunner: ms per denoise step without adapters and with one rank-128 adapter on all ten linears of all
              28 blocks, the two alternating in rounds (attach_lora / detach_lora happen between the timed windows).
Writes profiles/lora_gemm.json and profiles/lora_gemm.md (or --out PREFIX) and prints the JSON.

    python tools/lora_bench.py [--rounds 5] [--iters 200] [--steps 4] [--out profiles/lora_gemm]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

M = 14976
K2 = 128
# (name, N, K1, groups, epilogue): the block linears of the 2B step (D 2048) and of the 13B widths (D 4096)
SHAPES = [("2B qkv", 6144, 2048, 3, "none"), ("2B to_out / cross to_q", 2048, 2048, 1, "none"), ("2B ff1", 8192, 2048, 1, "gelu"),
          ("2B ff2", 2048, 8192, 1, "none"),
          ("13B qkv", 12288, 4096, 3, "none"), ("13B to_out / cross to_q", 4096, 4096, 1, "none"), ("13B ff1", 16384, 4096, 1, "gelu"),
          ("13B ff2", 4096, 16384, 1, "none")]


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def summary(xs, flops=None):
    med = statistics.median(xs)
    d = dict(median_us=round(med * 1e3, 1), min_us=round(min(xs) * 1e3, 1), max_us=round(max(xs) * 1e3, 1))
    if flops:
        d["tflops"] = round(flops / (med * 1e-3) / 1e12, 1)
    return d


def gemm_shapes(ops, rounds, iters, dev):
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(11)
    rn = lambda *s: (torch.randn(*s, generator=g, device=dev) * 0.05).to(bf)
    out = []
    for name, N, K1, groups, epi in SHAPES:
        a, w, bias = rn(M, K1), rn(N, K1), rn(N)
        down, up = rn(groups * K2, K1), rn(N, K2)
        t = ops.gemm(a, down)
        c, c2 = torch.empty(M, N, dtype=bf, device=dev), torch.empty(M, N, dtype=bf, device=dev)
        e = ops.EPI_GELU_TANH if epi == "gelu" else ops.EPI_NONE
        gcols = N // groups if groups > 1 else 0
        ids = dict(pair2=ops.gemm_kernel_id(a, w, bias, out=c, epilogue=e, a2=t, w2=up, a2_group_cols=gcols),
                   base=ops.gemm_kernel_id(a, w, bias, out=c, epilogue=e), base_tile=ops.gemm_kernel_id(a, w, bias, out=c, epilogue=e, algo=256))
        launches = dict(pair2=lambda: ops.gemm(a, w, bias, out=c, epilogue=e, a2=t, w2=up, a2_group_cols=gcols),
                        down=lambda: ops.gemm(a, down, out=t),
                        base=lambda: ops.gemm(a, w, bias, out=c2, epilogue=e),
                        base_tile=lambda: ops.gemm(a, w, bias, out=c2, epilogue=e, algo=256))
        for fn in launches.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in launches}
        for _ in range(rounds):
            for k, fn in launches.items():
                times[k].append(events_ms(fn, iters))
        flops = dict(pair2=2.0 * M * N * (K1 + K2), down=2.0 * M * K1 * groups * K2, base=2.0 * M * N * K1, base_tile=2.0 * M * N * K1)
        row = dict(shape=name, M=M, N=N, K1=K1, K2=K2, groups=groups, epilogue=epi, kernel_ids=ids,
                   **{k: summary(v, flops[k]) for k, v in times.items()})
        med = {k: statistics.median(v) for k, v in times.items()}
        row["pair2_over_base"] = round(med["pair2"] / med["base"], 3)
        row["pair2_over_base_tile"] = round(med["pair2"] / med["base_tile"], 3)
        row["base_tile_over_base"] = round(med["base_tile"] / med["base"], 3)
        row["adapter_cost_over_base"] = round((med["pair2"] + med["down"]) / med["base"], 3)
        out.append(row)
        del a, w, bias, down, up, t, c, c2
        torch.cuda.empty_cache()
    return out


def whole_step(rounds, steps, dev):
    import bench
    from ltxmi import lora
    r = bench.StepRunner(dev)
    ops, m = r.ops, r.m
    ops.set_step_invariant_caching(False)                       # as bench.py's headline number: every step does all its work
    g = torch.Generator(device=dev).manual_seed(12)
    mods = {}
    for i, blk in enumerate(m.transformer_blocks):
        for t in lora.BLOCK_TARGETS:
            lin = lora._get(blk, t)
            n_out, n_in = lin.weight.shape
            mods[f"transformer_blocks.{i}.{t}"] = ((torch.randn(K2, n_in, generator=g, device=dev) * n_in ** -0.5).to(torch.bfloat16),
                                                   (torch.randn(n_out, K2, generator=g, device=dev) * 0.02).to(torch.bfloat16), None)
    adapter = lora.LoraAdapter(mods)

    @torch.no_grad()
    def step():
        noise_pred = m(r.latents.to(torch.bfloat16).expand(bench.NUM_CONDS, -1, -1), freqs_cis=r.freqs, encoder_hidden_states=r.embeds,
                       encoder_attention_mask=r.mask, timestep=r.t_dev, skip_layer_mask=r.skip,
                       skip_layer_strategy=r.ltxmi.SkipLayerStrategy.AttentionValues, latent_shape=r.grid, ltxv_model=r.holder,
                       return_dict=False)[0]
        ops.guidance_step_(noise_pred, r.latents, r.dt, 3.0, 1.0, 0.7, True, True, True, r.ws)

    times = {"plain": [], "lora_r128": []}
    for _ in range(2):
        step()
    m.attach_lora(adapter, name="bench")
    for _ in range(2):
        step()
    m.detach_lora()
    torch.cuda.synchronize()
    for _ in range(rounds):
        times["plain"].append(events_ms(step, steps))
        m.attach_lora(adapter, name="bench")
        torch.cuda.synchronize()
        times["lora_r128"].append(events_ms(step, steps))
        m.detach_lora()
    assert torch.isfinite(r.latents).all()
    res = {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}
    res["lora_over_plain"] = round(res["lora_r128"]["median_ms"] / res["plain"]["median_ms"], 4)
    res["config"] = "768x512x97: N 4992, B_eff 3, 28 layers, step-invariant caching off; one rank-128 adapter on all ten linears of every block"
    return res


def markdown(result):
    lines = ["# Two-pair GEMM (LoRA, unmerged) -- measured by tools/lora_bench.py", "",
             f"One box, one process; {result['rounds']} rounds x {result['iters']} launches per figure, medians (min - max) in us; "
             f"M = {M}, K2 = {K2}.", "",
             "| shape | N x K1 | groups | pair2 (id) | down | base (id) | base, algo 256 | pair2 / base | pair2 / algo 256 | algo 256 / base | (pair2 + down) / base |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    f = lambda d: f"{d['median_us']} ({d['min_us']} - {d['max_us']}), {d['tflops']} TF"
    for r in result["gemm"]:
        lines.append(f"| {r['shape']} | {r['N']} x {r['K1']} | {r['groups']} | {f(r['pair2'])} ({r['kernel_ids']['pair2']}) | {f(r['down'])} | "
                     f"{f(r['base'])} ({r['kernel_ids']['base']}) | {f(r['base_tile'])} | {r['pair2_over_base']} | {r['pair2_over_base_tile']} | "
                     f"{r['base_tile_over_base']} | {r['adapter_cost_over_base']} |")
    s = result.get("step")
    if s:
        lines += ["", f"Whole step ({s['config']}): plain {s['plain']['median_ms']} ms ({s['plain']['min_ms']} - {s['plain']['max_ms']}), "
                      f"with the adapter {s['lora_r128']['median_ms']} ms ({s['lora_r128']['min_ms']} - {s['lora_r128']['max_ms']}): "
                      f"x {s['lora_over_plain']}."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_gemm"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lora_bench.py measures on the GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    from ltxmi import ops
    result = dict(rounds=a.rounds, iters=a.iters, gemm=gemm_shapes(ops, a.rounds, a.iters, dev))
    if not a.no_step:
        result["step"] = whole_step(a.rounds, a.steps, dev)
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        f.write(text + "\n")
    with open(a.out + ".md", "w") as f:
        f.write(markdown(result))


if __name__ == "__main__":
    main()
