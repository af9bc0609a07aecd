#!/usr/bin/env python3
"""What fusing a LoRA adapter into the weights buys and costs (``Transformer3DModel.fuse_lora``), beside the unmerged form.

One process on one box, three legs:
  step      bench.py's StepRunner (config 2: 768x512x97, N 4992, B_eff 3, 28 layers, step-invariant caching off): ms per denoise
            step with no adapter, with one rank-128 adapter on all 280 block linears attached (unmerged), and with the same
            adapter fused; the three alternate inside a round, --rounds rounds.  The fused model issues the launches of the
            plain model, so its median is expected inside the spread of the plain runs OF THIS SESSION.
  merge     wall time (host clock around a device synchronise) of ``fuse_lora``, ``set_fused_lora_weights`` and ``unfuse_lora``
            on that 2B model (280 merges), and on one block at the 13B widths (10 merges; x 48 blocks extrapolated).
  accuracy  relative L2 against the fp32 oracle on merged weights (W + s B A formed in float64) of the fused model, the unmerged
            model and the bf16 eager rendering, on the one-block 2B-width case of tests/test_gpu_lora.py (r16 at 0.5 + r64 with
            alpha 32 at 2.0), plain and mixed.  A fused weight drops adapter contributions below half a bf16 ulp of the base
            weight, which the unmerged path keeps in its accumulator.
Writes profiles/lora_fuse.json and profiles/lora_fuse.md (or --out PREFIX) and prints the JSON.

    python tools/lora_fuse_bench.py [--rounds 3] [--steps 4] [--legs step,merge,accuracy] [--out profiles/lora_fuse]"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from lora_bench import K2, events_ms  # noqa: E402

BF = torch.bfloat16


def rank128_adapter(m, dev, seed):
    from ltxmi import lora
    g = torch.Generator(device=dev).manual_seed(seed)
    mods = {}
    for i, blk in enumerate(m.transformer_blocks):
        for t in lora.BLOCK_TARGETS:
            n_out, n_in = lora._get(blk, t).weight.shape
            mods[f"transformer_blocks.{i}.{t}"] = ((torch.randn(K2, n_in, generator=g, device=dev) * n_in ** -0.5).to(BF),
                                                   (torch.randn(n_out, K2, generator=g, device=dev) * 0.02).to(BF), None)
    return lora.LoraAdapter(mods)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ms(xs):
    return dict(median_ms=round(statistics.median(xs), 3), min_ms=round(min(xs), 3), max_ms=round(max(xs), 3), runs=[round(x, 3) for x in xs])


def step_and_merge(rounds, steps, dev):
    import bench
    r = bench.StepRunner(dev)
    ops, m = r.ops, r.m
    ops.set_step_invariant_caching(False)                       # as bench.py's headline number: every step does all its work
    adapter = rank128_adapter(m, dev, 12)

    @torch.no_grad()
    def step():
        noise_pred = m(r.latents.to(BF).expand(bench.NUM_CONDS, -1, -1), freqs_cis=r.freqs, encoder_hidden_states=r.embeds,
                       encoder_attention_mask=r.mask, timestep=r.t_dev, skip_layer_mask=r.skip,
                       skip_layer_strategy=r.ltxmi.SkipLayerStrategy.AttentionValues, latent_shape=r.grid, ltxv_model=r.holder,
                       return_dict=False)[0]
        ops.guidance_step_(noise_pred, r.latents, r.dt, 3.0, 1.0, 0.7, True, True, True, r.ws)

    def warm():
        for _ in range(2):
            step()
        torch.cuda.synchronize()

    times = {"plain": [], "unmerged_r128": [], "fused_r128": []}
    merge = {"fuse_lora": [], "set_fused_lora_weights": [], "unfuse_lora": []}
    warm()
    m.attach_lora(adapter, name="bench")
    warm()
    m.detach_lora()
    m.fuse_lora(adapter, name="bench")
    warm()
    m.unfuse_lora()
    warm()
    for _ in range(rounds):
        times["plain"].append(events_ms(step, steps))
        m.attach_lora(adapter, name="bench")
        torch.cuda.synchronize()
        times["unmerged_r128"].append(events_ms(step, steps))
        m.detach_lora()
        merge["fuse_lora"].append(wall_ms(lambda: m.fuse_lora(adapter, name="bench")))
        step()                                                  # the packs of the fused weights are built outside the window
        torch.cuda.synchronize()
        times["fused_r128"].append(events_ms(step, steps))
        merge["set_fused_lora_weights"].append(wall_ms(lambda: m.set_fused_lora_weights({"bench": 0.5})))
        merge["unfuse_lora"].append(wall_ms(lambda: m.unfuse_lora()))
        step()
        torch.cuda.synchronize()
    assert torch.isfinite(r.latents).all()
    res = {k: ms(v) for k, v in times.items()}
    p = res["plain"]
    res["unmerged_over_plain"] = round(res["unmerged_r128"]["median_ms"] / p["median_ms"], 4)
    res["fused_over_plain"] = round(res["fused_r128"]["median_ms"] / p["median_ms"], 4)
    res["fused_median_inside_plain_spread"] = bool(p["min_ms"] <= res["fused_r128"]["median_ms"] <= p["max_ms"])
    res["config"] = ("768x512x97: N 4992, B_eff 3, 28 layers, step-invariant caching off; one rank-128 adapter on all ten linears of "
                     "every block (280 linears)")
    return res, {k: ms(v) for k, v in merge.items()}


def merge_13b_block(rounds, dev):
    from test_gpu_model import build_model, dit_case
    cfg, sd32 = dit_case(32, 128, 1, (1, 2, 2), 1, 8, caption=4096, seed=26)[:2]
    m = build_model(cfg, sd32)
    adapter = rank128_adapter(m, dev, 13)
    out = {"fuse_lora": [], "set_fused_lora_weights": [], "unfuse_lora": []}
    m.fuse_lora(adapter, name="bench")
    m.unfuse_lora()
    for _ in range(rounds):
        out["fuse_lora"].append(wall_ms(lambda: m.fuse_lora(adapter, name="bench")))
        out["set_fused_lora_weights"].append(wall_ms(lambda: m.set_fused_lora_weights({"bench": 0.5})))
        out["unfuse_lora"].append(wall_ms(lambda: m.unfuse_lora()))
    res = {k: ms(v) for k, v in out.items()}
    for k in out:
        res[k]["times_48_blocks_ms"] = round(48 * res[k]["median_ms"], 1)
    return res


def accuracy():
    import pytest
    import mixed_oracle
    import test_gpu_lora as t
    from test_gpu_model import DEV, rel, run_oracles
    c = t._case_2b()
    m, (x, enc, mask, ts, frac, grid) = c["m"], c["inputs"]
    merged32 = t._merged32(c["sd32"], c["adapters"])
    truth = run_oracles(c["cfg"], merged32, x, enc, mask, ts, frac, grid, truth_device=DEV, eager_device=DEV, **c["okw"])[0]
    truth_mixed = mixed_oracle.run(merged32, c["cfg"], x, enc, mask, ts, frac, grid, torch.float32, DEV, **c["okw"])
    with pytest.MonkeyPatch.context() as mp:
        t._unmerged_linear(c["adapters"], mp)
        eager = run_oracles(c["cfg"], c["sd32"], x, enc, mask, ts, frac, grid, truth_device=DEV, eager_device=DEV, **c["okw"])[1]
        eager_mixed = mixed_oracle.run(c["sd32"], c["cfg"], x, enc, mask, ts, frac, grid, BF, DEV, **c["okw"])
    res = {}
    for how in ("fused", "unmerged"):
        for ad, w in c["adapters"]:
            (m.fuse_lora if how == "fused" else m.attach_lora)(ad, weight=w)
        res[how] = rel(t._forward(m, x, enc, mask, ts, frac, grid, **c["mkw"]), truth)
        res[how + "_mixed"] = rel(t._forward(m, x, enc, mask, ts, frac, grid, mixed=True, **c["mkw"]), truth_mixed)
        (m.unfuse_lora if how == "fused" else m.detach_lora)()
    res["bf16_eager_unmerged"], res["bf16_eager_unmerged_mixed"] = rel(eager, truth), rel(eager_mixed, truth_mixed)
    res = {k: float(f"{v:.4e}") for k, v in res.items()}
    res["case"] = "one block at the 2B widths, N 624, B_eff 3 with the STG row; adapters r16 at 0.5 and r64 (alpha 32) at 2.0 on all ten linears"
    t._2B.clear()
    return res


def markdown(result):
    f = lambda d: f"{d['median_ms']} ms ({d['min_ms']} - {d['max_ms']}; runs {', '.join(str(x) for x in d['runs'])})"
    lines = ["# LoRA fused into the weights -- measured by tools/lora_fuse_bench.py", "",
             f"Box {result['box']}, {result['device']}, one process, one session ({result['session']}); {result['rounds']} rounds, the legs of a "
             f"round alternating; {result['steps']} steps per timed window.", ""]
    s = result.get("step")
    if s:
        inside = "inside" if s["fused_median_inside_plain_spread"] else "NOT inside"
        lines += [f"## Step time ({s['config']})", "", "| leg | ms per step | / no adapter |", "|---|---|---|",
                  f"| no adapter | {f(s['plain'])} | 1 |", f"| rank-128 adapter, unmerged | {f(s['unmerged_r128'])} | {s['unmerged_over_plain']} |",
                  f"| rank-128 adapter, fused | {f(s['fused_r128'])} | {s['fused_over_plain']} |", "",
                  f"The fused median is {inside} the spread of the no-adapter runs of this session.", ""]
    for key, title in (("merge_2b", "## Cost of the merge: the 2B model, 280 linears (wall time, device synchronised)"),
                       ("merge_13b_block", "## Cost of the merge: one block at the 13B widths, 10 linears (x 48 blocks extrapolated)")):
        mg = result.get(key)
        if mg:
            lines += [title, "", "| call | wall time |" + (" x 48 |" if key == "merge_13b_block" else ""),
                      "|---|---|" + ("---|" if key == "merge_13b_block" else "")]
            for k, d in mg.items():
                lines.append(f"| {k} | {f(d)} |" + (f" {d['times_48_blocks_ms']} ms |" if key == "merge_13b_block" else ""))
            lines.append("")
    a = result.get("accuracy")
    if a:
        lines += [f"## Accuracy: relative L2 against the fp32 oracle on merged weights ({a['case']})", "",
                  "| | fused | unmerged | bf16 eager, unmerged |", "|---|---|---|---|",
                  f"| bf16 stream | {a['fused']:.3e} | {a['unmerged']:.3e} | {a['bf16_eager_unmerged']:.3e} |",
                  f"| mixed (fp32 stream) | {a['fused_mixed']:.3e} | {a['unmerged_mixed']:.3e} | {a['bf16_eager_unmerged_mixed']:.3e} |", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--legs", default="step,merge,accuracy")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_fuse"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lora_fuse_bench.py measures on the GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    legs = a.legs.split(",")
    result = dict(box=socket.gethostname(), device=f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]})", session=time.strftime("%Y-%m-%d %H:%M:%S"),
                  rounds=a.rounds, steps=a.steps)
    if "accuracy" in legs:
        result["accuracy"] = accuracy()
    if "merge" in legs:
        result["merge_13b_block"] = merge_13b_block(a.rounds, dev)
    if "step" in legs:
        result["step"], result["merge_2b"] = step_and_merge(a.rounds, a.steps, dev)
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        f.write(text + "\n")
    with open(a.out + ".md", "w") as f:
        f.write(markdown(result))


if __name__ == "__main__":
    main()
