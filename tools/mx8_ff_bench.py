"""The feed-forward pair of a DiT block at M = 14 976 tokens, bf16 against MX-FP8, on one device in one session.

    python tools/mx8_ff_bench.py [--out profiles/mx8_ff] [--runs 3] [--iters 20]

bf16 leg   ops.gemm(GELU) -> ops.gemm(GATE_RESIDUAL, in place)                         (what the block runs today)
MX leg     ops.quantize_mx8(x) -> ops.gemm_mx8(GELU, MX output) -> ops.gemm_mx8(GATE_RESIDUAL, in place); the weights are
           quantised once, outside the timing, as a model would at load
for D = 2048 and D = 4096 (inner width 4 D).  The legs alternate, --runs times each.  A run is 5 warm-up calls, then --iters
calls of the whole pair between ONE pair of events on the launch stream (the pair's time: launch gaps included, so the MX leg
pays for its third launch), then --iters calls with every launch between events of its own (the per-kernel times).  Per kernel:
the median time of each run, PFLOP/s and the fraction of the MX-FP8 MFMA peak (5.0 PFLOP/s dense; the bf16 kernels against 2.5).
The condition for the model switch: the MEDIAN of the MX pair's run times below the FASTEST bf16 run.
step      bench.py's StepRunner (config 2: 768x512x97, N 4992, B_eff 3, 28 layers, step-invariant caching off): ms per denoise
          step without and with ``quantize_ff()``, alternating, --runs runs of --steps steps each.
accuracy  the whole 2B model (28 layers, N 624, B_eff 3 with the STG row: tests/test_gpu_model.py::test_transformer_2b_full_depth)
          against the fp32 oracle (run on the device): relative L2 of the bf16 model and of the model after ``quantize_ff()``.
Writes <out>.json and <out>.md."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, _p)

import torch  # noqa: E402

PEAK = {"bf16": 2.5e15, "mx8": 5.0e15}
M = 14976


def timed(calls, iters):
    """calls: [(name, fn)] run in order per iteration -> ({name: median ms}, ms per pair between one pair of events)."""
    for _ in range(5):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        for _, fn in calls:
            fn()
    e1.record()
    torch.cuda.synchronize()
    total = e0.elapsed_time(e1) / iters
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls] for _ in range(iters)]
    for it in range(iters):
        for (a, b), (_, fn) in zip(ev[it], calls):
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    per = {n: statistics.median(ev[it][i][0].elapsed_time(ev[it][i][1]) for it in range(iters)) for i, (n, _) in enumerate(calls)}
    return per, total


def step_times(runs, steps, dev):
    import bench
    from lora_bench import events_ms
    r = bench.StepRunner(dev)
    ops, m = r.ops, r.m
    ops.set_step_invariant_caching(False)

    @torch.no_grad()
    def step():
        noise_pred = m(r.latents.to(torch.bfloat16).expand(bench.NUM_CONDS, -1, -1), freqs_cis=r.freqs, encoder_hidden_states=r.embeds,
                       encoder_attention_mask=r.mask, timestep=r.t_dev, skip_layer_mask=r.skip,
                       skip_layer_strategy=r.ltxmi.SkipLayerStrategy.AttentionValues, latent_shape=r.grid, ltxv_model=r.holder,
                       return_dict=False)[0]
        ops.guidance_step_(noise_pred, r.latents, r.dt, 3.0, 1.0, 0.7, True, True, True, r.ws)

    times = {"bf16": [], "quantize_ff": []}
    for leg in ("bf16", "quantize_ff", "bf16"):          # warm both legs (the quantised weights are built here)
        if leg == "quantize_ff":
            m.quantize_ff()
        step(), step()
        torch.cuda.synchronize()
        if leg == "quantize_ff":
            m.unquantize_ff()
    for _ in range(runs):
        times["bf16"].append(events_ms(step, steps))
        m.quantize_ff()
        step()
        torch.cuda.synchronize()
        times["quantize_ff"].append(events_ms(step, steps))
        m.unquantize_ff()
    assert torch.isfinite(r.latents).all()
    res = {k: dict(runs_ms=[round(x, 3) for x in v], median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3),
                   max_ms=round(max(v), 3)) for k, v in times.items()}
    res["quantised_over_bf16"] = round(res["quantize_ff"]["median_ms"] / res["bf16"]["median_ms"], 4)
    res["config"] = "768x512x97: N 4992, B_eff 3, 28 layers, step-invariant caching off"
    return res


def accuracy():
    import ltxmi
    from oracle import dit
    from test_gpu_model import DEV, _Holder, build_model, dit_case, rel, run_oracles
    grid, B, T = (2, 13, 24), 3, 256
    cfg, sd32, x, enc, mask, ts, frac = dit_case(32, 64, 28, grid, B, T, caption=4096, seed=26)
    skip = dit.create_skip_layer_mask(28, 1, 3, 2, [19], torch.float32)
    truth, eager = run_oracles(cfg, sd32, x, enc, mask, ts, frac, grid, truth_device=DEV, eager_device=DEV, skip_layer_mask=skip,
                               skip_layer_strategy=dit.ATTENTION_VALUES)
    m = build_model(cfg, sd32)
    kw = dict(freqs_cis=m.precompute_freqs_cis(frac.to(DEV)), encoder_hidden_states=enc.to(DEV), encoder_attention_mask=mask.to(DEV),
              timestep=ts.to(DEV), skip_layer_mask=m.create_skip_layer_mask(1, 3, 2, [19]),
              skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues, latent_shape=grid, ltxv_model=_Holder(), return_dict=False)
    with torch.no_grad():
        res = dict(bf16=rel(m(x.to(DEV), **kw)[0], truth), reference_bf16_eager=rel(eager, truth))
        m.quantize_ff()
        res["quantize_ff"] = rel(m(x.to(DEV), **kw)[0], truth)
        res["quantize_ff_mixed"] = rel(m(x.float().to(DEV), mixed=True, **kw)[0], truth)
        m.unquantize_ff()
        res["bf16_mixed"] = rel(m(x.float().to(DEV), mixed=True, **kw)[0], truth)
    res = {k: float(f"{v:.4e}") for k, v in res.items()}
    res["case"] = "2B model, 28 layers, N 624, B_eff 3 with the STG row from block 19; relative L2 against the fp32 oracle"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx8_ff"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="pair,step,accuracy")
    a = ap.parse_args()
    from ltxmi import ops
    dev, bf = "cuda", torch.bfloat16
    result = dict(M=M, runs=a.runs, iters=a.iters, device=torch.cuda.get_device_name(0), widths={})
    for D in ((2048, 4096) if "pair" in a.only else ()):
        g = torch.Generator(device=dev).manual_seed(D)
        rn = lambda *s: torch.randn(*s, generator=g, device=dev)
        x = rn(M, D).to(bf)
        w1, b1 = (rn(4 * D, D) * D ** -0.5).to(bf), rn(4 * D).to(bf)
        w2, b2 = (rn(D, 4 * D) * (4 * D) ** -0.5).to(bf), rn(D).to(bf)
        res = rn(M, D).to(bf)
        gate_table, temb = (rn(D) * 0.1).to(bf), (rn(3, 6 * D) * 0.1).to(bf)
        gate = dict(gate_table=gate_table, gate_temb=temb[:, 2 * D:3 * D], rows_per_group=M // 3)
        h = torch.empty(M, 4 * D, dtype=bf, device=dev)
        w1q, w2q = ops.quantize_mx8(w1), ops.quantize_mx8(w2)
        xq = (torch.empty(M, D, dtype=ops.E4M3, device=dev), torch.empty(M, D // 32, dtype=torch.uint8, device=dev))
        hq = (torch.empty(M, 4 * D, dtype=ops.E4M3, device=dev), torch.empty(M, 4 * D // 32, dtype=torch.uint8, device=dev))
        r1, r2 = res.clone(), res.clone()
        legs = {
            "bf16": [("ff1", lambda: ops.gemm(x, w1, b1, out=h, epilogue=ops.EPI_GELU_TANH)),
                     ("ff2", lambda: ops.gemm(h, w2, b2, out=r1, epilogue=ops.EPI_GATE_RESIDUAL, residual=r1, **gate))],
            "mx8": [("quantize", lambda: ops.quantize_mx8(x, out=xq)),
                    ("ff1", lambda: ops.gemm_mx8(*xq, *w1q, bias=b1, epilogue=ops.EPI_GELU_TANH, mx_out=True, out=hq)),
                    ("ff2", lambda: ops.gemm_mx8(*hq, *w2q, bias=b2, out=r2, epilogue=ops.EPI_GATE_RESIDUAL, residual=r2, **gate))],
        }
        runs = {k: [] for k in legs}
        for _ in range(a.runs):
            for leg, calls in legs.items():                     # alternating
                r1.copy_(res), r2.copy_(res)
                per, total = timed(calls, a.iters)
                runs[leg].append(dict(per_kernel_ms=per, pair_ms=total))
        flop = 2.0 * M * D * 4 * D
        summary = {}
        for leg, rs in runs.items():
            pair = [r["pair_ms"] for r in rs]
            kern = {n: statistics.median(r["per_kernel_ms"][n] for r in rs) for n in rs[0]["per_kernel_ms"]}
            summary[leg] = dict(pair_ms_runs=pair, pair_ms_median=statistics.median(pair), pair_ms_fastest=min(pair), kernel_ms=kern,
                                pflops={n: flop / (kern[n] * 1e-3) / 1e15 for n in ("ff1", "ff2")},
                                of_peak={n: flop / (kern[n] * 1e-3) / PEAK[leg] for n in ("ff1", "ff2")},
                                of_mx8_peak={n: flop / (kern[n] * 1e-3) / PEAK["mx8"] for n in ("ff1", "ff2")})
        summary["merge_condition_holds"] = summary["mx8"]["pair_ms_median"] < summary["bf16"]["pair_ms_fastest"]
        result["widths"][str(D)] = summary
        print(D, json.dumps(summary), flush=True)
    if "step" in a.only:
        result["step"] = step_times(a.runs, a.steps, dev)
        print("step", json.dumps(result["step"]), flush=True)
    if "accuracy" in a.only:
        result["accuracy"] = accuracy()
        print("accuracy", json.dumps(result["accuracy"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(result, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write(f"# Feed-forward pair, bf16 against MX-FP8 (tools/mx8_ff_bench.py)\n\n{result['device']}, M = {M}, {a.runs} alternating runs "
                f"per leg of {a.iters} timed calls; times in ms.  Pair: the whole pair between one pair of events (launch gaps "
                f"included); kernels: each launch between its own events, median over the runs.\n\n")
        f.write("| D | leg | quantize | FF1 | FF2 | pair: runs | pair: median | FF1 PFLOP/s (of MX peak) | FF2 PFLOP/s (of MX peak) |\n|---|---|---|---|---|---|---|---|---|\n")
        for D, s in result["widths"].items():
            for leg in ("bf16", "mx8"):
                v = s[leg]
                qt = f"{v['kernel_ms']['quantize']:.3f}" if "quantize" in v["kernel_ms"] else "--"
                f.write(f"| {D} | {leg} | {qt} | {v['kernel_ms']['ff1']:.3f} | {v['kernel_ms']['ff2']:.3f} | "
                        f"{', '.join(f'{p:.3f}' for p in v['pair_ms_runs'])} | {v['pair_ms_median']:.3f} | "
                        f"{v['pflops']['ff1']:.3f} ({v['of_mx8_peak']['ff1']:.2f}) | {v['pflops']['ff2']:.3f} ({v['of_mx8_peak']['ff2']:.2f}) |\n")
        f.write("\n")
        for D, s in result["widths"].items():
            f.write(f"D = {D}: median of the MX-FP8 pair {s['mx8']['pair_ms_median']:.3f} ms against the fastest bf16 run "
                    f"{s['bf16']['pair_ms_fastest']:.3f} ms: the merge condition {'holds' if s['merge_condition_holds'] else 'does NOT hold'}.\n\n")
        if "step" in result:
            st = result["step"]
            f.write(f"## Step time ({st['config']})\n\n| leg | ms per step: runs | median |\n|---|---|---|\n")
            for leg in ("bf16", "quantize_ff"):
                f.write(f"| {leg} | {', '.join(str(x) for x in st[leg]['runs_ms'])} | {st[leg]['median_ms']} |\n")
            f.write(f"\nquantised / bf16 = {st['quantised_over_bf16']}\n\n")
        if "accuracy" in result:
            ac = result["accuracy"]
            f.write(f"## Accuracy ({ac['case']})\n\n| model | rel L2 |\n|---|---|\n")
            for k in ("bf16", "quantize_ff", "bf16_mixed", "quantize_ff_mixed", "reference_bf16_eager"):
                f.write(f"| {k} | {ac[k]:.3e} |\n")


if __name__ == "__main__":
    main()
