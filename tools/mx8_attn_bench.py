"""The four per-step attention linears of a DiT block at M = 14 976 tokens, bf16 against MX-FP8, on one device in one session
(the form of tools/mx8_ff_bench.py).

    python tools/mx8_attn_bench.py [--out profiles/mx8_attention] [--runs 3] [--iters 20] [--only linears,step,accuracy]

linears   for D = 2048 and D = 4096, each linear WITH the launch that feeds it, both between ONE pair of events (launch gaps
          included, so a quantised linear pays for its quantiser pass):
            attn1.qkv     bf16: ops.norm_modulate -> ops.gemm([3D, D], row sums)      MX: ops.norm_modulate_mx8 -> ops.gemm_mx8(row sums)
            attn1.to_out  bf16: ops.gemm(GATE_RESIDUAL, gated, in place)              MX: ops.quantize_mx8 -> ops.gemm_mx8(the same epilogue)
            attn2.to_q    bf16: ops.gemm([D, D], row sums)                            MX: ops.quantize_mx8 -> ops.gemm_mx8(row sums)
            attn2.to_out  bf16: ops.gemm(GATE_RESIDUAL, no gate, in place)            MX: ops.quantize_mx8 -> ops.gemm_mx8(the same epilogue)
            norm          ops.norm_modulate -> ops.quantize_mx8 against ops.norm_modulate_mx8 (the fused pass alone)
          The legs alternate, --runs runs each of --iters calls after 5 warm-up calls; median and spread (min - max) of the runs.
          A linear belongs in ``attn_mx8.DEFAULT_LINEARS`` when, at D = 2048, the MX median lies below the bf16 leg's fastest run.
step      bench.py's StepRunner (config 2: 768x512x97, N 4992, B_eff 3, 28 layers, step-invariant caching off): ms per denoise
          step for: no quantisation; quantize_ff(); quantize_ff() + quantize_attention(all four); and all four but one, for each.
accuracy  the whole 2B model (28 layers, N 624, B_eff 3 with the STG row) against the fp32 oracle on the device: relative L2 for
          the bf16 and the fp32 stream, for bf16, quantize_ff(), and quantize_ff() + the default and the full set.
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

M = 14976
NAMES = ("attn1.qkv", "attn1.to_out", "attn2.to_q", "attn2.to_out")


def pair_ms(calls, iters):
    """calls: functions run in order per iteration -> ms per iteration between one pair of events."""
    for _ in range(5):
        for fn in calls:
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        for fn in calls:
            fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(v):
    return dict(runs_ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def linear_legs(D, ops, dev):
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(D)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    x, a = rn(M, D).to(bf), rn(M, D).to(bf)
    wqkv, bqkv = (rn(3 * D, D) * D ** -0.5).to(bf), rn(3 * D).to(bf)
    w, b = (rn(D, D) * D ** -0.5).to(bf), rn(D).to(bf)
    table, temb = (rn(6, D) * 0.1).to(bf), (rn(3, 6 * D) * 0.1).to(bf)
    rpg = M // 3
    mod = (table[1], temb[:, D:2 * D], table[0], temb[:, :D])
    gate = dict(gate_table=table[2], gate_temb=temb[:, 2 * D:3 * D], rows_per_group=rpg)
    y, qkv, q = torch.empty(M, D, dtype=bf, device=dev), torch.empty(M, 3 * D, dtype=bf, device=dev), torch.empty(M, D, dtype=bf, device=dev)
    ss = torch.empty(M, D // 64, dtype=torch.float32, device=dev)
    xq = (torch.empty(M, D, dtype=ops.E4M3, device=dev), torch.empty(M, D // 32, dtype=torch.uint8, device=dev))
    wqkv_q, w_q = ops.quantize_mx8(wqkv), ops.quantize_mx8(w)           # once, outside the timing, as a model does
    res = rn(M, D).to(bf)
    r = [res.clone() for _ in range(4)]
    kind, eps = ops.NORM_RMS, 1e-6
    res_epi = lambda t, **kw: dict(out=t, epilogue=ops.EPI_GATE_RESIDUAL, residual=t, **kw)
    return {
        "attn1.qkv": {"bf16": [lambda: ops.norm_modulate(x, y, eps, kind, *mod, rpg),
                               lambda: ops.gemm(y, wqkv, bqkv, out=qkv, rowsumsq=ss, rowsumsq_cols=D)],
                      "mx8": [lambda: ops.norm_modulate_mx8(x, eps, kind, *mod, rpg, out=xq),
                              lambda: ops.gemm_mx8(*xq, *wqkv_q, bias=bqkv, out=qkv, rowsumsq=ss, rowsumsq_cols=D)]},
        "attn1.to_out": {"bf16": [lambda: ops.gemm(a, w, b, **res_epi(r[0], **gate))],
                         "mx8": [lambda: ops.quantize_mx8(a, out=xq), lambda: ops.gemm_mx8(*xq, *w_q, bias=b, **res_epi(r[1], **gate))]},
        "attn2.to_q": {"bf16": [lambda: ops.gemm(x, w, b, out=q, rowsumsq=ss, rowsumsq_cols=D)],
                       "mx8": [lambda: ops.quantize_mx8(x, out=xq),
                               lambda: ops.gemm_mx8(*xq, *w_q, bias=b, out=q, rowsumsq=ss, rowsumsq_cols=D)]},
        "attn2.to_out": {"bf16": [lambda: ops.gemm(a, w, b, **res_epi(r[2]))],
                         "mx8": [lambda: ops.quantize_mx8(a, out=xq), lambda: ops.gemm_mx8(*xq, *w_q, bias=b, **res_epi(r[3]))]},
        "norm": {"bf16": [lambda: ops.norm_modulate(x, y, eps, kind, *mod, rpg), lambda: ops.quantize_mx8(y, out=xq)],
                 "mx8": [lambda: ops.norm_modulate_mx8(x, eps, kind, *mod, rpg, out=xq)]},
    }, (r, res)


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

    legs = {"bf16": (False, None), "quantize_ff": (True, None), "ff+attention(all)": (True, NAMES)}
    legs.update({f"ff+all but {n}": (True, tuple(k for k in NAMES if k != n)) for n in NAMES})

    def run(leg, n):
        ff, linears = legs[leg]
        if ff:
            m.quantize_ff()
        if linears:
            m.quantize_attention(linears=linears)
        step(), step()                                  # the quantised weights are built here
        torch.cuda.synchronize()
        t = events_ms(step, n) if n else None
        if linears:
            m.unquantize_attention()
        if ff:
            m.unquantize_ff()
        return t

    times = {k: [] for k in legs}
    for leg in legs:
        run(leg, 0)
    for _ in range(runs):
        for leg in legs:                                # alternating
            times[leg].append(run(leg, steps))
    assert torch.isfinite(r.latents).all()
    res = {k: spread(v) for k, v in times.items()}
    res["config"] = "768x512x97: N 4992, B_eff 3, 28 layers, step-invariant caching off"
    return res


def accuracy():
    import ltxmi
    from ltxmi import attn_mx8
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
    res = dict(reference_bf16_eager=rel(eager, truth))
    with torch.no_grad():
        def both(tag):
            res[tag] = rel(m(x.to(DEV), **kw)[0], truth)
            res[tag + "_mixed"] = rel(m(x.float().to(DEV), mixed=True, **kw)[0], truth)
        both("bf16")
        m.quantize_ff()
        both("quantize_ff")
        for tag, linears in (("quantize_ff+attention_default", None), ("quantize_ff+attention_all", NAMES)):
            if attn_mx8.resolve(linears):
                m.quantize_attention(linears=linears)
                both(tag)
                m.unquantize_attention()
        m.unquantize_ff()
    res = {k: float(f"{v:.4e}") for k, v in res.items()}
    res["default_linears"] = list(attn_mx8.DEFAULT_LINEARS)
    res["case"] = "2B model, 28 layers, N 624, B_eff 3 with the STG row from block 19; relative L2 against the fp32 oracle"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx8_attention"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="linears,step,accuracy")
    a = ap.parse_args()
    from ltxmi import ops
    dev = "cuda"
    result = dict(M=M, runs=a.runs, iters=a.iters, device=torch.cuda.get_device_name(0), widths={})
    for D in ((2048, 4096) if "linears" in a.only else ()):
        legs, (r, res) = linear_legs(D, ops, dev)
        runs = {n: {"bf16": [], "mx8": []} for n in legs}
        for _ in range(a.runs):
            for n, two in legs.items():
                for leg in ("bf16", "mx8"):                 # alternating
                    for t in r:
                        t.copy_(res)
                    runs[n][leg].append(pair_ms(two[leg], a.iters))
        summary = {}
        for n, two in runs.items():
            s = {leg: spread(v) for leg, v in two.items()}
            s["mx8_over_bf16"] = round(s["mx8"]["median_ms"] / s["bf16"]["median_ms"], 4)
            s["faster_outside_the_bf16_spread"] = s["mx8"]["median_ms"] < s["bf16"]["min_ms"]
            summary[n] = s
        result["widths"][str(D)] = summary
        print(D, json.dumps(summary), flush=True)
    if "linears" in a.only:
        result["measured_default"] = [n for n in NAMES if result["widths"]["2048"][n]["faster_outside_the_bf16_spread"]]
        print("measured default set", result["measured_default"], flush=True)
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
        f.write(f"# Attention linears, bf16 against MX-FP8 (tools/mx8_attn_bench.py)\n\n{result['device']}, M = {M}, {a.runs} alternating "
                f"runs per leg of {a.iters} timed calls; ms per call of the linear WITH the launch that feeds it, between one pair of "
                f"events.  median (min - max) over the runs.\n\n")
        if result["widths"]:
            f.write("| D | linear | bf16 | MX-FP8 | MX / bf16 | MX median below the fastest bf16 run |\n|---|---|---|---|---|---|\n")
            fmt = lambda s: f"{s['median_ms']:.4f} ({s['min_ms']:.4f} - {s['max_ms']:.4f})"
            for D, summ in result["widths"].items():
                for n, s in summ.items():
                    f.write(f"| {D} | {n} | {fmt(s['bf16'])} | {fmt(s['mx8'])} | {s['mx8_over_bf16']} | "
                            f"{'yes' if s['faster_outside_the_bf16_spread'] else 'no'} |\n")
            f.write(f"\nThe default set by the rule (D = 2048): {', '.join(result['measured_default']) or 'none'}.\n\n")
        if "step" in result:
            st = result["step"]
            f.write(f"## Step time ({st['config']})\n\n| leg | ms per step: runs | median | min - max |\n|---|---|---|---|\n")
            for leg, v in st.items():
                if leg != "config":
                    f.write(f"| {leg} | {', '.join(str(x) for x in v['runs_ms'])} | {v['median_ms']} | {v['min_ms']} - {v['max_ms']} |\n")
            f.write("\n")
        if "accuracy" in result:
            ac = result["accuracy"]
            f.write(f"## Accuracy ({ac['case']})\n\ndefault set: {', '.join(ac['default_linears'])}\n\n| model | rel L2, bf16 stream | rel L2, fp32 stream |\n|---|---|---|\n")
            for k in ("bf16", "quantize_ff", "quantize_ff+attention_default", "quantize_ff+attention_all"):
                if k in ac:
                    f.write(f"| {k} | {ac[k]:.3e} | {ac[k + '_mixed']:.3e} |\n")
            f.write(f"| reference_bf16_eager | {ac['reference_bf16_eager']:.3e} | |\n")


if __name__ == "__main__":
    main()
