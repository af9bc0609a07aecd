"""LoRA adapters as MX-FP8 operand pairs (ltxmi_gemm_mx8_pair2), measured on one device in one session, legs alternating
(the form of tools/mx8_attn_bench.py and tools/lora_bench.py).

    python tools/mx8_lora_bench.py [--out profiles/mx8_lora] [--runs 3] [--iters 50] [--steps 5] [--only linears,step,accuracy]

linears   M = 14 976, N = K1 = D for D = 2048 and 4096, K2 = 128, bf16 output with a bias:
            pair2   ops.gemm_mx8(..., a2=, w2=)                              the two-pair call
            concat  ops.gemm_mx8 on the materialised concatenation, K1 + K2  the same K-tiles on the existing kernel: the yardstick
            base    ops.gemm_mx8 on the first pair alone
            down    ops.gemm_mx8(xq, down_q, mx_out=True), N = 128           the adapter's first launch
step      bench.py's StepRunner (config 2: 768x512x97, N 4992, B_eff 3, 28 layers, step-invariant caching off) with one rank-128
          adapter on all ten linears of every block: quantised (feed-forward + the default attention set) with MX-FP8 adapters;
          quantised after fuse_lora; bf16 with the adapter unmerged; bf16 without an adapter.
accuracy  one block at the 2B widths (the "2b" case of tests/test_gpu_mx8_model.py), bf16 and fp32 stream, r16 + r128 adapters:
          relative L2 against the fp32 oracle on merged weights of MX base + MX adapters, MX base quantised from fused weights,
          and bf16 unmerged.
Writes <out>.json and the tables of <out>.md; what an existing <out>.md holds from its ``<!-- notes:`` line on (the hand-written
reading of the figures, and `python bench.py` against the parent commit, which needs a second checkout) is kept."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, _p)

import torch  # noqa: E402

M, K2 = 14976, 128
NOTES_MARK = "<!-- notes:"      # <out>.md from this line on is written by hand (what the figures say, bench.py against the parent)


def spread(v):
    return dict(runs_ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def linear_legs(D, ops, dev):
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(D)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    xq, wq = ops.quantize_mx8(rn(M, D).to(bf)), ops.quantize_mx8((rn(D, D) * D ** -0.5).to(bf))
    down_q = ops.quantize_mx8((rn(K2, D) * D ** -0.5).to(bf))
    up_q = ops.quantize_mx8((rn(D, K2) * 0.02).to(bf))
    bias = rn(D).to(bf)
    t = ops.gemm_mx8(*xq, *down_q, mx_out=True)
    cat = lambda a, b: torch.cat([a.view(torch.uint8), b.view(torch.uint8)], 1).contiguous()
    xc, wc = (cat(xq[0], t[0]).view(ops.E4M3), cat(xq[1], t[1])), (cat(wq[0], up_q[0]).view(ops.E4M3), cat(wq[1], up_q[1]))
    out = torch.empty(M, D, dtype=bf, device=dev)
    legs = {"pair2": lambda: ops.gemm_mx8(*xq, *wq, bias=bias, out=out, a2=t, w2=up_q),
            "concat": lambda: ops.gemm_mx8(*xc, *wc, bias=bias, out=out),
            "base": lambda: ops.gemm_mx8(*xq, *wq, bias=bias, out=out),
            "down": lambda: ops.gemm_mx8(*xq, *down_q, mx_out=True, out=t)}
    a = legs["pair2"]().clone()
    assert torch.equal(a, legs["concat"]()), "the two-pair call differs from the concatenated one"
    return legs


def linears(runs, iters, dev):
    from lora_bench import events_ms
    from ltxmi import ops
    res = {}
    for D in (2048, 4096):
        legs = linear_legs(D, ops, dev)
        times = {k: [] for k in legs}
        for fn in legs.values():
            events_ms(fn, 5)
        for _ in range(runs):
            for k, fn in legs.items():                  # alternating
                times[k].append(events_ms(fn, iters))
        res[str(D)] = {k: spread(v) for k, v in times.items()}
    return res


def step_times(runs, steps, dev):
    import bench
    from lora_bench import events_ms
    from ltxmi import lora
    r = bench.StepRunner(dev)
    ops, m = r.ops, r.m
    ops.set_step_invariant_caching(False)
    g = torch.Generator(device=dev).manual_seed(12)
    mods = {}
    for i, blk in enumerate(m.transformer_blocks):
        for t in lora.BLOCK_TARGETS:
            n_out, n_in = lora._get(blk, t).weight.shape
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

    def quantise():
        m.quantize_ff()
        m.quantize_attention()

    def unquantise():
        m.unquantize_attention()
        m.unquantize_ff()

    def mx_adapters():
        quantise()
        m.attach_lora(adapter, name="bench", mx8=True)
        return lambda: (m.detach_lora(), unquantise())

    def fused():
        m.fuse_lora(adapter, name="bench")
        quantise()
        return lambda: (unquantise(), m.unfuse_lora())

    def unmerged():
        m.attach_lora(adapter, name="bench")
        return m.detach_lora

    legs = {"mx8 + mx8 adapters": mx_adapters, "fused, then mx8": fused, "bf16 + unmerged": unmerged, "bf16": lambda: (lambda: None)}
    times = {k: [] for k in legs}

    def run(leg, n):
        undo = legs[leg]()
        step(), step()                                  # quantised weights and adapter state are built here
        torch.cuda.synchronize()
        t = events_ms(step, n) if n else None
        undo()
        return t

    for leg in legs:
        run(leg, 0)
    for _ in range(runs):
        for leg in legs:                                # alternating
            times[leg].append(run(leg, steps))
    assert torch.isfinite(r.latents).all()
    res = {k: spread(v) for k, v in times.items()}
    res["config"] = ("768x512x97: N 4992, B_eff 3, 28 layers, step-invariant caching off; one rank-128 adapter on all ten linears of "
                     "every block; quantised = quantize_ff() + quantize_attention() (the default set)")
    return res


def accuracy():
    from test_gpu_lora import _adapters, _merged32
    from test_gpu_model import rel
    from test_gpu_mx8_model import _case, _forward, _oracle
    c = _case("2b")
    m = c["m"]
    adapters = _adapters(c["cfg"], [(16, 5, None, 0.5), (128, 6, 32.0, 2.0)])
    merged = dict(c, sd32=_merged32(c["sd32"], adapters))
    res = {}
    for mixed in (False, True):
        truth = _oracle(merged, torch.float32, mixed)
        tag = "_mixed" if mixed else ""

        def attach(**kw):
            for i, (ad, w) in enumerate(adapters):
                m.attach_lora(ad, weight=w, name=f"a{i}", **kw)
        attach()
        res["bf16_unmerged" + tag] = rel(_forward(c, mixed), truth)
        m.detach_lora()
        m.quantize_ff()
        m.quantize_attention(linears=("attn1.qkv", "attn1.to_out", "attn2.to_q", "attn2.to_out"))
        attach(mx8=True)
        res["mx8_base_mx8_adapters" + tag] = rel(_forward(c, mixed), truth)
        m.detach_lora()
        m.unquantize_attention()
        m.unquantize_ff()
        for i, (ad, w) in enumerate(adapters):
            m.fuse_lora(ad, weight=w, name=f"f{i}")
        m.quantize_ff()
        m.quantize_attention(linears=("attn1.qkv", "attn1.to_out", "attn2.to_q", "attn2.to_out"))
        res["mx8_base_from_fused" + tag] = rel(_forward(c, mixed), truth)
        m.unquantize_attention()
        m.unquantize_ff()
        m.unfuse_lora()
        res["adapter_quantisation_cost" + tag] = res["mx8_base_mx8_adapters" + tag] - res["mx8_base_from_fused" + tag]
    res = {k: float(f"{v:.4e}") for k, v in res.items()}
    res["case"] = ("one block at the 2B widths, N 624, B_eff 3 with the STG row, r16 + r128 on all ten linears; all six per-step linears "
                   "quantised; relative L2 against the fp32 oracle on merged weights")
    return res


def markdown(result):
    cell = lambda s: f"{s['median_ms']:.4f} ({s['min_ms']:.4f} - {s['max_ms']:.4f})"
    lines = ["# LoRA adapters as MX-FP8 operand pairs (tools/mx8_lora_bench.py)", "",
             f"{result['device']}, {result['runs']} alternating runs per leg; ms, median (min - max) over the runs.", ""]
    if "linears" in result:
        lines += [f"## Per linear (M = {M}, N = K1 = D, K2 = {K2}, {result['iters']} calls per run)", "",
                  "| D | two-pair call | concatenation on ltxmi_gemm_mx8 (yardstick) | first pair alone | down GEMM (N = 128, MX output) | "
                  "pair2 / concat | pair2 / base | pair2 median inside the yardstick's spread |", "|---|---|---|---|---|---|---|---|"]
        for D, r in result["linears"].items():
            p, c, b = r["pair2"], r["concat"], r["base"]
            lines.append(f"| {D} | {cell(p)} | {cell(c)} | {cell(b)} | {cell(r['down'])} | {p['median_ms'] / c['median_ms']:.4f} | "
                         f"{p['median_ms'] / b['median_ms']:.4f} | {'yes' if c['min_ms'] <= p['median_ms'] <= c['max_ms'] else 'no'} |")
        lines.append("")
    if "step" in result:
        lines += [f"## Step time ({result['step']['config']})", "", "| leg | ms per step: runs | median | min - max |", "|---|---|---|---|"]
        for k, s in result["step"].items():
            if k != "config":
                lines.append(f"| {k} | {', '.join(map(str, s['runs_ms']))} | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} |")
        lines.append("")
    if "accuracy" in result:
        a = result["accuracy"]
        lines += [f"## Precision cost ({a['case']})", "", "| model | rel L2, bf16 stream | rel L2, fp32 stream |", "|---|---|---|"]
        for k in ("mx8_base_mx8_adapters", "mx8_base_from_fused", "bf16_unmerged", "adapter_quantisation_cost"):
            lines.append(f"| {k} | {a[k]:.3e} | {a[k + '_mixed']:.3e} |")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx8_lora"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="linears,step,accuracy")
    a = ap.parse_args()
    dev = torch.device("cuda")
    result = dict(device=torch.cuda.get_device_name(0), runs=a.runs, iters=a.iters)
    only = a.only.split(",")
    if "linears" in only:
        result["linears"] = linears(a.runs, a.iters, dev)
    if "step" in only:
        result["step"] = step_times(a.runs, a.steps, dev)
    if "accuracy" in only:
        result["accuracy"] = accuracy()
    with open(a.out + ".json", "w") as f:
        json.dump(result, f, indent=1)
    notes = ""
    if os.path.exists(a.out + ".md"):                   # the hand-written reading of the figures stays behind the new tables
        with open(a.out + ".md") as f:
            old = f.read()
        if NOTES_MARK in old:
            notes = old[old.index(NOTES_MARK):]
    with open(a.out + ".md", "w") as f:
        f.write(markdown(result) + "\n" + notes)
    print(markdown(result))


if __name__ == "__main__":
    main()
