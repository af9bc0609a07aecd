#!/usr/bin/env python3
"""The T5-v1.1-XXL text encoder (tools/t5_bench.py's model: 24 blocks, d_model 4096, 64 heads, d_ff 10240, random bf16 weights)
with its projections in MX-FP8 (``T5EncoderModel.quantize``), at 2 x 256 and 2 x 128 tokens.  One process on one box:

  encode      the unquantised encode (the parent's code: a model that was never quantised reaches no new op) and the quantised
              one alternate, --runs runs each; a run is --warmup encodes, then the median of --rounds encodes timed by device
              events around the un-instrumented call.  Quantised twice: with ``t5_mx8.DEFAULT_LINEARS`` and with all four linears;
  families    an event pair around every launch of one further quantised encode per round, summed per family;
  per linear  the quantised call WITH the quantiser pass it needs against the bf16 call WITH the launch that pass replaces
              (qkv, wi: the norm; o: nothing against quantize_mx8; wo: the gated GELU), on the operands of every block in turn as
              an encode meets them (no block's weights are met twice in a row), bf16 and MX-FP8 sweeps alternating.  A linear
              belongs in the default set only if its quantised pair wins at both row counts, its median outside the bf16 pair's
              spread (the rule of profiles/mx8_attention.md);
  forms       each tile form of ops.gemm_mx8_skinny forced, per shape, the same sweep;
  memory      resident bytes after ``quantize(keep_bf16=False)`` with the default set.
The floor is what reading every linear's weights once costs at the two rates the project quotes (tools/t5_bench.py).
Writes profiles/t5_mx8.json (or --out PREFIX.json) and prints it; profiles/t5_mx8.md is written from it by hand.

    python tools/t5_mx8_bench.py [--runs 3] [--rounds 7] [--warmup 2] [--layers 24] [--out profiles/t5_mx8]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from t5_bench import HBM_RATES_TBS, XXL, random_state_dict, stats  # noqa: E402


def inputs(cfg, B, L, dev):
    g = torch.Generator().manual_seed(L)
    ids = torch.randint(1, cfg["vocab_size"], (B, L), generator=g).to(dev)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, L - L // 3:] = 0
    return ids, mask.to(dev)


def time_encodes(model, ids, mask, rounds, warmup):
    for _ in range(warmup):
        model(ids, attention_mask=mask)
    torch.cuda.synchronize()
    xs = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model(ids, attention_mask=mask)
        e1.record()
        e1.synchronize()
        xs.append(e0.elapsed_time(e1))
    return statistics.median(xs)


def family_times(model, cfg, ids, mask, rounds):
    from ltxmi import ops
    B, L = ids.shape
    M, D, F, H, inner = B * L, cfg["d_model"], cfg["d_ff"], cfg["num_heads"], cfg["num_heads"] * cfg["d_kv"]
    both = lambda N, K, epi: [("gemm_mx8_skinny", M, N, K, epi), ("gemm", M, N, K, epi)]
    families = {
        "gemm qkv": both(3 * inner, D, ops.EPI_NONE), "gemm o (+ residual)": both(D, inner, ops.EPI_GATE_RESIDUAL),
        "gemm wi_0 | wi_1": both(2 * F, D, ops.EPI_NONE), "gemm wo (+ residual)": both(D, F, ops.EPI_GATE_RESIDUAL),
        "attention": [("attention_relbias", B, H, L, L, cfg["d_kv"])],
        "norm (-> MX-FP8)": [("rmsnorm_weight_mx8", M, D)], "norm (bf16)": [("rmsnorm_weight", M, D)],
        "quantise (attention context)": [("quantize_mx8", M, inner)],
        "gated gelu (-> MX-FP8)": [("gated_gelu_mx8", M, F)], "gated gelu (bf16)": [("gated_gelu", M, F)],
        "embedding": [("embedding", M, D)],
    }
    per = {k: [] for k in families}
    count = {}
    for _ in range(rounds):
        ops.watch_launches([k for keys in families.values() for k in keys])
        model(ids, attention_mask=mask)
        torch.cuda.synchronize()
        times = ops.launch_times_ms()
        ops.watch_launches(None)
        for fam, keys in families.items():
            per[fam].append(sum(sum(times.get(k, [])) for k in keys))
            count[fam] = sum(len(times.get(k, [])) for k in keys)
    n = cfg["num_layers"]
    fam_bytes = {"gemm qkv": n * 3 * inner * D, "gemm o (+ residual)": n * inner * D, "gemm wi_0 | wi_1": n * 2 * F * D,
                 "gemm wo (+ residual)": n * F * D}                        # e4m3 bytes; the scales add 1/32
    out = {}
    for fam, xs in per.items():
        if not count[fam]:
            continue
        d = dict(stats(xs), launches=count[fam], us_per_launch=round(statistics.median(xs) / count[fam] * 1e3, 1))
        if fam in fam_bytes:
            d["weight_gb"] = round(fam_bytes[fam] * 33 / 32 / 1e9, 3)
            d["weight_tb_per_s"] = round(fam_bytes[fam] * 33 / 32 / (statistics.median(xs) * 1e-3) / 1e12, 3)
        out[fam] = d
    return out


def per_linear(model, cfg, B, L, sweeps):
    """{linear: {bf16: stats of the per-block pair time in us, mx8: the same, ratio}} and the forced forms per shape."""
    from ltxmi import ops, t5_mx8
    dev = model.device
    M, D, F, inner = B * L, cfg["d_model"], cfg["d_ff"], cfg["num_heads"] * cfg["d_kv"]
    g = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev).to(torch.bfloat16)
    x, ctx, h = rnd(M, D), rnd(M, inner), rnd(M, 2 * F)
    stream = rnd(M, D)
    blocks = list(model.encoder.block)
    atts = [b.layer[0].SelfAttention for b in blocks]
    ffs = [b.layer[1].DenseReluDense for b in blocks]
    norms = [b.layer[0].layer_norm for b in blocks]
    R = ops.EPI_GATE_RESIDUAL
    model.quantize(linears=t5_mx8.LINEARS)
    for a, f in zip(atts, ffs):                  # every quantised operand exists before anything is timed
        for mod, names in ((a, ("qkv", "o")), (f, ("wi", "wo"))):
            for n in names:
                t5_mx8.weights(mod, n)
    calls = {
        "qkv": (lambda i: ops.gemm(norms[i](x), atts[i]._pack("qkv", [atts[i].q, atts[i].k, atts[i].v])),
                lambda i, form=0: ops.gemm_mx8_skinny(*ops.rmsnorm_weight_mx8(x, norms[i].weight, 1e-6), *t5_mx8.weights(atts[i], "qkv"),
                                                      form=form)),
        "o": (lambda i: ops.gemm(ctx, atts[i].o.weight, out=stream, epilogue=R, residual=stream),
              lambda i, form=0: ops.gemm_mx8_skinny(*ops.quantize_mx8(ctx), *t5_mx8.weights(atts[i], "o"), out=stream, epilogue=R,
                                                    residual=stream, form=form)),
        "wi": (lambda i: ops.gemm(norms[i](x), ffs[i]._pack("wi", [ffs[i].wi_0, ffs[i].wi_1])),
               lambda i, form=0: ops.gemm_mx8_skinny(*ops.rmsnorm_weight_mx8(x, norms[i].weight, 1e-6), *t5_mx8.weights(ffs[i], "wi"),
                                                     form=form)),
        "wo": (lambda i: ops.gemm(ops.gated_gelu(h), ffs[i].wo.weight, out=stream, epilogue=R, residual=stream),
               lambda i, form=0: ops.gemm_mx8_skinny(*ops.gated_gelu_mx8(h), *t5_mx8.weights(ffs[i], "wo"), out=stream, epilogue=R,
                                                     residual=stream, form=form)),
    }

    def sweep(fn):
        """One pass over the blocks, an event pair around each call pair -> the median per-block time in us."""
        stream.zero_()
        evs = []
        for i in range(len(blocks)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(i)
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(b) for a, b in evs) * 1e3

    out, forms = {}, {}
    for name, (bf, mx) in calls.items():
        sweep(bf), sweep(mx)                     # warm-up of both
        t = {"bf16": [], "mx8": []}
        for _ in range(sweeps):
            t["bf16"].append(sweep(bf))
            t["mx8"].append(sweep(mx))
        s = {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for k, v in t.items()}
        s["ratio"] = round(s["mx8"]["median_us"] / s["bf16"]["median_us"], 3)
        s["wins"] = s["mx8"]["median_us"] < s["bf16"]["min_us"]
        out[name] = s
        forms[name] = {}
        for form in ops.MXT_FORMS:
            sweep(lambda i: mx(i, form))
            forms[name][f"form {form}"] = round(statistics.median(sweep(lambda i: mx(i, form)) for _ in range(sweeps)), 1)
    model.unquantize()
    return out, forms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweeps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_mx8"))
    a = ap.parse_args()
    from ltxmi import loading, t5_mx8
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cfg = dict(XXL, num_layers=a.layers)
    model = loading.load_t5_encoder(random_state_dict(cfg, dev), cfg, device=dev)
    n, D, F, inner = cfg["num_layers"], cfg["d_model"], cfg["d_ff"], cfg["num_heads"] * cfg["d_kv"]
    weight_bytes = n * (4 * inner * D + 3 * F * D) * 33 // 32          # e4m3 + one scale byte per 32
    res = dict(config=cfg, device=torch.cuda.get_device_name(0), runs=a.runs, rounds=a.rounds, warmup=a.warmup, sweeps=a.sweeps,
               default_linears=list(t5_mx8.DEFAULT_LINEARS), mx8_linear_weight_bytes=weight_bytes,
               weight_read_floor_ms={k: round(weight_bytes / (r * 1e12) * 1e3, 4) for k, r in HBM_RATES_TBS.items()}, shapes=[])
    torch.cuda.empty_cache()
    res["resident_gb_bf16"] = round(torch.cuda.memory_allocated() / 1e9, 2)
    for L in (256, 128):
        ids, mask = inputs(cfg, 2, L, dev)
        legs = {"bf16": None, "mx8 default set": None, "mx8 all four": t5_mx8.LINEARS}
        runs = {k: [] for k in legs}
        for _ in range(a.runs):
            for leg, linears in legs.items():
                if leg != "bf16":
                    model.quantize(linears=linears)
                runs[leg].append(round(time_encodes(model, ids, mask, a.rounds, a.warmup), 4))
                if leg != "bf16":
                    model.unquantize()
        model.quantize()
        fam = family_times(model, cfg, ids, mask, a.rounds)
        model.unquantize()
        lin, forms = per_linear(model, cfg, 2, L, a.sweeps)
        shape = dict(B=2, L=L, rows=2 * L, encode_ms={k: dict(runs=v, median=statistics.median(v)) for k, v in runs.items()},
                     families_default_set=fam, per_linear_us=lin, forced_forms_us=forms)
        for leg in ("mx8 default set", "mx8 all four"):
            shape["encode_ms"][leg]["below_fastest_bf16_run"] = statistics.median(runs[leg]) < min(runs["bf16"])
            shape["encode_ms"][leg]["over_floor"] = {k: round(statistics.median(runs[leg]) / v, 2) for k, v in res["weight_read_floor_ms"].items()}
        res["shapes"].append(shape)
    model.quantize(keep_bf16=False)
    torch.cuda.empty_cache()
    res["resident_gb_mx8_keep_bf16_false"] = round(torch.cuda.memory_allocated() / 1e9, 2)
    ids, mask = inputs(cfg, 2, 128, dev)
    model(ids, attention_mask=mask)              # and it still encodes
    torch.cuda.synchronize()
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
