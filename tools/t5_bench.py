#!/usr/bin/env python3
"""One encode of the T5-v1.1-XXL text encoder (ltxmi.T5EncoderModel: 24 blocks, d_model 4096, 64 heads, d_ff 10240; random
bf16 weights made on the device) at 2 x 256 and 2 x 128 tokens: per kernel family and in total, beside the weight-read floor.

One process on one box.  After --warmup encodes, --rounds encodes are timed: the total with device events around the
un-instrumented call (median, min, max), then the families with an event pair around every launch of a further encode per
round (ops.watch_launches), summed per family (medians over the rounds).  The floor is what reading every linear's weights
once from HBM costs -- at M = B L <= 512 rows a projection is bound by its weight bytes -- at the two rates the project
quotes: 6.29 TB/s (the measured copy rate of the chip) and 4.0 TB/s (ltxmi_norm_modulate_bf16, this library's own row kernel).
Writes profiles/t5_encoder.json (or --out PREFIX.json) and prints it; profiles/t5_encoder.md is written from it by hand.

    python tools/t5_bench.py [--rounds 7] [--warmup 2] [--layers 24] [--out profiles/t5_encoder]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

XXL = dict(d_model=4096, d_kv=64, d_ff=10240, num_heads=64, num_layers=24, vocab_size=32128, relative_attention_num_buckets=32,
           relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
HBM_RATES_TBS = {"chip copy rate 6.29 TB/s": 6.29, "own row kernel 4.0 TB/s": 4.0}


def random_state_dict(cfg, dev):
    import ltxmi
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in ltxmi.T5EncoderModel(dict(cfg)).state_dict().items()}
    g = torch.Generator(device=dev).manual_seed(0)
    sd = {}
    for name, shape in shapes.items():
        if "layer_norm" in name:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g, device=dev)
        elif "relative_attention_bias" in name or name == "shared.weight":
            t = torch.randn(shape, generator=g, device=dev)
        else:
            t = torch.randn(shape, generator=g, device=dev) / math.sqrt(shape[1])
        sd[name] = t.to(torch.bfloat16)
    return sd


def stats(xs):
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4))


def bench_shape(model, cfg, B, L, rounds, warmup):
    from ltxmi import ops
    dev = model.device
    g = torch.Generator().manual_seed(L)
    ids = torch.randint(1, cfg["vocab_size"], (B, L), generator=g).to(dev)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, L - L // 3:] = 0
    mask = mask.to(dev)
    M, D, F, H, inner = B * L, cfg["d_model"], cfg["d_ff"], cfg["num_heads"], cfg["num_heads"] * cfg["d_kv"]
    families = {
        "gemm qkv": [("gemm", M, 3 * inner, D, ops.EPI_NONE)],
        "gemm o (+ residual)": [("gemm", M, D, inner, ops.EPI_GATE_RESIDUAL)],
        "gemm wi_0 | wi_1": [("gemm", M, 2 * F, D, ops.EPI_NONE)],
        "gemm wo (+ residual)": [("gemm", M, D, F, ops.EPI_GATE_RESIDUAL)],
        "attention": [("attention_relbias", B, H, L, L, cfg["d_kv"])],
        "norm": [("rmsnorm_weight", M, D)],
        "gated gelu": [("gated_gelu", M, F)],
        "embedding": [("embedding", M, D)],
    }
    for _ in range(warmup):
        model(ids, attention_mask=mask)
    torch.cuda.synchronize()
    totals, per_family = [], {k: [] for k in families}
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model(ids, attention_mask=mask)
        e1.record()
        e1.synchronize()
        totals.append(e0.elapsed_time(e1))
        ops.watch_launches([k for keys in families.values() for k in keys])
        model(ids, attention_mask=mask)
        torch.cuda.synchronize()
        times = ops.launch_times_ms()
        ops.watch_launches(None)
        for fam, keys in families.items():
            per_family[fam].append(sum(sum(times.get(k, [])) for k in keys))
    n = cfg["num_layers"]
    weight_bytes = 2 * n * (4 * inner * D + 3 * F * D)
    launches = {"gemm qkv": n, "gemm o (+ residual)": n, "gemm wi_0 | wi_1": n, "gemm wo (+ residual)": n, "attention": n,
                "norm": 2 * n + 1, "gated gelu": n, "embedding": 1}
    fam_bytes = {"gemm qkv": 2 * n * 3 * inner * D, "gemm o (+ residual)": 2 * n * inner * D, "gemm wi_0 | wi_1": 2 * n * 2 * F * D,
                 "gemm wo (+ residual)": 2 * n * F * D}
    out = dict(B=B, L=L, rows=M, total=stats(totals), linear_weight_bytes=weight_bytes, families={})
    for fam, xs in per_family.items():
        d = dict(stats(xs), launches=launches[fam])
        if fam in fam_bytes:
            d["weight_gb"] = round(fam_bytes[fam] / 1e9, 3)
            d["weight_tb_per_s"] = round(fam_bytes[fam] / (statistics.median(xs) * 1e-3) / 1e12, 3)
            d["tflops"] = round(2 * M * (fam_bytes[fam] / 2) / (statistics.median(xs) * 1e-3) / 1e12, 1)
        out["families"][fam] = d
    out["sum_of_families_ms"] = round(sum(statistics.median(xs) for xs in per_family.values()), 4)
    out["weight_read_floor_ms"] = {k: round(weight_bytes / (r * 1e12) * 1e3, 4) for k, r in HBM_RATES_TBS.items()}
    out["total_over_floor"] = {k: round(out["total"]["median_ms"] / v, 2) for k, v in out["weight_read_floor_ms"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_encoder"))
    a = ap.parse_args()
    from ltxmi import loading
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cfg = dict(XXL, num_layers=a.layers)
    model = loading.load_t5_encoder(random_state_dict(cfg, dev), cfg, device=dev)
    res = dict(config=cfg, device=torch.cuda.get_device_name(0), rounds=a.rounds, warmup=a.warmup,
               parameters=sum(p.numel() for p in model.parameters()),
               shapes=[bench_shape(model, cfg, 2, L, a.rounds, a.warmup) for L in (256, 128)])
    res["resident_gb_after_encodes"] = round(torch.cuda.memory_allocated() / 1e9, 2)
    res["peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)           # loading holds the file's tensors beside the stacked ones
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
