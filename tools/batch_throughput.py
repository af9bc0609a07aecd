#!/usr/bin/env python3
"""Videos per second for b videos in ONE pipeline call against b single calls in sequence.

Size: config 2 (768 x 512 x 97: N = 4992 tokens, 28 layers, random-init 2B weights as bench.py builds them),
``LTXVideoPipeline.__call__`` itself with ``output_type="latent"`` (prompt embeddings in, latents out: the denoise loop with
its host work, no T5, no VAE), b = 1, 2, 3, 4, every video with a prompt row and a generator of its own.
  (a) distilled  8 steps, guidance scale 1, STG 0: B_eff = b
  (b) dev        --dev-steps steps (40), guidance scale 3, STG 1 with block 19 skipped, rescale 0.7, joint_pass, and the
                 product's defaults stg_row_dedup / dead_row_elimination on: B_eff = 3 b
One process, one box; per b the two forms alternate (batched call, then the b single calls) for --rounds rounds after a
warm-up of both; wall clock around each form with a device synchronisation at both ends.  Medians, with the rounds' spread.
Writes profiles/batched_generation.json (or --out) and prints it; --bench-json embeds the box's ``python bench.py`` line.

    python tools/batch_throughput.py [--rounds 5] [--dev-steps 40] [--batches 1 2 3 4] [--bench-json FILE] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dev-steps", type=int, default=40)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 3, 4])
    ap.add_argument("--bench-json", default=None, help="a file holding the box's `python bench.py` result line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched_generation.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "batch_throughput.py measures on the GPU"
    import ltxmi
    dev = "cuda:0"
    torch.cuda.set_device(0)
    m, _ = bench.build_transformer(dev)
    pipe = ltxmi.LTXVideoPipeline(transformer=m, scheduler=ltxmi.RectifiedFlowScheduler(shifting="SD3", target_shift_terminal=0.1))
    bmax = max(a.batches)
    g = torch.Generator(device=dev).manual_seed(0)
    emb, neg = (torch.randn(bmax, bench.T_TEXT, 4096, generator=g, device=dev).to(torch.bfloat16) for _ in range(2))
    mask, nmask = torch.zeros(bmax, bench.T_TEXT, device=dev), torch.zeros(bmax, bench.T_TEXT, device=dev)
    mask[:, :96] = 1
    nmask[:, :8] = 1
    settings = {
        "distilled": dict(num_inference_steps=8, guidance_scale=1.0, stg_scale=0.0, rescaling_scale=1.0),
        "dev": dict(num_inference_steps=a.dev_steps, guidance_scale=3.0, stg_scale=1.0, rescaling_scale=0.7, skip_block_list=[19],
                    skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues),
    }
    chunks = {"distilled": 1, "dev": 3}

    def generate(rows, seeds, kw):
        out = pipe(height=512, width=768, num_frames=97, frame_rate=25.0, output_type="latent", is_video=True, joint_pass=True,
                   prompt_embeds=emb[rows], prompt_attention_mask=mask[rows], negative_prompt_embeds=neg[rows],
                   negative_prompt_attention_mask=nmask[rows],
                   generator=[torch.Generator(device=dev).manual_seed(s) for s in seeds], **kw)
        assert out.shape == (len(seeds), bench.C_LAT) + bench.GRID
        return out

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def summary(xs, videos, steps, rows_per_step):
        """rows_per_s: transformer rows (a video's chunk of one step) per second, the unit of README's B_eff figures."""
        med = statistics.median(xs)
        return dict(median_s=round(med, 4), min_s=round(min(xs), 4), max_s=round(max(xs), 4), rounds_s=[round(x, 4) for x in xs],
                    videos_per_s=round(videos / med, 4), rows_per_s=round(steps * rows_per_step / med, 2))

    result = dict(config="768x512x97: N 4992, 28 layers, random-init 2B weights, output_type=latent, joint_pass",
                  rounds=a.rounds, settings={k: {kk: (vv.name if hasattr(vv, "name") else vv) for kk, vv in v.items()}
                                             for k, v in settings.items()}, results={})
    for name, kw in settings.items():
        steps = kw["num_inference_steps"]
        per_b = result["results"][name] = {}
        for b in a.batches:
            seeds = list(range(100, 100 + b))

            def batched():
                return generate(slice(0, b), seeds, kw)

            def singles():
                return [generate(slice(j, j + 1), seeds[j:j + 1], kw) for j in range(b)]

            one, many = batched(), singles()                                    # warm-up of both forms
            equal = all(torch.equal(one[j:j + 1], many[j]) for j in range(b))
            times = {"batched": [], "singles": []}
            for _ in range(a.rounds):
                times["batched"].append(timed(batched))
                times["singles"].append(timed(singles))
            rows = chunks[name] * b
            per_b[str(b)] = dict(
                B_eff=rows, videos_bit_equal_to_single_calls=equal,
                batched=summary(times["batched"], b, steps, rows),
                singles=summary(times["singles"], b, steps, rows),
            )
            s = per_b[str(b)]
            s["batched_over_singles_videos_per_s"] = round(s["batched"]["videos_per_s"] / s["singles"]["videos_per_s"], 4)
            print(f"{name} b={b}: batched {s['batched']['videos_per_s']} videos/s, singles {s['singles']['videos_per_s']} "
                  f"videos/s, ratio {s['batched_over_singles_videos_per_s']}, bit-equal {equal}", flush=True)
    if a.bench_json:
        with open(a.bench_json) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        result["bench_py"] = json.loads(lines[-1])
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
