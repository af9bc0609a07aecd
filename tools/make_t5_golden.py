#!/usr/bin/env python3
"""Writes tests/golden/t5_tiny.safetensors and tests/golden/t5_buckets.json: what Hugging Face ``transformers`` computes for
the tiny T5 encoder of tests/t5_double.py, so that the float64 restatement stays pinned where ``transformers`` is absent.

  t5_tiny.safetensors   input_ids [2, 24] int64, attention_mask [2, 24] int64, last_hidden_state [2, 24, 128] fp32 --
                        ``transformers.T5EncoderModel`` (eager, fp32, eval) on t5_double.init_state_dict(TINY, seed=0);
                        the weights are NOT stored: they come from the seeded CPU generator again
  t5_buckets.json       T5Attention._relative_position_bucket(d, bidirectional=True, 32, 128) for d = -511 .. 511

    python tools/make_t5_golden.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

import t5_double as td  # noqa: E402


def hf_model(cfg, sd):
    import transformers
    hf_cfg = transformers.T5Config(**{k: v for k, v in cfg.items()}, dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
    model = transformers.T5EncoderModel(hf_cfg).eval()
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"encoder.embed_tokens.weight"}, (missing, unexpected)
    return model


def hf_buckets(lo=-511, hi=511):
    from transformers.models.t5.modeling_t5 import T5Attention
    d = torch.arange(lo, hi + 1, dtype=torch.long)
    return T5Attention._relative_position_bucket(d, bidirectional=True, num_buckets=32, max_distance=128).tolist()


def main():
    sd = td.init_state_dict(td.TINY, seed=0)
    ids, mask = td.tiny_inputs()
    with torch.no_grad():
        out = hf_model(td.TINY, sd)(input_ids=ids, attention_mask=mask)[0]
    golden = os.path.join(ROOT, "tests", "golden")
    save_file({"input_ids": ids, "attention_mask": mask, "last_hidden_state": out.float().contiguous()},
              os.path.join(golden, "t5_tiny.safetensors"))
    with open(os.path.join(golden, "t5_buckets.json"), "w") as f:
        json.dump({"lo": -511, "hi": 511, "num_buckets": 32, "max_distance": 128, "buckets": hf_buckets()}, f)
    print("wrote", golden)


if __name__ == "__main__":
    main()
