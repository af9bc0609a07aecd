"""LoRA adapters fused into the weights, on the CPU: ``lora.merged_weight`` (one rounding: the witness and the per-element
bound), ``fuse_lora`` / ``set_fused_lora_weights`` / ``unfuse_lora`` through the model's host logic on the CPU doubles
(tests/lora_fuse_cpu_cases.py, each case in a process of its own), and a fused model under sequence parallelism (gloo, two
ranks), which refuses attached adapters only."""
import os
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import lora_cpu_cases as cases
import lora_fuse_cpu_cases as fuse_cases
from test_distributed import _dit_setup, _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", sorted(fuse_cases.CASES))
def test_fused_adapters_on_the_cpu_doubles(case):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lora_fuse_cpu_cases.py"), case], capture_output=True,
                       text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


def _usp_fused_case(rank, world):
    """tests/test_distributed.py::_usp_case on a model with one FUSED adapter: never refused, plain and micro-batched within
    that test's 2e-3 of the model's own one-rank forward, and not the un-fused model's output."""
    from ltxmi import distributed as sp, loading
    ltxmi, m, x, fc, kw = _dit_setup(False)
    cfg = dict(num_attention_heads=4, attention_head_dim=64, num_layers=3, cross_attention_dim=256)
    with torch.no_grad():
        base = m(x.clone(), freqs_cis=fc, return_dict=False, **kw)[0]
        m.fuse_lora(loading.load_lora(cases.make_adapter_sd(cfg, 16, seed=5)), name="a")
        assert m.fused_lora_names() == ["a"] and m.lora_names() == []
        ref = m(x.clone(), freqs_cis=fc, return_dict=False, **kw)[0]                 # one rank, default processor
        sp.enable_sequence_parallel(m, overlap=False)
        plain = sp.usp_dit_forward(m, x.clone(), fc, **kw)[0]
        sp.enable_sequence_parallel(m)
        assert m._sp_overlap
        out = sp.usp_dit_forward(m, x.clone(), fc, **kw)[0]
    assert out.shape == ref.shape and torch.equal(out, plain)
    err = float((out.float() - ref.float()).norm() / ref.float().norm())
    moved = float((out.float() - base.float()).norm() / base.float().norm())
    assert err < 2e-3, err
    assert moved > 1e-2, moved


def _worker(rank, world, port, q):
    for p in (ROOT, os.path.join(ROOT, "ltx-video-gpupoor_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _usp_fused_case(rank, world)
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_usp_dit_forward_with_a_fused_adapter_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=30)
    for rank, res in results:
        assert res == "ok", f"rank {rank}:\n{res}"


def test_fuse_interface_and_refusals_without_a_kernel():
    """The interface stands beside ``attach_lora``; a weight that is not bf16 is refused by name before anything is written."""
    import ltxmi
    from ltxmi import loading
    from oracle import dit
    assert all(hasattr(ltxmi.Transformer3DModel, n) for n in ("fuse_lora", "set_fused_lora_weights", "unfuse_lora", "fused_lora_names"))
    cfg = dict(dit.default_2b_config(), num_attention_heads=2, attention_head_dim=64, num_layers=2, cross_attention_dim=128,
               caption_channels=128)
    m = ltxmi.Transformer3DModel(**cfg).eval()                                       # fp32 weights
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(TypeError, match="transformer_blocks.0.attn1.to_q"):
        m.fuse_lora(loading.load_lora(cases.make_adapter_sd(cfg, 16, seed=1)))
    assert m.fused_lora_names() == [] and "_lora_fused" not in m.__dict__
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    with pytest.raises(KeyError):
        m.unfuse_lora("x")
    m.unfuse_lora()                                                                  # nothing fused: nothing to do
