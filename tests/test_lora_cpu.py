"""LoRA adapters on the CPU: the loader's key grammar and errors, attach / detach / weights through the model's host logic on
the CPU doubles (tests/lora_cpu_cases.py, each case in a process of its own), parity with oracle/dit.py in float64 on merged
weights, the text K/V caches, and the refusals."""
import os
import subprocess
import sys

import pytest
import torch

import lora_cpu_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
CFG = dict(num_attention_heads=2, attention_head_dim=64, num_layers=2, cross_attention_dim=128)


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_host_logic_on_the_cpu_doubles(case):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lora_cpu_cases.py"), case], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


def test_double_of_the_two_pair_gemm_is_the_concatenated_gemm():
    """tests/cpu_ops_double_lora.py::gemm against a float64 statement of include/ltxmi.h, grouped and with every epilogue form."""
    import cpu_ops_double_lora as dbl
    from ltxmi import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(BF)
    M, N, K, K2 = 24, 256, 128, 64
    a, w, bias, t, w2, res = rn(M, K), rn(N, K) * 0.1, rn(N), rn(M, 2 * K2), rn(N, K2) * 0.1, rn(M, N)
    gt, ge = rn(N) * 0.5, rn(3, N) * 0.5
    acc = a.double() @ w.double().T + bias.double()
    acc[:, :128] += t[:, :K2].double() @ w2[:128].double().T
    acc[:, 128:] += t[:, K2:].double() @ w2[128:].double().T
    ss = torch.zeros(M, 2)
    out = dbl.gemm(a, w, bias, a2=t, w2=w2, a2_group_cols=128, rowsumsq=ss, rowsumsq_cols=128)
    torch.testing.assert_close(out.double(), acc, rtol=2.0 ** -8, atol=1e-6)
    torch.testing.assert_close(ss.double(), out[:, :128].double().reshape(M, 2, 64).pow(2).sum(-1), rtol=1e-5, atol=1e-6)
    gate = gt.double()[None] + ge.double().repeat_interleave(8, 0)
    buf = res.clone()
    dbl.gemm(a, w, bias, out=buf, epilogue=ops.EPI_GATE_RESIDUAL, residual=buf, gate_table=gt, gate_temb=ge, rows_per_group=8,
             a2=t, w2=w2, a2_group_cols=128)
    torch.testing.assert_close(buf.double(), res.double() + gate * acc, rtol=2.0 ** -8, atol=1e-2 * float(acc.abs().max()) * 2.0 ** -8)
    one = dbl.gemm(a, w, None, epilogue=ops.EPI_GELU_TANH, a2=t[:, :K2], w2=w2)
    want = torch.nn.functional.gelu(a.double() @ w.double().T + t[:, :K2].double() @ w2.double().T, approximate="tanh")
    torch.testing.assert_close(one.double(), want, rtol=2.0 ** -8, atol=1e-6)
    assert torch.equal(dbl.gemm(a, w, bias), dbl._base_gemm(a, w, bias))


# ---------------------------------------------------------------------------------------------------------- the loader
@pytest.mark.parametrize("prefix", ["", "diffusion_model.", "model.diffusion_model.", "transformer."])
@pytest.mark.parametrize("spelling", ["A", "down"])
@pytest.mark.parametrize("alpha", [None, 8.0])
def test_loader_reads_every_spelling(prefix, spelling, alpha):
    from ltxmi import loading, lora
    sd = cases.make_adapter_sd(CFG, 16, seed=1, alpha=alpha, prefix=prefix, spelling=spelling)
    ad = loading.load_lora(sd)
    assert sorted(ad.modules) == sorted(f"transformer_blocks.{i}.{t}" for i in range(2) for t in lora.BLOCK_TARGETS)
    down, up, al = ad.modules["transformer_blocks.1.ff.net.0.proj"]
    assert down.shape == (16, 128) and up.shape == (512, 16) and al == alpha
    assert ad.scale("transformer_blocks.1.ff.net.0.proj", 2.0) == (2.0 * 8.0 / 16 if alpha else 2.0)
    plain = cases.make_adapter_sd(CFG, 16, seed=1, alpha=alpha)
    assert torch.equal(down, plain["transformer_blocks.1.ff.net.0.proj.lora_A.weight"])


def test_loader_reads_a_safetensors_file_and_nothing_else(tmp_path):
    from safetensors.torch import save_file
    from ltxmi import loading
    sd = cases.make_adapter_sd(CFG, 16, seed=1, prefix="diffusion_model.", alpha=4.0)
    path = tmp_path / "adapter.safetensors"
    save_file(sd, str(path))
    ad = loading.load_lora(path)
    assert torch.equal(ad.modules["transformer_blocks.0.attn2.to_out.0"][1], sd["diffusion_model.transformer_blocks.0.attn2.to_out.0.lora_B.weight"])
    with pytest.raises(ValueError, match="safetensors"):
        loading.load_lora(str(tmp_path / "adapter.pt"))


def test_loader_errors():
    from ltxmi import loading
    good = cases.make_adapter_sd(CFG, 16, seed=1, targets=("attn1.to_q",), blocks=[0])
    p = "transformer_blocks.0.attn1.to_q"
    assert len(loading.load_lora(good).modules) == 1
    with pytest.raises(KeyError, match="half a pair"):
        loading.load_lora({k: v for k, v in good.items() if "lora_B" not in k})
    with pytest.raises(KeyError, match="half a pair"):
        loading.load_lora(dict(good, **{p.replace("to_q", "to_k") + ".alpha": torch.tensor(4.0)}))
    with pytest.raises(ValueError, match="do not make a pair"):
        loading.load_lora(dict(good, **{p + ".lora_B.weight": torch.zeros(128, 8, dtype=BF)}))
    with pytest.raises(KeyError, match="names no linear"):
        loading.load_lora({k.replace("attn1.to_q", "attn1.to_z"): v for k, v in good.items()})
    with pytest.raises(KeyError, match="names no linear"):
        loading.load_lora({k.replace("transformer_blocks.0.", "blocks.0."): v for k, v in good.items()})
    with pytest.raises(KeyError, match="neither"):
        loading.load_lora(dict(good, **{p + ".weight": torch.zeros(128, 128)}))
    with pytest.raises(KeyError, match="two down"):
        loading.load_lora(dict(good, **{p + ".lora_down.weight": good[p + ".lora_A.weight"]}))
    with pytest.raises(ValueError, match="scalar"):
        loading.load_lora(dict(good, **{p + ".alpha": torch.ones(2)}))
    with pytest.raises(ValueError, match="no adapter"):
        loading.load_lora({})


def _tiny_model():
    import ltxmi
    from oracle import dit
    cfg = dict(dit.default_2b_config(), caption_channels=128, **CFG)
    return ltxmi.Transformer3DModel(**cfg).to(BF).eval(), cfg


def test_attach_checks_shapes_names_and_strictness():
    """A shape that does not fit the linear and a block the model does not have raise; the four non-block linears raise under
    strict=True, listing them, and are skipped and returned under strict=False.  (No kernel runs: attach is host work.)"""
    from ltxmi import loading
    m, cfg = _tiny_model()
    sd = cases.make_adapter_sd(cfg, 16, seed=1)
    with pytest.raises(ValueError, match="but the linear is"):
        m.attach_lora(loading.load_lora(dict(sd, **{"transformer_blocks.0.ff.net.2.lora_A.weight": torch.zeros(16, 256, dtype=BF)})))
    with pytest.raises(KeyError, match="names no linear of this model"):
        m.attach_lora(loading.load_lora(cases.make_adapter_sd(cfg, 16, seed=1, blocks=[2])))
    assert m.lora_names() == []
    other = dict(sd, **{"proj_out.lora_A.weight": torch.zeros(16, 128, dtype=BF), "proj_out.lora_B.weight": torch.zeros(128, 16, dtype=BF),
                        "adaln_single.linear.lora_A.weight": torch.zeros(16, 128, dtype=BF),
                        "adaln_single.linear.lora_B.weight": torch.zeros(768, 16, dtype=BF)})
    with pytest.raises(ValueError, match="adaln_single.linear, proj_out"):
        m.attach_lora(loading.load_lora(other))
    assert m.lora_names() == [] and m.transformer_blocks[0].attn1.__dict__.get("_lora") is None
    assert m.attach_lora(loading.load_lora(other), strict=False, name="x") == ["adaln_single.linear", "proj_out"]
    assert m.lora_names() == ["x"]
    with pytest.raises(ValueError, match="attached already"):
        m.attach_lora(loading.load_lora(sd), name="x")
    with pytest.raises(KeyError):
        m.set_lora_weights({"y": 1.0})
    with pytest.raises(KeyError):
        m.detach_lora("y")
    e0 = m.transformer_blocks[0].attn2.__dict__["_lora_epoch"]
    m.set_lora_weights({"x": 0.5})
    assert m.transformer_blocks[0].attn2.__dict__["_lora_epoch"] > e0
    m.detach_lora()
    assert m.lora_names() == [] and m.transformer_blocks[1].ff.__dict__["_lora"] is None


def test_sequence_parallel_refuses_adapters():
    import ltxmi
    from ltxmi import distributed as sp, loading
    m, cfg = _tiny_model()
    m.attach_lora(loading.load_lora(cases.make_adapter_sd(cfg, 16, seed=1)))
    with pytest.raises(NotImplementedError, match="LoRA"):
        sp.usp_dit_forward(m, torch.zeros(1, 8, 128, dtype=BF), (None, None))
    blk = m.transformer_blocks[0]
    for proc in (sp.UlyssesAttnProcessor(simulate_world=1), sp.RingAttnProcessor()):
        blk.attn1.set_processor(proc)
        with pytest.raises(NotImplementedError, match="LoRA"):           # before any kernel is asked for
            blk.attn1([torch.zeros(1, 8, 128, dtype=BF)], freqs_cis=None)
    blk.attn1.set_processor(ltxmi.AttnProcessor2_0())
    m.detach_lora()
    with pytest.raises(TypeError):                                        # past the refusal: the kernels refuse CPU tensors
        blk.attn1([torch.zeros(1, 8, 128, dtype=BF)], freqs_cis=None)


def test_pipeline_signature_is_untouched():
    """Adapters are state of ``pipeline.transformer``: the pipeline call keeps the reference's signature."""
    import inspect
    import ltxmi
    assert not any("lora" in p.lower() for p in inspect.signature(ltxmi.LTXVideoPipeline.__call__).parameters)
    assert all(hasattr(ltxmi.Transformer3DModel, n) for n in ("attach_lora", "set_lora_weights", "detach_lora"))
