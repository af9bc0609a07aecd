"""LoRA adapters on a real MI355X: ``Transformer3DModel`` with adapters attached (the two-pair GEMM kernels on the model's own
shapes, with every fused epilogue) under ``assert_parity`` of tests/test_gpu_model.py:

        err(ours) <= err(bf16 eager, unmerged) + 2e-3          (relative L2 against the fp32 truth)

The truth is the oracle in fp32 on MERGED weights, ``W + s B A`` formed in float64 -- the unmerged formula without its
roundings.  The eager yardstick is the oracle's bf16 rendering with every adapted linear restated the way the reference's
patched ``nn.Linear`` computes it, ``base(x) + s * up(down(x))``, each step rounded as torch rounds it (``oracle.leaves.linear``
wrapped for the duration of the call; the oracle's files are not touched).  The oracles run on the GPU (torch's eager kernels;
nothing of libltxmi)."""
import pytest
import torch
import torch.nn.functional as F

import lora_cpu_cases as cases
import mixed_oracle
from test_gpu_model import BF, DEV, _Holder, assert_parity, build_model, dit_case, rel, run_oracles

pytestmark = pytest.mark.gpu


def _adapters(cfg, specs):
    """[(LoraAdapter, weight)] for specs = [(rank, seed, alpha, weight)] on all ten linears of every block."""
    from ltxmi import loading
    return [(loading.load_lora(cases.make_adapter_sd(cfg, r, seed=s, alpha=al)), w) for r, s, al, w in specs]


def _unmerged_linear(adapters, monkeypatch):
    """Wrap ``oracle.leaves.linear``: base(x) + s * up(down(x)) in the dtype of x, for the linears the adapters name."""
    from oracle import leaves
    table = {}
    for ad, weight in adapters:
        for path, (down, up, _) in ad.modules.items():
            table.setdefault(path, []).append((down.to(DEV), up.to(DEV), ad.scale(path, weight)))
    base = leaves.linear

    def linear(x, sd, p):
        y = base(x, sd, p)
        for down, up, s in table.get(p[:-1], ()):
            y = y + s * F.linear(F.linear(x, down.to(x.dtype)), up.to(x.dtype))
        return y

    monkeypatch.setattr(leaves, "linear", linear)
    return table


def _merged32(sd32, adapters):
    """W + s B A formed in float64 (on the device: rocBLAS), handed to the fp32 oracle."""
    out = dict(sd32)
    for ad, weight in adapters:
        for path, (down, up, _) in ad.modules.items():
            k = path + ".weight"
            w = out[k].to(device=DEV, dtype=torch.float64)
            out[k] = w + ad.scale(path, weight) * (up.to(device=DEV, dtype=torch.float64) @ down.to(device=DEV, dtype=torch.float64))
    return {k: v.float().cpu() if v.is_cuda else v for k, v in out.items()}


def _forward(m, x, enc, mask, ts, frac, grid, mixed=False, **kw):
    with torch.no_grad():
        return m(x.float().to(DEV) if mixed else x.to(DEV), freqs_cis=m.precompute_freqs_cis(frac.to(DEV)),
                 encoder_hidden_states=enc.to(DEV), encoder_attention_mask=mask.to(DEV), timestep=ts.to(DEV), latent_shape=grid,
                 ltxv_model=_Holder(), mixed=mixed, return_dict=False, **kw)[0]


_2B = {}


def _case_2b():
    """One block at the 2B widths (32 x 64, FF 8192, caption 4096), N = 624, B_eff 3 with the STG row; adapters of rank 16
    (weight 0.5) and rank 64 (alpha 32, weight 2.0) together on all ten linears.  Built once for the tests that share it."""
    if not _2B:
        import ltxmi
        from oracle import dit
        grid, B, T = (3, 13, 16), 3, 128
        cfg, sd32, x, enc, mask, ts, frac = dit_case(32, 64, 1, grid, B, T, caption=4096, seed=16)
        adapters = _adapters(cfg, [(16, 5, None, 0.5), (64, 6, 32.0, 2.0)])
        m = build_model(cfg, sd32)
        okw = dict(skip_layer_mask=dit.create_skip_layer_mask(1, 1, 3, 2, [0], torch.float32), skip_layer_strategy=dit.ATTENTION_VALUES)
        mkw = dict(skip_layer_mask=m.create_skip_layer_mask(1, 3, 2, [0]), skip_layer_strategy=ltxmi.SkipLayerStrategy.AttentionValues)
        _2B.update(cfg=cfg, sd32=sd32, inputs=(x, enc, mask, ts, frac, grid), adapters=adapters, m=m, okw=okw, mkw=mkw)
        _2B["base"] = _forward(m, *_2B["inputs"], **mkw)
        _2B["base_mixed"] = _forward(m, *_2B["inputs"], mixed=True, **mkw)
    return _2B


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _2B.clear()


def test_2b_width_block_with_two_adapters(monkeypatch):
    from ltxmi import ops
    c = _case_2b()
    m, (x, enc, mask, ts, frac, grid) = c["m"], c["inputs"]
    truth = run_oracles(c["cfg"], _merged32(c["sd32"], c["adapters"]), x, enc, mask, ts, frac, grid, truth_device=DEV,
                        eager_device=DEV, **c["okw"])[0]
    _unmerged_linear(c["adapters"], monkeypatch)
    eager = run_oracles(c["cfg"], c["sd32"], x, enc, mask, ts, frac, grid, truth_device=DEV, eager_device=DEV, **c["okw"])[1]
    for (ad, w), name in zip(c["adapters"], ("r16", "r64")):
        m.attach_lora(ad, weight=w, name=name)
    try:
        blk = m.transformer_blocks[0]
        assert blk.attn1.__dict__["_lora"]["qkv"].down.shape == (3 * 128, 2048)          # 16 + 64 = 80 -> 128, three members
        # the kernels the adapted linears take at these shapes: M = 1872 x N 6144 / 8192 are 192 / 256 tiles of 256
        e = lambda *s: torch.empty(*s, dtype=BF)
        assert ops.gemm_kernel_id(e(1872, 2048), e(6144, 2048), a2=e(1872, 384), w2=e(6144, 128), a2_group_cols=2048) == 4
        assert ops.gemm_kernel_id(e(1872, 2048), e(2048, 2048), a2=e(1872, 128), w2=e(2048, 128)) == 3
        out = _forward(m, x, enc, mask, ts, frac, grid, **c["mkw"])
        assert rel(out, c["base"]) > 5e-2, "the adapters did nothing"
        assert_parity(out, truth, eager, "2B width, 1 block, N 624, adapters r16 + r64")
        assert rel(out[2], out[1]) > 1e-3                                                # the STG row is perturbed
    finally:
        m.detach_lora()
    assert torch.equal(_forward(m, x, enc, mask, ts, frac, grid, **c["mkw"]), c["base"]), "detach_lora() does not restore the output"


def test_2b_width_block_mixed_precision(monkeypatch):
    c = _case_2b()
    m, (x, enc, mask, ts, frac, grid) = c["m"], c["inputs"]
    truth = mixed_oracle.run(_merged32(c["sd32"], c["adapters"]), c["cfg"], x, enc, mask, ts, frac, grid, torch.float32, DEV, **c["okw"])
    _unmerged_linear(c["adapters"], monkeypatch)
    eager = mixed_oracle.run(c["sd32"], c["cfg"], x, enc, mask, ts, frac, grid, BF, DEV, **c["okw"])
    for ad, w in c["adapters"]:
        m.attach_lora(ad, weight=w)
    try:
        out = _forward(m, x, enc, mask, ts, frac, grid, mixed=True, **c["mkw"])
        assert rel(out, c["base_mixed"]) > 5e-2
        assert_parity(out, truth, eager, "mixed 2B width, 1 block, N 624, adapters r16 + r64")
    finally:
        m.detach_lora()
    assert torch.equal(_forward(m, x, enc, mask, ts, frac, grid, mixed=True, **c["mkw"]), c["base_mixed"])


def test_zero_up_matrices_change_no_bit():
    """Adapters whose up matrices are zero: every adapted linear runs the two-pair kernel (ids 3 and 4 at these shapes) where
    the base model runs the 128x128 and the persistent kernel, and the model output is the base model's bit for bit -- the
    kernels agree on the model's own shapes, epilogues included (row sums, GELU, gate + residual)."""
    from ltxmi import loading, ops
    c = _case_2b()
    m, (x, enc, mask, ts, frac, grid) = c["m"], c["inputs"]
    sd = {k: (torch.zeros_like(v) if ".lora_B." in k else v) for k, v in cases.make_adapter_sd(c["cfg"], 64, seed=9).items()}
    seen = []
    real = ops.gemm

    def spy(*a, **k):
        seen.append("a2" in k)
        return real(*a, **k)

    m.attach_lora(loading.load_lora(sd))
    ops.gemm = spy
    try:
        out = _forward(m, x, enc, mask, ts, frac, grid, **c["mkw"])
        out_mixed = _forward(m, x, enc, mask, ts, frac, grid, mixed=True, **c["mkw"])
    finally:
        ops.gemm = real
        m.detach_lora()
    # per forward: QKV, to_out, cross to_q, text K/V (projected once, then cached), cross to_out, FF1, FF2
    assert sum(seen) >= 13, "the adapted linears did not take the two-pair call"
    assert torch.equal(out, c["base"]) and torch.equal(out_mixed, c["base_mixed"])


def test_13b_width_block_with_two_adapters(monkeypatch):
    """One block at the 13B widths (32 x 128, FF 16384), N = 1040, B 2: the widths of the checkpoint the reference's distilled
    rank-128 LoRA file is for."""
    grid, B, T = (5, 13, 16), 2, 128
    cfg, sd32, x, enc, mask, ts, frac = dit_case(32, 128, 1, grid, B, T, caption=4096, seed=26)
    adapters = _adapters(cfg, [(16, 5, None, 0.5), (128, 6, 64.0, 2.0)])
    truth = run_oracles(cfg, _merged32(sd32, adapters), x, enc, mask, ts, frac, grid, truth_device=DEV, eager_device=DEV)[0]
    m = build_model(cfg, sd32)
    base = _forward(m, x, enc, mask, ts, frac, grid)
    _unmerged_linear(adapters, monkeypatch)
    eager = run_oracles(cfg, sd32, x, enc, mask, ts, frac, grid, truth_device=DEV, eager_device=DEV)[1]
    for ad, w in adapters:
        m.attach_lora(ad, weight=w)
    assert m.transformer_blocks[0].ff.__dict__["_lora"]["ff2"].down.shape == (192, 16384)    # 16 + 128 = 144 -> 192
    out = _forward(m, x, enc, mask, ts, frac, grid)
    assert out.shape == (2, 1040, 128) and rel(out, base) > 5e-2
    assert_parity(out, truth, eager, "13B width, 1 block, N 1040, adapters r16 + r128")
    m.detach_lora()
    assert torch.equal(_forward(m, x, enc, mask, ts, frac, grid), base)
