"""LoRA adapters FUSED into the weights (``fuse_lora`` / ``set_fused_lora_weights`` / ``unfuse_lora``, ``lora.merged_weight``)
through the host logic on the CPU doubles of ``ltxmi.ops`` -- run by tests/test_lora_fuse_cpu.py, each case in a process of its
own (``python tests/lora_fuse_cpu_cases.py <case>``), on the tiny DiT of tests/lora_cpu_cases.py.  TEST INFRASTRUCTURE ONLY.

The double's residual epilogue (tests/cpu_ops_double.py ``gemm``: fp32 ``a @ w^T``, ``+ residual`` in fp32, one rounding) is the
kernel's EPI_RESIDUAL as far as the merge goes -- one fp32 sum that includes the base, rounded once -- so nothing is corrected
here."""
import sys

import torch

from lora_cpu_cases import BF, F64, make_adapter_sd, merged, rel, setup

WITNESS = 1.0078125            # 1 + 2^-7: bf16(1 + 2^-8 + 2^-16); 1 + 2^-8 alone is a tie and rounds to even, 1.0


def witness_operands(n_out=128, k_in=128, device="cpu"):
    """base = 1, one entry of rank 2: up[:, 0] = up[:, 1] = 1, down[0] = 2^-8, down[1] = 2^-16, s = 1.  Rounding bf16(delta)
    before the add gives 1 + bf16(2^-8 + 2^-16) = 1 + 2^-8 -> 1.0; merging the components one after the other gives
    bf16(1 + 2^-8) = 1.0, then bf16(1 + 2^-16) = 1.0.  One rounding of the fp32 sum gives 1.0078125."""
    base = torch.ones(n_out, k_in, dtype=BF, device=device)
    up = torch.zeros(n_out, 2, dtype=BF, device=device)
    up[:, :2] = 1
    down = torch.zeros(2, k_in, dtype=BF, device=device)
    down[0], down[1] = 2.0 ** -8, 2.0 ** -16
    return base, down, up


def witness_adapters(path, n_out=128, k_in=128):
    """The two rank components of ``witness_operands`` as two adapters of rank 1 on the linear ``path``."""
    from ltxmi import loading
    _, down, up = witness_operands(n_out, k_in)
    return [loading.load_lora({path + ".lora_A.weight": down[i:i + 1].clone(), path + ".lora_B.weight": up[:, i:i + 1].clone()})
            for i in range(2)]


def drawn_operands(n_out, k_in, ranks, seed, device="cpu"):
    """(base, [(down, up, s)]) drawn as ``make_adapter_sd`` draws: down ~ in^-1/2, up ~ 0.5 r^-1/2, the base ~ in^-1/2, all bf16."""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(n_out, k_in, generator=g) * k_in ** -0.5).to(BF).to(device)
    entries = []
    for i, r in enumerate(ranks):
        down = (torch.randn(r, k_in, generator=g) * k_in ** -0.5).to(BF).to(device)
        up = (torch.randn(n_out, r, generator=g) * 0.5 * r ** -0.5).to(BF).to(device)
        entries.append((down, up, (1.0, 0.5, 2.0)[i % 3]))
    return base, entries


def bound_ratio(got, base, entries):
    """Largest |got - truth| / bound over the elements, truth in float64 on the bf16 operands ``merged_weight`` uses:

        bound = 1/2 ulp_bf16(bf16(truth)) + (R + 2) 2^-24 (|base| + |bf16(s up)| |down|)

    one rounding, plus fp32 accumulation over the R (padded) terms and the base.  Also returns the share of elements that are
    not the correctly rounded truth."""
    from ltxmi import lora
    ups = [(u.float() * s).to(BF).to(F64) for _, u, s in entries]
    downs = [d.to(BF).to(F64) for d, _, _ in entries]
    up, down = torch.cat(ups, 1), torch.cat(downs, 0)
    R = (up.shape[1] + lora.RANK_PAD - 1) // lora.RANK_PAD * lora.RANK_PAD
    truth = base.to(F64) + up @ down
    mag = base.to(F64).abs() + up.abs() @ down.abs()
    rounded = truth.to(torch.float32).to(BF)
    exponent = torch.frexp(rounded.to(F64))[1]                        # |x| = m 2^e, m in [1/2, 1): ulp_bf16(x) = 2^(e - 8)
    ulp = torch.ldexp(torch.ones_like(truth), exponent - 8)
    bound = 0.5 * ulp + (R + 2) * 2.0 ** -24 * mag
    ratio = ((got.to(F64) - truth).abs() / bound).max().item()
    off = (got != rounded).double().mean().item()
    return ratio, off


def other_adapter_sd(model, paths, rank, seed, scale=0.5):
    """An adapter state dict for any linears of ``model`` by path, drawn as ``make_adapter_sd`` draws."""
    from ltxmi import lora
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for path in paths:
        n_out, n_in = lora._get(model, path).weight.shape
        sd[f"{path}.lora_A.weight"] = (torch.randn(rank, n_in, generator=g) * n_in ** -0.5).to(BF)
        sd[f"{path}.lora_B.weight"] = (torch.randn(n_out, rank, generator=g) * scale * rank ** -0.5).to(BF)
    return sd


def merged_state_dict(model_sd, adapters):
    """The state dict of a model (bf16 weights) with ``adapters`` = [(LoraAdapter, weight)] folded in by ``lora.merged_weight``,
    one call per linear with the entries of all adapters in order: what a model LOADED on merged weights carries."""
    from ltxmi import lora
    out = {k: v.clone() for k, v in model_sd.items()}
    paths = list(dict.fromkeys(p for ad, _ in adapters for p in ad.modules))
    for path in paths:
        entries = [(ad.modules[path][0], ad.modules[path][1], ad.scale(path, w)) for ad, w in adapters if path in ad.modules]
        out[path + ".weight"] = lora.merged_weight(model_sd[path + ".weight"].detach(), entries)
    return out


def _two(cfg):
    from ltxmi import loading
    return loading.load_lora(make_adapter_sd(cfg, 16, seed=5)), loading.load_lora(make_adapter_sd(cfg, 64, seed=6, alpha=32.0))


def _weights(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def case_witness():
    """One rounding, from an fp32 sum that includes the base: by ``merged_weight``, and for two separately fused adapters."""
    from ltxmi import lora
    ltxmi, cfg, sd, m, forward, _ = setup()
    base, down, up = witness_operands()
    got = lora.merged_weight(base, [(down, up, 1.0)])
    assert got.dtype == BF and got.shape == base.shape and bool((got.float() == WITNESS).all()), got.float().unique()
    assert bool((base == 1).all())
    # the forms that round twice, in torch: both give 1.0
    delta = (up.float() @ down.float()).to(BF)
    assert bool(((base.float() + delta.float()).to(BF) == 1).all())
    step = (base.float() + up[:, :1].float() @ down[:1].float()).to(BF)
    assert bool(((step.float() + up[:, 1:].float() @ down[1:].float()).to(BF) == 1).all())
    # the components as two adapters fused one after the other on one linear: still one rounding for both
    path = "transformer_blocks.0.attn1.to_q"
    w = m.transformer_blocks[0].attn1.to_q.weight
    with torch.no_grad():
        w.fill_(1.0)
    a, b = witness_adapters(path)
    m.fuse_lora(a, name="a")
    assert bool((w == 1).all()), "2^-8 alone is a tie: rounds to even"
    m.fuse_lora(b, name="b")
    assert bool((w.float() == WITNESS).all()), w.float().unique()
    m.unfuse_lora("a")
    assert bool((w == 1).all())
    m.unfuse_lora()
    assert bool((w == 1).all()) and m.fused_lora_names() == []


def case_bound():
    """``merged_weight`` against float64 within the derived per-element bound, N_out = K_in = 512, R = 128; the padded ranks
    16 + 64 + 100 and a K_in that is no multiple of 8 too; ``out`` aliasing the base gives the same bits."""
    from ltxmi import lora
    setup()
    for n_out, k_in, ranks in ((512, 512, (128,)), (512, 256, (16, 64, 100)), (136, 260, (16,))):
        base, entries = drawn_operands(n_out, k_in, ranks, seed=n_out + k_in)
        got = lora.merged_weight(base, entries)
        ratio, off = bound_ratio(got, base, entries)
        print(f"merged_weight {(n_out, k_in, ranks)}: largest |got - truth| / bound {ratio:.3f}, not correctly rounded {off:.1e}")
        assert ratio <= 1.0, ratio
        alias = base.clone()
        assert lora.merged_weight(alias, entries, out=alias) is alias and torch.equal(alias, got)
    try:
        # a row stride of 130 elements: the residual's leading dimension is no multiple of 4
        lora.merged_weight(torch.zeros(128, 130, dtype=BF)[:, :128], [(torch.zeros(16, 128, dtype=BF), torch.zeros(128, 16, dtype=BF), 1.0)],
                           what="some.linear")
    except ValueError as e:
        assert "some.linear" in str(e), e
    else:
        raise AssertionError("a leading dimension the GEMM refuses was taken")


def case_bit_identity():
    """After ``fuse_lora`` the forward is that of a second model LOADED on the ``merged_weight`` results, bit for bit, plain and
    mixed -- with a forward before the fuse, so that the packs and the text K/V caches of the base weights exist then."""
    ltxmi, cfg, sd, m, forward, _ = setup()
    a, b = _two(cfg)
    base_w = _weights(m)
    base, base_mixed = forward(), forward(mixed=True)
    assert m.transformer_blocks[0].attn2.derived_slots(), "no pack / text K/V cache exists before the fuse"
    params = {k: (p, p.data_ptr(), p._version) for k, p in m.named_parameters()}
    m.fuse_lora(a, weight=0.5, name="a")
    m.fuse_lora(b, weight=2.0, name="b")
    for k, (p, ptr, ver) in params.items():
        q = dict(m.named_parameters())[k]
        assert q is p and q.data_ptr() == ptr, k
        if k.endswith(".weight") and k[:-7] in a.modules:
            assert q._version > ver, f"{k}: the version counter did not move"
    assert all(blk.attn1.__dict__.get("_lora") is None and blk.ff.__dict__.get("_lora") is None for blk in m.transformer_blocks)
    out, out_mixed = forward(), forward(mixed=True)
    assert rel(out, base) > 1e-2 and rel(out_mixed, base_mixed) > 1e-2, "stale packs or text K/V: the fuse did nothing"
    sd2 = merged_state_dict(base_w, [(a, 0.5), (b, 2.0)])
    assert _same(_weights(m), sd2)
    m2 = ltxmi.Transformer3DModel(**cfg)
    m2.load_state_dict(sd2)
    m2 = m2.to(BF).eval()
    assert torch.equal(forward(model=m2), out) and torch.equal(forward(model=m2, mixed=True), out_mixed)


def case_lifecycle():
    from ltxmi import loading
    ltxmi, cfg, sd, m, forward, _ = setup()
    a, b = _two(cfg)
    base_w, base, n_buffers = _weights(m), forward(), len(list(m.buffers()))
    m.fuse_lora(b, weight=2.0, name="b")
    only_b_w, only_b = _weights(m), forward()
    m.unfuse_lora()
    assert _same(_weights(m), base_w) and torch.equal(forward(), base) and m.fused_lora_names() == []
    assert "_lora_fused" not in m.__dict__, "the record outlives the last adapter"
    # unfuse one of two: what remains is a fresh fuse of the other
    m.fuse_lora(a, weight=0.5, name="a")
    m.fuse_lora(b, weight=2.0, name="b")
    assert m.fused_lora_names() == ["a", "b"] and m.lora_names() == []
    both_w = _weights(m)
    m.unfuse_lora("a")
    assert m.fused_lora_names() == ["b"] and _same(_weights(m), only_b_w) and torch.equal(forward(), only_b)
    # set_fused_lora_weights is a fresh fuse at those strengths
    m.set_fused_lora_weights({"b": 0.75})
    assert not _same(_weights(m), only_b_w)
    m.set_fused_lora_weights({"b": 2.0})
    assert _same(_weights(m), only_b_w)
    m.unfuse_lora()
    m.fuse_lora(a, weight=1.5, name="a")
    m.fuse_lora(b, weight=0.25, name="b")
    m.set_fused_lora_weights({"a": 0.5, "b": 2.0})
    assert _same(_weights(m), both_w)
    # the state dict is the fused weights and nothing else; the base copies are neither parameters nor buffers
    st = m.__dict__["_lora_fused"]
    assert set(st.base) == set(a.modules) and all(t.dtype == BF for t in st.base.values())
    assert m.state_dict().keys() == base_w.keys() and len(list(m.buffers())) == n_buffers
    assert "_lora_adapters" not in m.__dict__ and "_lora_epoch" not in m.__dict__
    try:
        m.load_state_dict(base_w)
    except RuntimeError as e:
        assert "unfuse_lora() first" in str(e)
    else:
        raise AssertionError("load_state_dict on a fused model did not raise")
    for bad in (lambda: m.unfuse_lora("x"), lambda: m.set_fused_lora_weights({"x": 1.0})):
        try:
            bad()
        except KeyError:
            pass
        else:
            raise AssertionError("an unknown name was accepted")
    try:
        m.fuse_lora(a, name="a")
    except ValueError as e:
        assert "fused already" in str(e)
    else:
        raise AssertionError("a second adapter of one name was accepted")
    # the base copies follow .to(): both round trips leave them usable
    m.to(BF)
    m.float()
    assert all(t.dtype == torch.float32 for t in st.base.values())
    m.to(BF)
    assert _same(_weights(m), both_w)
    m.unfuse_lora("a")
    assert _same(_weights(m), only_b_w)
    m.unfuse_lora()
    assert _same(_weights(m), base_w) and torch.equal(forward(), base)
    # keep_base=False: merged in place, the same bits, nothing kept, and no way back
    part = loading.load_lora(make_adapter_sd(cfg, 16, seed=6, targets=("attn1.to_k", "ff.net.2"), blocks=[1]))
    m.fuse_lora(b, weight=2.0, name="b", keep_base=False)
    assert _same(_weights(m), only_b_w) and m.fused_lora_names() == ["b"] and not m.__dict__["_lora_fused"].base
    for bad in (lambda: m.unfuse_lora(), lambda: m.unfuse_lora("b"), lambda: m.set_fused_lora_weights({"b": 1.0}),
                lambda: m.fuse_lora(part, name="part")):
        try:
            bad()
        except RuntimeError as e:
            assert "keep_base=False" in str(e), e
        else:
            raise AssertionError("a keep_base=False merge was taken back")
    assert _same(_weights(m), only_b_w) and m.fused_lora_names() == ["b"]


def case_non_block():
    """An adapter that names proj_out and adaln_single.linear as well as block linears: ``attach_lora(strict=True)`` still raises,
    ``fuse_lora`` takes it; parity with oracle/dit.py in float64 on merged weights at the bound of lora_cpu_cases.case_oracle."""
    from ltxmi import loading
    ltxmi, cfg, sd, m, forward, oracle = setup()
    e_base = rel(forward(), oracle(merged(sd, [])))
    base_w = _weights(m)
    ad_sd = dict(make_adapter_sd(cfg, 16, seed=5), **other_adapter_sd(m, ("proj_out", "adaln_single.linear", "patchify_proj",
                                                                          "caption_projection.linear_2"), 16, seed=8))
    ad = loading.load_lora(ad_sd)
    try:
        m.attach_lora(ad)
    except ValueError as e:
        assert "adaln_single.linear" in str(e) and "proj_out" in str(e)
    else:
        raise AssertionError("attach_lora(strict=True) took linears outside the blocks")
    m.fuse_lora(ad, weight=1.0, name="all")
    assert m.lora_names() == [] and m.fused_lora_names() == ["all"]
    for path in ("proj_out", "adaln_single.linear", "patchify_proj", "caption_projection.linear_2"):
        assert not torch.equal(m.state_dict()[path + ".weight"], base_w[path + ".weight"]), path
    truth = oracle(merged(sd, [(ad, 1.0)]))
    e = rel(forward(), truth)
    moved = rel(truth, oracle(merged(sd, [])))
    print(f"rel L2 vs float64 merged oracle: fused {e:.3e}, no adapter {e_base:.3e}; the adapter moves the output by {moved:.3e}")
    assert moved > 5e-2, "the adapter is too weak to test anything"
    assert e < 2e-2 and e < 2 * e_base + 1e-3, (e, e_base)
    e_mixed = rel(forward(mixed=True), truth)
    print(f"mixed=True: {e_mixed:.3e}")
    assert e_mixed < 2e-2
    # the errors attach_lora raises for a path or a shape that does not fit
    for bad_sd, exc in ((make_adapter_sd(cfg, 16, seed=1, blocks=[2]), KeyError),
                        (dict(ad_sd, **{"proj_out.lora_A.weight": torch.zeros(16, 256, dtype=BF)}), ValueError)):
        try:
            m.fuse_lora(loading.load_lora(bad_sd), name="bad")
        except exc:
            pass
        else:
            raise AssertionError("fuse_lora took an adapter that does not fit")
    assert m.fused_lora_names() == ["all"]
    m.unfuse_lora()
    assert _same(_weights(m), base_w)


def case_fused_plus_attached():
    """``fuse_lora(a)`` + ``attach_lora(b)``: b runs unmerged on top of the fused weights; against the oracle on both merged."""
    ltxmi, cfg, sd, m, forward, oracle = setup()
    a, b = _two(cfg)
    e_base = rel(forward(), oracle(merged(sd, [])))
    m.fuse_lora(a, weight=0.5, name="a")
    fused_only = forward()
    m.attach_lora(b, weight=2.0, name="b")
    assert m.fused_lora_names() == ["a"] and m.lora_names() == ["b"]
    truth = oracle(merged(sd, [(a, 0.5), (b, 2.0)]))
    out = forward()
    e = rel(out, truth)
    print(f"rel L2 vs float64 merged oracle: fused a + attached b {e:.3e}, no adapter {e_base:.3e}")
    assert rel(out, fused_only) > 1e-2
    assert e < 2e-2 and e < 2 * e_base + 1e-3, (e, e_base)
    assert rel(forward(mixed=True), truth) < 2e-2
    m.detach_lora()
    assert m.fused_lora_names() == ["a"] and m.lora_names() == [] and torch.equal(forward(), fused_only)
    ep = m.__dict__["_lora_epoch"]
    m.set_fused_lora_weights({"a": 1.0})
    m.unfuse_lora()
    assert m.__dict__["_lora_epoch"] == ep, "the adapter epoch belongs to the attached adapters"


CASES = {"witness": case_witness, "bound": case_bound, "bit_identity": case_bit_identity, "lifecycle": case_lifecycle,
         "non_block": case_non_block, "fused_plus_attached": case_fused_plus_attached}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
