"""ltxmi/derived.py: the keyed cache by itself, every module that packs weights through it, and the two step-invariant
sites of the DiT on the CPU doubles (tests/derived_cache_cases.py, each case in a process of its own)."""
import gc
import importlib.util
import os
import subprocess
import sys
import weakref

import pytest
import torch

import derived_cache_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the helper alone
@pytest.fixture(scope="module")
def derived():
    """derived.py loaded as a file: neither the package's __init__ nor the library is touched."""
    spec = importlib.util.spec_from_file_location("derived_alone", os.path.join(ROOT, "ltx-video-gpupoor_amd", "ltxmi", "derived.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src = open(spec.origin).read()
    assert "import ops" not in src and "_lib" not in src
    return mod


class _Counting:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return object()


def test_helper_hits_misses_and_what_it_cannot_see(derived):
    cache, build = derived.DerivedCache(), _Counting()
    a, b = torch.zeros(4), torch.zeros(4)
    v = cache.get((a, b, None), ("slot",), build)
    assert cache.get((a, b, None), ("slot",), build) is v and build.n == 1
    for i, t in enumerate((a, b)):                                   # an in-place edit of any ONE source
        t.add_(1)
        v2 = cache.get((a, b, None), ("slot",), build)
        assert v2 is not v and build.n == 2 + i
        v = v2
    assert cache.get((a, b, None), ("other",), build) is not v and build.n == 4      # an extra is part of the key
    v = cache.get((a, b, None), ("other",), build)
    a.data.add_(1)                                                   # no version counter moves: not seen ...
    assert cache.get((a, b, None), ("other",), build) is v and build.n == 4
    cache.clear()                                                    # ... until the cache is cleared
    assert len(cache) == 0 and cache.get((a, b, None), ("other",), build) is not v and build.n == 5


def test_helper_takes_inference_tensors(derived):
    cache, build = derived.DerivedCache(), _Counting()
    with torch.inference_mode():
        t = torch.zeros(4)
    assert t.is_inference() and derived.tensor_version(t) == -1 and derived.tensor_version(torch.zeros(4)) == 0
    v = cache.get((t,), (), build)
    assert cache.get((t,), (), build) is v and build.n == 1


def test_helper_tells_views_of_one_storage_apart(derived):
    """Same address, another dtype, shape or stride: each is a key of its own."""
    base = torch.zeros(8)
    views = [base[:4], base.view(torch.int32)[:4], base[:2], base[::2], base[:4].view(2, 2)]
    assert len({v.data_ptr() for v in views}) == 1
    cache, build = derived.DerivedCache(8), _Counting()
    values = [cache.get((v,), (), build) for v in views]
    assert build.n == len(views) == len(cache) and len({id(v) for v in values}) == len(views)
    assert [cache.get((v,), (), build) for v in views] == values and build.n == len(views)
    # layout=False (sources whose shape and stride cannot change at one address) leaves those two out, and only those
    plain = derived.DerivedCache(8, layout=False)
    assert plain.get((views[0],), (), build) is plain.get((views[2],), (), build) is plain.get((views[3],), (), build)
    assert plain.get((views[1],), (), build) is not plain.get((views[0],), (), build)


def test_helper_keeps_its_sources_alive(derived):
    cache, build = derived.DerivedCache(), _Counting()
    t = torch.zeros(4)
    ref = weakref.ref(t)
    cache.get((t,), (), build)
    del t
    gc.collect()
    assert ref() is not None                       # the address in the key cannot be handed to another tensor
    cache.clear()
    gc.collect()
    assert ref() is None


def test_helper_capacity_and_disabled(derived):
    cache, build = derived.DerivedCache(4), _Counting()
    ts = [torch.zeros(4) for _ in range(5)]
    for t in ts:
        cache.get((t,), (), build)
        assert len(cache) <= 4
    assert build.n == 5 and len(cache) == 1        # full means cleared: the fifth key is alone
    off, build = derived.DerivedCache(4), _Counting()
    a = off.get((ts[0],), (), build, enabled=False)
    assert off.get((ts[0],), (), build, enabled=False) is not a and build.n == 2 and len(off) == 0


# ------------------------------------------------------------------------------------------------- every pack site
T5_TINY = dict(d_model=128, d_kv=64, d_ff=256, num_heads=2, num_layers=1, vocab_size=32)


def _attention(cross):
    from ltxmi.attention import Attention
    m = Attention(query_dim=128, cross_attention_dim=128 if cross else None, heads=2, dim_head=64, bias=True, qk_norm="rms_norm")
    mods = [m.to_k, m.to_v] if cross else [m.to_q, m.to_k, m.to_v]
    return m, (m.packed_kv if cross else m.packed_qkv), lambda: [t for l in mods for t in (l.weight, l.bias)]


def _t5(which):
    from ltxmi import t5
    cfg = t5.T5Config(T5_TINY)
    if which == "qkv":
        m = t5.T5Attention(cfg, False)
        names = ["q", "k", "v"]
    else:
        m = t5.T5DenseGatedActDense(cfg)
        names = ["wi_0", "wi_1"]
    return m, lambda: m._pack(which, [getattr(m, n) for n in names]), lambda: [getattr(m, n).weight for n in names]


def _causal_conv(d2s):
    from ltxmi.autoencoder import CausalConv3d
    m = CausalConv3d(64, 64)
    return m, lambda: m.packed(d2s), lambda: [m.conv.weight, m.conv.bias]


def _conv_params(dims, shuffle):
    from ltxmi.latent_upsampler import _ConvParams
    m = _ConvParams(64, 64, dims)
    return m, lambda: m.packed(shuffle), lambda: [m.weight, m.bias]


def _rel_bias():
    from ltxmi import t5
    m = t5.T5EncoderModel(T5_TINY)
    return m, lambda: m.rel_bias(8), lambda: [m.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight]


SITES = {"attention-qkv": lambda: _attention(False), "attention-kv": lambda: _attention(True),
         "t5-qkv": lambda: _t5("qkv"), "t5-wi": lambda: _t5("wi"),
         "causalconv3d": lambda: _causal_conv(False), "causalconv3d-d2s": lambda: _causal_conv(True),
         "convparams-2d": lambda: _conv_params(2, 0), "convparams-2d-shuffle": lambda: _conv_params(2, 1),
         "convparams-3d": lambda: _conv_params(3, 0), "convparams-3d-shuffle": lambda: _conv_params(3, 1),
         "rel-bias-8": _rel_bias}


def _tensors(value):
    """The tensors of a site's value: a tensor, (weight, bias or None) or (table, center)."""
    return [t for t in (value if isinstance(value, tuple) else (value,)) if isinstance(t, torch.Tensor)]


def _same(a, b):
    return all(x is y for x, y in zip(_tensors(a), _tensors(b)))


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(_tensors(a), _tensors(b)))


@pytest.mark.parametrize("site", sorted(SITES))
def test_pack_site_follows_its_sources(site):
    torch.manual_seed(0)
    m, call, sources = SITES[site]()
    v = call()
    assert _same(call(), v)
    # an in-place edit of each source tensor on its own (weight and bias apart) rebuilds, to what a fresh build gives
    for i in range(len(sources())):
        with torch.no_grad():
            sources()[i].mul_(0.5)
        v2 = call()
        assert not _same(v2, v) and not _equal(v2, v), (site, i)
        m.invalidate_packed()
        assert _equal(call(), v2), (site, i)
        v = call()
    # .to() and load_state_dict() invalidate by themselves (this cast moves no tensor: only the hook can tell)
    m.to(torch.float32)
    assert not _same(call(), v) and _equal(call(), v)
    v = call()
    m.load_state_dict(m.state_dict())
    assert not _same(call(), v) and _equal(call(), v)
    # an edit through .data is not seen until invalidate_packed()
    v = call()
    sources()[0].data.mul_(2.0)
    assert _same(call(), v)
    m.invalidate_packed()
    assert not _same(call(), v) and not _equal(call(), v)


def test_t5_share_packed_makes_the_members_views_of_the_operand():
    for which in ("qkv", "wi"):
        m, call, sources = _t5(which)
        before = torch.cat([w.detach().clone() for w in sources()])
        m.share_packed()
        operand = call()
        assert torch.equal(operand, before)
        offset = 0
        for w in sources():                                        # the members' weights are the operand's row blocks ...
            assert w.data_ptr() == operand.data_ptr() + offset
            offset += w.numel() * w.element_size()
        assert offset == operand.numel() * operand.element_size()
        assert call() is operand                                   # ... and the operand is no copy of them
        m.invalidate_packed()
        assert call() is not operand and torch.equal(call(), operand)


# ------------------------------------------------------------------------------------------------- the step-invariant sites
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_step_invariant_sites_on_the_cpu_doubles(case):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "derived_cache_cases.py"), case], capture_output=True,
                       text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
