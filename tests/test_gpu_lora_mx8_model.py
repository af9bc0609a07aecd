"""``attach_lora(..., mx8=True)`` on a quantised model, on a real MI355X: adapters on linears that run in MX-FP8 are MX-FP8 operand
pairs of the linear's own GEMM (ltxmi/lora.py ``pair_mx8``, include/ltxmi_mx_lora.h).

Cases of tests/test_gpu_mx8_model.py (2b, 2b mixed, 13b), each with ``quantize_ff()`` and ``quantize_attention(linears=all four)``
and adapters of rank 16 and 128 together on all ten block linears (tests/lora_cpu_cases.py, as tests/test_gpu_lora.py builds
them).  Truth: ``oracle/dit.py`` in float64 (tests/mixed_oracle.py for mixed) with ``leaves`` patched for the format as
tests/test_gpu_mx8_model.py and tests/test_gpu_attn_mx8_model.py patch it AND for the adapter: on a quantised linear
``y = lin(qdq(x), qdq(W)) + lin(qdq(T), qdq(bf16(s up)))`` with ``T = lin(qdq(x), qdq(down))``, the adapters of a linear stacked
along r and padded with zeros to a multiple of 128 as the product stacks them, T quantised from its high-precision value;
attn2.to_k / to_v, which stay bf16, get the unmerged formula of tests/test_gpu_lora.py.  Yardstick: the same patched oracle in
bf16.  ``assert_parity`` and ``RTOL`` of tests/test_gpu_model.py; the cap of the MX tests (format cost + the bf16 unmerged
model's error + RTOL) against the unpatched oracle on merged weights ``W + s B A``, printed."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_attn_mx8_model import LINEARS, ORACLE_PATHS, _patch
from test_gpu_lora import _adapters, _merged32
from test_gpu_model import BF, DEV, RTOL, assert_parity, rel
from test_gpu_mx8_model import _CASES, _case, _forward, _oracle, _qdq

pytestmark = pytest.mark.gpu

SPECS = [(16, 5, None, 0.5), (128, 6, 32.0, 2.0)]          # (rank, seed, alpha, weight)
MX_ENDS = tuple(e for n in LINEARS for e in ORACLE_PATHS[n]) + ("ff.net.0.proj.", "ff.net.2.")
QUANTISED_LINEARS = 6                                      # per block: qkv, attn1.to_out, attn2.to_q, attn2.to_out, FF1, FF2


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _CASES.clear()


def _patch_adapters(mp, adapters):
    """On top of the format's patches: the adapter term of every linear the adapters name."""
    from oracle import leaves
    table = {}
    for ad, weight in adapters:
        for path, (down, up, _) in ad.modules.items():
            table.setdefault(path, []).append((down.to(DEV), up.to(DEV), ad.scale(path, weight)))
    stacked = {}

    def operands(p, dt):
        if (p, dt) not in stacked:
            downs = torch.cat([d.to(BF) for d, _, _ in table[p]], 0)
            ups = torch.cat([(u.float() * s).to(BF) for _, u, s in table[p]], 1)
            R = (downs.shape[0] + 127) // 128 * 128
            down = torch.zeros((R, downs.shape[1]), dtype=dt, device=DEV)
            down[:downs.shape[0]] = downs.to(dt)
            up = torch.zeros((ups.shape[0], R), dtype=dt, device=DEV)
            up[:, :ups.shape[1]] = ups.to(dt)
            stacked[(p, dt)] = (_qdq(down), _qdq(up))
        return stacked[(p, dt)]

    base = leaves.linear

    def linear(x, sd, p):
        y = base(x, sd, p)
        if p[:-1] not in table:
            return y
        if p.endswith(MX_ENDS):
            down, up = operands(p[:-1], x.dtype)
            return y + F.linear(_qdq(F.linear(_qdq(x), down)), up)
        for down, up, s in table[p[:-1]]:                  # attn2.to_k / to_v: bf16, unmerged (tests/test_gpu_lora.py)
            y = y + s * F.linear(F.linear(x, down.to(x.dtype)), up.to(x.dtype))
        return y

    mp.setattr(leaves, "linear", linear)


def _quantise(m, keep_bf16=True):
    m.quantize_attention(linears=LINEARS, keep_bf16=keep_bf16)
    m.quantize_ff(keep_bf16=keep_bf16)


def _restore(m):
    m.detach_lora()
    if m.attention_quantized:
        m.unquantize_attention()
    if m.ff_quantized:
        m.unquantize_ff()


@pytest.mark.parametrize("name,mixed", [("2b", False), ("2b", True), ("13b", False)])
def test_mx8_adapters_against_the_patched_oracle(name, mixed, monkeypatch):
    from ltxmi import ops
    c = _case(name)
    m = c["m"]
    layers = len(m.transformer_blocks)
    adapters = _adapters(c["cfg"], SPECS)
    hi = torch.float32 if mixed else torch.float64
    merged = dict(c, sd32=_merged32(c["sd32"], adapters))
    plain_hi, plain32 = _oracle(merged, hi, mixed), _oracle(merged, torch.float32, mixed)
    with monkeypatch.context() as mp:
        _patch(mp, ff=True)
        _patch_adapters(mp, adapters)
        truth, eager = _oracle(c, hi, mixed), _oracle(c, BF, mixed)
    try:
        for i, (ad, w) in enumerate(adapters):
            m.attach_lora(ad, weight=w, name=f"a{i}")
        bf16_unmerged = _forward(c, mixed)
        m.detach_lora()
        _quantise(m)
        q_base = _forward(c, mixed)
        launches = []
        real = ops.gemm_mx8
        ops.gemm_mx8 = lambda *a, **k: (launches.append("a2" in k), real(*a, **k))[1]
        try:
            _forward(c, mixed)
            assert len(launches) == QUANTISED_LINEARS * layers and not any(launches), launches
            for i, (ad, w) in enumerate(adapters):
                with pytest.raises(RuntimeError, match=r"unquantize_(ff|attention)\(\) first"):
                    m.attach_lora(ad, weight=w)
                m.attach_lora(ad, weight=w, name=f"a{i}", mx8=True)
            assert m.lora_names() == ["a0", "a1"]
            del launches[:]
            out = _forward(c, mixed)
            # twice per quantised linear: the down GEMM (MX output) and the linear's own call with the pair
            assert len(launches) == 2 * QUANTISED_LINEARS * layers and sum(launches) == QUANTISED_LINEARS * layers, launches
        finally:
            ops.gemm_mx8 = real
        what = f"{name}{' mixed' if mixed else ''}, r16 + r128 as MX-FP8 pairs on a quantised model"
        assert rel(out, q_base) > 1e-3, "the adapters did nothing"
        assert_parity(out, truth, eager, what)
        format_cost, bf16_err, ours = rel(truth, plain_hi), rel(bf16_unmerged, plain32), rel(out, plain32)
        print(f"{what}: precision cost: rel L2 against the UNPATCHED fp32 oracle on merged weights {ours:.3e} (the bf16 unmerged "
              f"model {bf16_err:.3e}; the format alone, patched against unpatched oracle, {format_cost:.3e}); "
              f"cap {format_cost + bf16_err + RTOL:.3e}")
        assert ours <= format_cost + bf16_err + RTOL
        assert torch.equal(_forward(c, mixed), out), "two forwards differ"
        m.set_lora_weights({"a1": 0.5})
        assert rel(_forward(c, mixed), out) > 1e-4, "set_lora_weights did nothing"
        m.set_lora_weights({"a1": SPECS[1][3]})
        assert torch.equal(_forward(c, mixed), out), "set_lora_weights back does not give the first bits"
        m.detach_lora()
        assert torch.equal(_forward(c, mixed), q_base), "detach_lora() does not restore the quantised model's bits"
    finally:
        _restore(m)


def test_zero_up_adapter_changes_no_bit_and_unquantize_rebuilds_bf16_pairs():
    from ltxmi import loading, lora
    import lora_cpu_cases as cases
    c = _case("2b")
    m = c["m"]
    adapters = _adapters(c["cfg"], SPECS)
    try:
        for i, (ad, w) in enumerate(adapters):
            m.attach_lora(ad, weight=w, name=f"a{i}")
        bf16_unmerged = _forward(c)
        m.detach_lora()
        _quantise(m)
        q_base = _forward(c)
        sd = {k: (torch.zeros_like(v) if ".lora_B." in k else v) for k, v in cases.make_adapter_sd(c["cfg"], 64, seed=9).items()}
        m.attach_lora(loading.load_lora(sd), mx8=True)
        slots = m.transformer_blocks[0].attn1.__dict__["_lora"]
        assert isinstance(slots["qkv"], lora.LoraSlotMx8) and slots["qkv"].down[0].shape[0] == 3 * 128
        assert isinstance(m.transformer_blocks[0].attn2.__dict__["_lora"]["kv"], lora.LoraSlot)
        assert torch.equal(_forward(c), q_base), "a zero-up adapter changes bits"
        m.detach_lora()
        # unquantize_* with mx8 adapters attached: the slots become bf16 ones, the model the unquantised model with adapters
        for i, (ad, w) in enumerate(adapters):
            m.attach_lora(ad, weight=w, name=f"a{i}", mx8=True)
        m.unquantize_attention()
        m.unquantize_ff()
        assert all(isinstance(s, lora.LoraSlot) for o in (m.transformer_blocks[0].attn1, m.transformer_blocks[0].ff)
                   for s in o.__dict__["_lora"].values())
        assert torch.equal(_forward(c), bf16_unmerged), "not the unquantised model with the adapters attached"
    finally:
        _restore(m)


class _CountingLib:
    """Stands in for the library object ltxmi/ops.py reaches ltxmi_gemm_mx8_pair2 through: counts the calls of that entry itself."""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "ltxmi_gemm_mx8_pair2":
            return fn

        def entry(*a):
            self.calls += 1
            return fn(*a)
        return entry


def test_a_model_without_mx8_adapters_never_reaches_the_new_entry(monkeypatch):
    from ltxmi import _lib_mxl
    c = _case("2b")
    m = c["m"]
    adapters = _adapters(c["cfg"], SPECS[:1])
    counting = _CountingLib(_lib_mxl.lib)
    monkeypatch.setattr(_lib_mxl, "lib", counting)         # ops.py calls _lib_mxl.lib.ltxmi_gemm_mx8_pair2 at every launch
    try:
        _forward(c)
        m.attach_lora(adapters[0][0], name="a")            # bf16 adapters on an unquantised model
        _forward(c)
        m.detach_lora()
        _quantise(m)
        q_base = _forward(c)
        assert counting.calls == 0
        m.attach_lora(adapters[0][0], name="a", mx8=True)  # ... and the count does see the entry when it is reached
        assert rel(_forward(c), q_base) > 1e-4
        assert counting.calls == QUANTISED_LINEARS * len(m.transformer_blocks)
    finally:
        _restore(m)


def test_keep_bf16_false_takes_mx8_adapters_and_gives_the_same_bits():
    c = _case("2b")
    m = c["m"]
    adapters = _adapters(c["cfg"], SPECS)
    try:
        _quantise(m)
        for i, (ad, w) in enumerate(adapters):
            m.attach_lora(ad, weight=w, name=f"a{i}", mx8=True)
        out = _forward(c)
        _restore(m)
        _quantise(m, keep_bf16=False)
        assert m.transformer_blocks[0].ff.net[2].weight.numel() == 0 and m.transformer_blocks[0].attn1.to_q.weight.numel() == 0
        for i, (ad, w) in enumerate(adapters):
            m.attach_lora(ad, weight=w, name=f"a{i}", mx8=True)
        assert torch.equal(_forward(c), out), "keep_bf16=False then attach_lora(mx8=True) differs from the keep_bf16=True run"
        m.set_lora_weights({"a0": 0.25})
        assert rel(_forward(c), out) > 1e-4
    finally:
        _CASES.clear()                                       # this model cannot be given back
