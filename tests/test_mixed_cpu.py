"""mixed_precision (the fp32 residual stream) without a GPU: the plain-torch restatement of the reference's ``mixed=True``
data flow against the reference's own output (G16), the product's host logic on CPU doubles of the two new row kernels,
the pipeline's handling of the flag, and the argument checks of the two new entry points."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import mixed_kernel_cases as mk
import mixed_oracle
import norm_cases as nc
from oracle import dit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-5, atol=2e-6)   # fp32 vs fp32, as tests/test_oracle_golden.py
BF = torch.bfloat16
STRATEGIES = {"AttentionValues": dit.ATTENTION_VALUES, "AttentionSkip": dit.ATTENTION_SKIP, "Residual": dit.RESIDUAL,
              "TransformerBlock": dit.TRANSFORMER_BLOCK}


@pytest.fixture(scope="module")
def g16():
    from mixed_cpu_cases import load_g16
    return load_g16()


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


CASE_NAMES = ["L2.sample", "L2.token", "L8.sample", "L4.AttentionValues", "L4.AttentionSkip", "L4.Residual", "L4.TransformerBlock"]


def test_g16_holds_the_cases_the_tests_name(g16):
    t, meta = g16
    assert [c["name"] for c in meta["cases"]] == CASE_NAMES
    assert meta["skip_blocks"] == [1, 2] and torch.equal(t["skip_layer_mask"][:, 2], torch.tensor([1.0, 0.0, 0.0, 1.0]))
    assert all(t[n + ".mixed"].dtype == BF and t[n + ".fp32"].dtype == torch.float32 for n in CASE_NAMES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_g16_mixed_oracle_against_the_reference(g16, name):
    """tests/mixed_oracle.py against the reference's own ``forward(mixed=True)`` under CPU autocast, on the conditions
    ``test_g5_transformer_bf16_twin`` applies to the bf16 twin; run in fp32 it is the reference's fp32 forward."""
    from mixed_cpu_cases import g16_state_dict
    t, meta = g16
    case = next(c for c in meta["cases"] if c["name"] == name)
    cfg = dict(meta["cfg"], num_layers=case["layers"])
    sd32 = g16_state_dict(t, meta, case["layers"])
    kw = {}
    if case["strategy"] is not None:
        skip = dit.create_skip_layer_mask(case["layers"], 1, 3, 2, meta["skip_blocks"], torch.float32)
        torch.testing.assert_close(skip, t["skip_layer_mask"], rtol=0, atol=0)
        kw = dict(skip_layer_mask=skip, skip_layer_strategy=STRATEGIES[case["strategy"]])
    ts = t["ts_tok"] if case["per_token"] else t["ts"]
    truth, out = mixed_oracle.oracles(sd32, cfg, t["x"], t["enc"], t["mask"], ts, t["indices_grid"], tuple(meta["grid"]), **kw)
    assert out.dtype == BF
    torch.testing.assert_close(truth, t[name + ".fp32"], **TOL)
    ref = t[name + ".mixed"].float()
    err = _rel(out, ref)
    e_ref, e_orc = _rel(ref, t[name + ".fp32"]), _rel(out, t[name + ".fp32"])
    print(f"{name}: oracle vs reference {err:.3e}; vs fp32: oracle {e_orc:.3e}, reference {e_ref:.3e}, "
          f"plain bf16 reference {_rel(t[name + '.bf16'], t[name + '.fp32']):.3e}")
    assert err < 1e-2, err
    assert e_orc < 2 * e_ref + 1e-3, (e_orc, e_ref)


def test_mixed_oracle_in_fp32_is_the_plain_fp32_oracle(g16):
    """With every cast a no-op the restatement IS oracle.dit's forward: the rounding points are all that it adds."""
    from mixed_cpu_cases import g16_state_dict
    t, meta = g16
    cfg = dict(meta["cfg"], num_layers=4)
    sd32 = g16_state_dict(t, meta, 4)
    skip = dit.create_skip_layer_mask(4, 1, 3, 2, [1, 2], torch.float32)
    fc = dit.precompute_freqs_cis(t["indices_grid"], cfg, torch.float32)
    for code in STRATEGIES.values():
        kw = dict(encoder_attention_mask=t["mask"], latent_shape=tuple(meta["grid"]), skip_layer_mask=skip, skip_layer_strategy=code)
        a = mixed_oracle.transformer3d_forward_mixed(sd32, cfg, t["x"], fc, t["enc"], t["ts_tok"], torch.float32, **kw)
        b = dit.transformer3d_forward(sd32, cfg, t["x"], fc, t["enc"], t["ts_tok"], **kw)
        torch.testing.assert_close(a, b, **TOL)


@pytest.mark.parametrize("case", ["model", "rounding_points", "bf16_untouched", "pipeline"])
def test_host_logic_on_the_cpu_doubles(case):
    """tests/mixed_cpu_cases.py in a process of its own (the doubles replace functions of ``ltxmi.ops`` process-wide)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mixed_cpu_cases.py"), case], capture_output=True,
                       text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


def test_sequence_parallel_refuses_the_fp32_stream():
    import ltxmi
    from ltxmi import distributed as sp
    with pytest.raises(NotImplementedError, match="fp32 residual stream"):
        sp.usp_dit_forward(None, torch.zeros(1, 8, 16), (None, None), mixed=True)
    for proc in (sp.UlyssesAttnProcessor(), sp.RingAttnProcessor()):
        blk = ltxmi.attention.BasicTransformerBlock(128, 2, 64, cross_attention_dim=128, activation_fn="gelu-approximate",
                                                    attention_bias=True, norm_elementwise_affine=False, qk_norm="rms_norm",
                                                    standardization_norm="rms_norm", use_rope=True).to(BF)
        blk.attn1.set_processor(proc)
        with pytest.raises(NotImplementedError, match="fp32 residual stream"):
            blk(torch.zeros(1, 8, 128), timestep=torch.zeros(1, 1, 6 * 128, dtype=BF))


def test_ops_wrappers_refuse_cpu_and_wrong_dtypes():
    from ltxmi import ops
    h, y = torch.zeros(4, 64), torch.zeros(4, 64, dtype=BF)
    with pytest.raises(TypeError):
        ops.gate_residual_f32_(h, y)
    with pytest.raises(TypeError):
        ops.norm_modulate_f32in(h, y, 1e-6, ops.NORM_RMS, y[0], y, y[0], y, 1)


@pytest.mark.parametrize("rpg", mk.GROUPS)
@pytest.mark.parametrize("D", mk.WIDTHS)
@pytest.mark.parametrize("kind", mk.KINDS)
def test_kernel_case_bounds_hold_for_an_fp32_restatement_of_the_norm(kind, D, rpg):
    """The cases tests/test_gpu_mixed.py runs: the formula in fp32 with one rounding to bf16 meets the three metrics of
    tests/norm_cases.py on fp32 rows too, so the bound asks nothing of a kernel that fp32 arithmetic does not give."""
    out, truth, mag = mk.norm_restated(kind, D, rpg)
    f = nc.compare(out, truth, mag, what=f"restated norm_modulate_f32in {kind} D={D} rpg={rpg}")
    assert nc.excess(out, truth, mag) <= nc.MEASURED_EXCESS * 2, nc.excess(out, truth, mag)
    assert f["element"] <= 1


@pytest.mark.parametrize("D", mk.WIDTHS)
def test_kernel_case_bounds_hold_for_the_gate_pass(D):
    """The doubles of the gate pass on the GPU test's inputs: the rounded form IS the expected bits; a fused multiply-add
    (float64 product and sum, one rounding to fp32) meets the one-ulp bound, as does the ungated single addition; the cases
    separate the two forms."""
    import cpu_ops_double_mixed as dbl
    for rpg in mk.GROUPS:
        h, y, table, temb = mk.gate_case(D, rpg)
        g32 = mk.gate32(table, temb, rpg)
        want = mk.gate_rounded_expected(h, y, g32)
        got, hb = h.clone(), torch.empty(mk.ROWS, D, dtype=BF)
        dbl.gate_residual_f32_(got, y, table, temb, rpg, round_product=1, h_bf16=hb)
        assert torch.equal(got, want) and torch.equal(hb, want.to(BF))
        fused = (h.double() + g32.double() * y.double()).float()
        assert mk.gate_unrounded_check(fused, h, y, g32) <= 1.0
        assert not torch.equal(fused, want)
        with pytest.raises(AssertionError):
            mk.gate_unrounded_check(want, h, y, g32)                   # the bf16 rounding is far outside one fp32 ulp
        assert mk.gate_unrounded_check(h + y.float(), h, y, None) <= 1.0


def test_argument_validation_without_gpu():
    """The two new entry points refuse bad arguments before anything needs a device (status, then ltxmi_last_error)."""
    from ltxmi import _lib
    lib = _lib.lib
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) & ~63
    INVALID, UNSUPPORTED = -1, -2

    def norm(x=base, ldx=64, y=base + 4096, ldy=64, rows=4, D=64, kind=0, sc_t=base + 8192, sc_e=base + 8192, sh_t=base + 8192,
             sh_e=base + 8192, temb_ld=64, rpg=1):
        return lib.ltxmi_norm_modulate_f32in_bf16(x, ldx, y, ldy, rows, D, 1e-6, kind, sc_t, sc_e, sh_t, sh_e, temb_ld, rpg, None)

    def gate(h=base, ldh=64, y=base + 4096, ldy=64, rows=4, D=64, g_t=base + 8192, g_e=base + 8192, gate_ld=64, rpg=1, rnd=1,
             hb=base + 12288, ldhb=64):
        return lib.ltxmi_gate_residual_f32(h, ldh, y, ldy, rows, D, g_t, g_e, gate_ld, rpg, rnd, hb, ldhb, None)

    rows = [
        (norm(x=None), INVALID, b"NULL"), (norm(y=None), INVALID, b"NULL"), (norm(sc_e=None), INVALID, b"NULL"),
        (norm(sh_t=None), INVALID, b"NULL"), (norm(rows=0), INVALID, b"non-positive"), (norm(rpg=0), INVALID, b"non-positive"),
        (norm(rpg=-3), INVALID, b"non-positive"), (norm(kind=2), INVALID, b"kind"), (norm(y=base), INVALID, b"alias"),
        (norm(D=60), UNSUPPORTED, b"multiple of 8"), (norm(D=8200, ldx=8200, ldy=8200), UNSUPPORTED, b"8192"),
        (norm(ldx=66), UNSUPPORTED, b"strides"), (norm(ldy=68), UNSUPPORTED, b"strides"), (norm(ldx=56), UNSUPPORTED, b"strides"),
        (norm(temb_ld=4), UNSUPPORTED, b"strides"), (norm(x=base + 8), UNSUPPORTED, b"aligned"),
        (norm(sc_e=base + 8192 + 2), UNSUPPORTED, b"aligned"),
        (gate(h=None), INVALID, b"NULL"), (gate(y=None), INVALID, b"NULL"), (gate(rows=0), INVALID, b"non-positive"),
        (gate(D=0), INVALID, b"non-positive"), (gate(g_e=None), INVALID, b"gate_temb"), (gate(rpg=0), INVALID, b"rows_per_group"),
        (gate(rpg=-1), INVALID, b"rows_per_group"), (gate(rnd=2), INVALID, b"round_product"), (gate(hb=base), INVALID, b"different"),
        (gate(D=60), UNSUPPORTED, b"multiple of 8"), (gate(D=8200, ldh=8200, ldy=8200, ldhb=8200), UNSUPPORTED, b"8192"),
        (gate(ldh=66), UNSUPPORTED, b"strides"), (gate(ldy=60), UNSUPPORTED, b"strides"), (gate(ldhb=68), UNSUPPORTED, b"strides"),
        (gate(gate_ld=12), UNSUPPORTED, b"strides"), (gate(h=base + 4), UNSUPPORTED, b"aligned"),
        (gate(hb=base + 12288 + 8), UNSUPPORTED, b"aligned"), (gate(rows=1 << 30, D=64), UNSUPPORTED, b"too many"),
    ]
    # (each call above was followed by other calls: check the status here, the message in a second pass)
    for i, (status, want, _) in enumerate(rows):
        assert status == want, (i, status, want)
    for call, want, text in [(lambda: norm(D=60), UNSUPPORTED, b"multiple of 8"), (lambda: norm(rpg=0), INVALID, b"rows_per_group=0"),
                             (lambda: gate(g_e=None), INVALID, b"a gate_table needs gate_temb"),
                             (lambda: gate(D=8200, ldh=8200, ldy=8200, ldhb=8200), UNSUPPORTED, b"D=8200"),
                             (lambda: gate(h=None), INVALID, b"NULL")]:
        assert call() == want and text in lib.ltxmi_last_error(), lib.ltxmi_last_error()
    # what the ungated form ignores stays ignored: no gate_table -> gate_temb, gate_ld, rows_per_group, round_product are free
    assert lib.ltxmi_gate_residual_f32(base, 64, base + 4096, 64, 4, 60, None, None, 7, 0, 9, None, 0, None) == UNSUPPORTED
    assert b"multiple of 8" in lib.ltxmi_last_error()
