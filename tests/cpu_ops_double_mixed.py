"""CPU stand-ins for the two row kernels of the fp32 residual stream -- TEST INFRASTRUCTURE ONLY.

Installed on top of tests/cpu_ops_double.py (``install()`` here calls that one first): ``ops.norm_modulate_f32in`` and
``ops.gate_residual_f32_`` with the kernels' argument meaning and their rounding points (include/ltxmi.h, 0.8), so that the
mixed-precision host logic of ``Transformer3DModel`` / ``BasicTransformerBlock`` / ``LTXVideoPipeline`` runs on the CPU."""
import torch

import cpu_ops_double
from cpu_ops_double import _rows

BF16 = torch.bfloat16


def _gate(table, temb, rows_per_group, rows):
    return table.float()[None] + temb.float().repeat_interleave(rows_per_group, dim=0)[:rows]


def norm_modulate_f32in(x, out, eps, kind, scale_table, scale_temb, shift_table, shift_temb, rows_per_group):
    assert x.dtype == torch.float32 and out.dtype == BF16, (x.dtype, out.dtype)
    assert x.data_ptr() != out.data_ptr()
    # the bf16 double computes in fp32 from whatever it is given and rounds once at the store: the same arithmetic
    return cpu_ops_double.norm_modulate(x, out, eps, kind, scale_table, scale_temb, shift_table, shift_temb, rows_per_group)


def gate_residual_f32_(h, y, gate_table=None, gate_temb=None, rows_per_group=1, round_product=0, h_bf16=None):
    assert h.dtype == torch.float32 and y.dtype == BF16, (h.dtype, y.dtype)
    assert (gate_table is None) == (gate_temb is None)
    h2, y2 = _rows(h), _rows(y)
    rows = h2.shape[0]
    p = y2.float()
    if gate_table is not None:
        p = _gate(gate_table, gate_temb, rows_per_group, rows) * p
        if round_product:
            p = p.to(BF16).float()
    h2.add_(p)
    if h_bf16 is not None:
        assert h_bf16.dtype == BF16
        _rows(h_bf16).copy_(h2.to(BF16))
    return h


NAMES = ["norm_modulate_f32in", "gate_residual_f32_"]


def install():
    """cpu_ops_double.install() + the two functions above (this process only)."""
    ops = cpu_ops_double.install()
    for n in NAMES:
        setattr(ops, n, globals()[n])
    return ops
