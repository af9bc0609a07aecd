"""Inputs and truths for the two row kernels of the fp32 residual stream -- TEST INFRASTRUCTURE ONLY (plain module, no GPU).

Shared by tests/test_mixed_cpu.py (the fp32 restatement meets the bounds: they come from the formats, not from a kernel)
and tests/test_gpu_mixed.py (the kernels on an MI355X).

Shapes: D in {128, 136, 2048, 4096, 4104, 8192} (1, 1 ragged, 4, 8, 16 ragged and 16 chunks of 8 channels per lane for the
norm -- every instance of the kernel; 16, 17, 256, 512, 513, 1024 lanes per row for the gate pass), rows = 4 * 4 * 3 + 5 = 53 (the last workgroup and the last wave end ragged), rows_per_group in
{1, 7, rows} (7: groups straddle waves and workgroups), row strides D + 8.

norm_modulate_f32in: the float64 truth and the three metrics of tests/norm_cases.py (``norm_modulate_op`` / ``compare``,
imported), on fp32 rows that are NOT bf16 values; for LayerNorm one row has its mean at 300 standard deviations.

gate_residual_f32:
  round_product = 1   bit-equal to torch's  h + (g32 * y32).to(bf16).float()  with g32 = table.float() + temb.float(): every
                      step is one correctly rounded operation, there is nothing to contract or reorder;
  round_product = 0,  |out - truth64| <= ulp32(max(|h|, |g y|)) per element, truth64 = h + g32 y in float64: a fused
  and gate = None     multiply-add is half an ulp of the sum off, and the sum is at most twice the larger term."""
import torch

import norm_cases as nc

BF = torch.bfloat16
F64 = torch.float64
WIDTHS = [128, 136, 2048, 4096, 4104, 8192]
ROWS = 4 * 4 * 3 + 5
GROUPS = [1, 7, ROWS]
KINDS = ["rms", "layer"]
PAD_COLS = 8


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def stream_rows(D, kind="rms", seed=0):
    """fp32 [ROWS, D] residual-stream rows: randn * 2 (24-bit mantissas), row scales over six decades on a few rows, and for
    LayerNorm row 3 with its mean at 300 standard deviations."""
    g = _gen(8100 + seed)
    x = torch.randn(ROWS, D, generator=g) * 2
    x[5] *= 1e-3
    x[11] *= 1e3
    if kind == "layer":
        x[3] = torch.randn(D, generator=g) + 300.0
    assert not torch.equal(x, x.to(BF).float())
    return x


def norm_case(kind, D, rpg):
    """(x fp32, table bf16 [6, D], temb bf16 [groups, 6 D], truth, mag)."""
    x = stream_rows(D, kind)
    table, temb = nc.modulation((ROWS + rpg - 1) // rpg, D)
    truth, mag = nc.norm_modulate_op(x, kind, nc.EPS_DIT, table[1], nc.group_rows(temb[:, D:2 * D], rpg, ROWS), table[0],
                                     nc.group_rows(temb[:, :D], rpg, ROWS))
    return x, table, temb, truth, mag


def norm_restated(kind, D, rpg):
    x, table, temb, truth, mag = norm_case(kind, D, rpg)
    out, _ = nc.norm_modulate_op(x, kind, nc.EPS_DIT, table[1], nc.group_rows(temb[:, D:2 * D], rpg, ROWS), table[0],
                                 nc.group_rows(temb[:, :D], rpg, ROWS), dt=torch.float32)
    return out.to(BF), truth, mag


def gate_case(D, rpg, seed=0):
    """(h fp32 [ROWS, D], y bf16, gate table bf16 [D], gate temb bf16 [groups, D] as a column block of [groups, 6 D])."""
    g = _gen(8200 + seed)
    h = stream_rows(D, seed=seed + 1)
    y = (torch.randn(ROWS, D, generator=g) * 1.5).to(BF)
    y[7] *= 100.0
    table, temb = nc.modulation((ROWS + rpg - 1) // rpg, D, seed=2)
    return h, y, table[2], temb[:, 2 * D:3 * D]


def gate32(table, temb, rpg):
    """The fp32 gate per row: table + temb of the row's group, one fp32 addition (exact for almost every bf16 pair)."""
    return table.float()[None] + nc.group_rows(temb.float(), rpg, ROWS)


def gate_rounded_expected(h, y, g32):
    return h + (g32 * y.float()).to(BF).float()


def ulp32(v):
    """Spacing of float32 at |v| (float64 tensor); the smallest normal's spacing below it."""
    v = v.abs().to(F64).clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 23)


def gate_unrounded_check(out, h, y, g32, what=""):
    """|out - (h + g y)| <= ulp32(max(|h|, |g y|)), the truth in float64; g32 None = the ungated h + y."""
    p = y.to(F64) if g32 is None else g32.to(F64) * y.to(F64)
    truth = h.to(F64) + p
    bound = ulp32(torch.maximum(h.to(F64).abs(), p.abs()))
    err = (out.detach().cpu().to(F64) - truth).abs()
    worst = float((err / bound).max())
    assert worst <= 1.0, f"{what}: an element is {worst:.3f} ulp of max(|h|, |g y|) from the float64 result"
    return worst
