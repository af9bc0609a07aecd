"""Cases and float64 restatements for the two entries of include/ltxmi_mx_attn.h -- TEST INFRASTRUCTURE ONLY (plain module, no
GPU), built on tests/mx8_cases.py (the format, the GEMM operands and truth) and tests/norm_cases.py (the norm's truth).  Shared by
tests/test_mxa_cases.py (CPU) and tests/test_gpu_mxa_kernels.py (MI355X).

ROW SUMS (ltxmi_gemm_mx8_rowsumsq).  "GEMM, round to bf16, row sums": ``rowsumsq`` is the float64 sum of squares of a STORED bf16
output over each 64-column block below ``cols``; ``gemm_rowsumsq_restate`` applies it to mx8_cases' fp32 restatement of the GEMM.
On the device the output must equal ``ops.gemm_mx8``'s bit for bit, and the sums are held to ``rowsumsq`` of that output at
rtol 1e-5 / atol 1e-6, the figures tests/test_gpu_gemm_paths.py holds the bf16 GEMM's sums to: 64 non-negative fp32 terms,
each product exact to 2^-24, summed in any order, are within 64 * 2^-24 = 3.8e-6 of the exact sum, relatively.
  (300, 288, 256)   cols 64 (one block of the first tile), 192, 256 (a whole tile; the ragged 32-column tile has no block);
  (520, 544, 384)   cols 320 (the sums cross a tile boundary and stop inside the second tile), 512 (two whole tiles; the ragged
                    third tile holds 32 columns);
  (1, 288, 256)     M = 1.
Each with and without a bias, over the operand families plain and row_scales.
EXACT SUMS (``rss_exact``): mx8_cases' flat probe, whose outputs are small integers; the sums are then exact in fp32 in any order
and must equal the float64 sums, with no tolerance, at the first block, a whole band of tiles and into the narrow last band.

FUSED NORM + QUANTISE (ltxmi_norm_modulate_mx8).  "norm-modulate, round to bf16, quantise": ``norm_quant_restate`` is
norm_cases.norm_modulate_op in float64, one rounding to bf16, mx8_cases.quantize.  On the device the entry must equal the two
launches it replaces bit for bit, so the restatement is the CPU's statement of what both compute, not the device's yardstick.
Rows {1, 37, 300} (one workgroup's rows, a ragged last workgroup), D {64, 2048, 2080, 4096} (one chunk per lane, the last lane of
the 4-chunk kernel full, the first width of the 16-chunk kernel with a ragged chunk walk, a wide row), both norm kinds,
rows_per_group {1, 13} (13 divides neither 37 nor 300: a group ends inside a workgroup)."""
import torch

import mx8_cases as mc
import norm_cases as nc

BF, F64 = mc.BF, mc.F64
EPS = 1e-6

RSS_SHAPES = {(300, 288, 256): (64, 192, 256), (520, 544, 384): (320, 512), (1, 288, 256): (64,)}
RSS_FAMILIES = ["plain", "row_scales"]
RSS_CASES = [dict(shape=s, cols=c, bias=b, family=f) for s, cc in RSS_SHAPES.items() for c in cc for b in (True, False)
             for f in RSS_FAMILIES]
RSS_RTOL, RSS_ATOL = 1e-5, 1e-6
# exact sums on mx8_cases' flat probe, one K-tile.  (300, 2336, 128) is 2 x 10 tiles in bands of 8: cols 64 is the first block,
# 2048 the whole first band, 2304 reaches into the narrow band (the last, 32-column tile holds no block); (257, 64, 128) is 2 x 1
# tiles, one row in the second
RSS_EXACT_SHAPES = {(300, 2336, 128): (64, 2048, 2304), (257, 64, 128): (64,)}
RSS_EXACT_CASES = [dict(shape=s, cols=c, bias=b) for s, cc in RSS_EXACT_SHAPES.items() for c in cc for b in (True, False)]

NORM_ROWS, NORM_D, NORM_KINDS, NORM_RPG = (1, 37, 300), (64, 2048, 2080, 4096), ("rms", "layer"), (1, 13)
NORM_CASES = [dict(rows=r, D=D, kind=k, rpg=g) for r in NORM_ROWS for D in NORM_D for k in NORM_KINDS for g in NORM_RPG]


def rss_id(c):
    return "x".join(map(str, c["shape"])) + f"-cols{c['cols']}-{'bias' if c['bias'] else 'nobias'}-{c['family']}"


def norm_id(c):
    return f"{c['rows']}x{c['D']}-{c['kind']}-rpg{c['rpg']}"


# ------------------------------------------------------------------------------------------------- row sums
def rowsumsq(c, cols):
    """c [M, N] bf16 (the stored output) -> float64 [M, cols / 64]."""
    assert c.dtype == BF and cols % 64 == 0 and 0 < cols <= c.shape[1]
    return (c[:, :cols].to(F64) ** 2).reshape(c.shape[0], cols // 64, 64).sum(dim=-1)


def gemm_rowsumsq_restate(d, cols, bias=True):
    """mx8_cases.make's operands -> (C bf16 [M, N], sums float64 [M, cols / 64]): fp32 product of the de-quantised operands, the
    bias, one rounding to bf16, the sums of what was rounded."""
    acc = mc.product(d, torch.float32)[0]
    c = (acc + d["bias"].to(torch.float32) if bias else acc).to(BF)
    return c, rowsumsq(c, cols)


def rss_exact_id(c):
    return "x".join(map(str, c["shape"])) + f"-cols{c['cols']}-{'bias' if c['bias'] else 'nobias'}"


def rss_exact(c, device="cpu"):
    """An RSS_EXACT_CASES entry -> mx8_cases.exact's dict (epilogue none, bf16 output) with ``sums`` float64 [M, cols / 64]: the
    outputs are integers of magnitude <= 15 (<= 7 without the bias), so a block's sum is an integer <= 64 * 225 and every partial
    sum in any order is exact in fp32: the device's sums must EQUAL these."""
    d = mc.exact(dict(shape=c["shape"], epi="none", bias=c["bias"], out="bf16", in_place=False, rpg=None, one_hot="a"), device)
    d["sums"] = rowsumsq(d["truth"].to(BF), c["cols"])
    return d


def rss_exact_ok(d):
    t, s = d["truth"], d["sums"]
    return mc.exact_ok(d) and bool((t == t.round()).all()) and float(t.abs().max()) <= 15 and float(s.max()) <= 64 * 225 and \
        bool((s.to(torch.float32).to(F64) == s).all())


# ------------------------------------------------------------------------------------------------- fused norm + quantise
def norm_inputs(c, family="plain"):
    """(x [rows, D], table [6, D], temb [groups, 6 D]) bf16 as norm_cases draws them; scale = row 1, shift = row 0."""
    groups = (c["rows"] + c["rpg"] - 1) // c["rpg"]
    return (nc.make(family, c["rows"], c["D"]),) + nc.modulation(groups, c["D"])


def modulation_views(table, temb, D):
    """-> (scale_table [D], scale_temb [groups, D], shift_table [D], shift_temb [groups, D]): views, the temb ones row-strided."""
    return table[1], temb[:, D:2 * D], table[0], temb[:, :D]


def norm_quant_restate(x, kind, table, temb, rpg, eps=EPS):
    """-> (y bf16 [rows, D], q float8_e4m3fn [rows, D], scales uint8 [rows, D / 32])."""
    rows, D = x.shape
    sc_t, sc_e, sh_t, sh_e = modulation_views(table, temb, D)
    y = nc.norm_modulate_op(x, kind, eps, sc_t, nc.group_rows(sc_e, rpg, rows), sh_t, nc.group_rows(sh_e, rpg, rows))[0].to(BF)
    return (y,) + mc.quantize(y)


def witness_inputs(D):
    """mx8_cases.witness_rows with a modulation of scale = 0 and shift = 0: RMS-normalised, every row is its witness pattern times
    one factor, so the blocks' amax sit in fixed ratios around the scale rule's thresholds wherever that factor puts them."""
    x = mc.witness_rows(D)
    return x, torch.zeros(6, D, dtype=BF), torch.zeros(x.shape[0], 6 * D, dtype=BF)
