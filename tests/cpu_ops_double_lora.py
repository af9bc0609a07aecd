"""The CPU stand-in of ``ops.gemm`` with the second operand pair -- TEST INFRASTRUCTURE ONLY.

Installed on top of tests/cpu_ops_double_mixed.py (``install()`` here calls that one first).  ``gemm(..., a2=, w2=,
a2_group_cols=)`` has the meaning of ltxmi_gemm_pair2_bf16 (include/ltxmi.h): it is tests/cpu_ops_double.py's ``gemm`` run,
group by group, on the concatenation [a | a2_g], [w | w2] of the group's output columns -- fp32 arithmetic, one rounding to the
output dtype, the epilogue applied to the sum.  Without ``a2`` it is that function's own call."""
import torch

import cpu_ops_double
import cpu_ops_double_mixed
from cpu_ops_double import _rows

_base_gemm = cpu_ops_double.gemm


def gemm(a, w, bias=None, out=None, epilogue=0, residual=None, gate_table=None, gate_temb=None, rows_per_group=1,
         algo=0, rowsumsq=None, rowsumsq_cols=0, a_kblock=0, a_kblock_stride=0, a2=None, w2=None, a2_group_cols=0):
    if a2 is None:
        assert w2 is None
        return _base_gemm(a, w, bias, out, epilogue, residual, gate_table, gate_temb, rows_per_group, algo, rowsumsq,
                          rowsumsq_cols, a_kblock, a_kblock_stride)
    assert not a_kblock, "a K-blocked A takes no second pair"
    x, t = _rows(a), _rows(a2)
    M, (N, K) = x.shape[0], w.shape
    K2 = w2.shape[1]
    gcols = a2_group_cols or N
    groups = N // gcols
    assert K2 % 64 == 0 and N % gcols == 0 and (a2_group_cols == 0 or gcols % 128 == 0)
    assert t.shape == (M, groups * K2) and w2.shape[0] == N and t.dtype == x.dtype == w2.dtype
    res = torch.empty((M, N), dtype=a.dtype)
    for g in range(groups):
        cols = slice(g * gcols, (g + 1) * gcols)
        res[:, cols] = _base_gemm(torch.cat([x, t[:, g * K2:(g + 1) * K2]], 1), torch.cat([w[cols], w2[cols]], 1),
                                  None if bias is None else bias[cols], None, epilogue,
                                  None if residual is None else _rows(residual)[:, cols],
                                  None if gate_table is None else gate_table[cols],
                                  None if gate_temb is None else gate_temb[:, cols], rows_per_group)
    if rowsumsq is not None:
        nb = rowsumsq_cols // 64
        rowsumsq[:, :nb] = res[:, :rowsumsq_cols].float().reshape(M, nb, 64).pow(2).sum(-1)
    if out is None:
        return res
    _rows(out).copy_(res)
    return out


def install():
    """cpu_ops_double_mixed.install() + the two-pair ``gemm`` (this process only)."""
    ops = cpu_ops_double_mixed.install()
    ops.gemm = gemm
    return ops
