"""Cases of the two-pair GEMM (ltxmi_gemm_pair2_bf16, ``ops.gemm(..., a2=, w2=)``) -- TEST INFRASTRUCTURE ONLY (plain module).

Shared by tests/test_lora_gemm_cases.py (CPU) and tests/test_gpu_lora_gemm.py (MI355X).

A call with K1 + K2 is, numerically, a GEMM of that K: the inputs are ``gemm_cases.make`` on the CONCATENATED K, cut into
(A | A2) and (W | W2) at K1; truth and per-element magnitude are ``gemm_cases.gemm_op`` on the materialised concatenation, the
bounds ``gemm_cases.compare`` with its SLACK -- all imported, none copied.  On top of that the kernel must give the BITS
``ops.gemm`` gives on the concatenation (same K-tile order, same epilogue sequence).

Grouped cases (a packed projection with a packed adapter): ``make`` runs on K1 + groups * K2 columns; group g's A2 is columns
[K1 + g K2, K1 + (g + 1) K2) of that A, W2 is columns [K1, K1 + K2) of that W, and the concatenation of group g is compared on
its column slice [g group_cols, (g + 1) group_cols).

(K1, K2) put the pair boundary inside the two-tile prologue (64 + 64, 64 + 128), at the first refill (128 + 64), at an odd and an
even total (192 + 64, 128 + 192) and on a step-like K (2048 + 128)."""
import ctypes

import torch

import gemm_cases as gc

SMALL_MN = (300, 264)            # the 128x128 two-pair kernel (id 3): 3 x 3 tiles, ragged both ways
BIG_MN = (5000, 4104)            # the 256x256 one (id 4): 20 x 17 = 340 tiles, ragged both ways, last N band 8 columns wide
K_SPLITS = [(64, 64), (64, 128), (128, 64), (192, 64), (128, 192), (2048, 128)]
ROWSUMSQ_COLS = [64, 320]


def _case(mn, k1, k2, epi="none", family="plain", bias=True, want=3, algo=0, groups=1, group_cols=0, **form):
    M, N = mn
    return dict(M=M, N=N, K1=k1, K2=k2, K=k1 + groups * k2, epi=epi, family=family, bias=bias, id=want, algo=algo,
                groups=groups, group_cols=group_cols, **form)


def case_id(c):
    s = f"{c['M']}x{c['N']}x{c['K1']}+{c['K2']}-{c['epi']}-{c['family']}"
    if not c["bias"]:
        s += "-nobias"
    if c["algo"]:
        s += f"-algo{c['algo']}"
    if c["group_cols"]:
        s += f"-{c['groups']}groups{c['group_cols']}"
    for k in ("rows_per_group", "in_place", "a2_view"):
        if k in c:
            s += f"-{k}{c[k]}"
    return s + f"-id{c['id']}"


GPU_CASES = []
for _mn, _want in ((SMALL_MN, 3), (BIG_MN, 4)):
    # the pair boundary at every place of the K-tile stream; A2 contiguous (lda2 = K2) and a column view of a wider tensor
    GPU_CASES += [_case(_mn, k1, k2, want=_want) for k1, k2 in K_SPLITS]
    GPU_CASES += [_case(_mn, k1, k2, want=_want, a2_view=True) for k1, k2 in ((64, 64), (128, 64), (2048, 128))]
    # every epilogue, two families, bias on and off
    GPU_CASES += [_case(_mn, 128, 64, epi=e, family=f, want=_want) for f in ("plain", "cancel") for e in ("none", "gelu", "silu")
                  if (e, f) != ("none", "plain")]
    GPU_CASES += [_case(_mn, 128, 64, epi=e, bias=False, want=_want) for e in ("none", "gelu", "gate")]
    GPU_CASES += [_case(_mn, 128, 64, epi="gate", family=f, want=_want, rows_per_group=r, in_place=ip)
                  for f, r, ip in (("plain", 37, True), ("plain", 37, False), ("plain", 256, True), ("plain", 256, False),
                                   ("cancel", 37, True), ("cancel", 256, False))]
    GPU_CASES += [_case(_mn, 128, 64, epi="residual", family=f, want=_want, in_place=ip)
                  for f, ip in (("plain", True), ("plain", False), ("cancel", False))]
    GPU_CASES += [_case(_mn, 2048, 128, epi="gelu", want=_want), _case(_mn, 2048, 128, epi="gate", want=_want, a2_view=True)]
# packed adapters: N = 768 in three groups of 256 columns on both forms (43 x 3 = 129 tiles of 256 for id 4), six groups of 128 on id 3
GPU_CASES += [_case((300, 768), 128, 64, groups=3, group_cols=256, want=3),
              _case((300, 768), 128, 64, groups=3, group_cols=256, want=3, a2_view=True),
              _case((10800, 768), 128, 64, groups=3, group_cols=256, want=4),
              _case((10800, 768), 128, 64, groups=3, group_cols=256, want=4, a2_view=True),
              _case((300, 768), 128, 64, groups=6, group_cols=128, want=3)]
GPU_CASES += [_case((1, 8), 64, 64, want=3)]
# forced forms: the 256x256 kernel on the small shape, the 128x128 one on the big
GPU_CASES += [_case(SMALL_MN, 128, 64, epi="gelu", want=4, algo=256), _case(BIG_MN, 128, 64, epi="gelu", want=3, algo=128)]

# the edges of the epilogue the two forms share with gemm.hip's tile kernels (gemm_cases.EDGE_CASES), on the smallest stream
# (K = 64 with K2 = 64: nk = 2, the pair switches inside the prologue): M = 129, N = 136, no bias with every epilogue
for _want, _algo in ((3, 0), (4, 256)):
    GPU_CASES += [_case(gc.EDGE_MN, 64, 64, epi=e, bias=False, want=_want, algo=_algo)
                  for e in ("none", "gelu", "silu", "gate", "residual")]
    GPU_CASES += [_case(gc.EDGE_MN, 64, 64, epi="gelu", want=_want, algo=_algo), _case((17, 8), 64, 128, want=_want, algo=_algo)]
GPU_CASES += [_case((1, 8), 64, 64, want=4, algo=256)]

# (family, epilogue, K of the concatenation) of every case above and of the row-sums test
SLACK_CASES = sorted({(c["family"], c["epi"], c["K1"] + c["K2"]) for c in GPU_CASES} | {("plain", "none", 192)})


# ------------------------------------------------------------------------------------------------------ operands
def split(c, d):
    """(a1, w1, a2, w2) of case ``c`` cut out of the inputs ``d`` that ``gemm_cases.make`` made on c["K"] columns."""
    K1, K2 = c["K1"], c["K2"]
    a, w = d["a"], d["w"]
    a2 = a[:, K1:] if c.get("a2_view") else a[:, K1:].contiguous()
    return a[:, :K1].contiguous(), w[:, :K1].contiguous(), a2, w[:, K1:K1 + K2].contiguous()


def concatenation(c, d, g=0):
    """The inputs of the plain GEMM that group ``g`` of the case equals: [A | A2_g], [W | W2] on the group's output columns."""
    if c["groups"] == 1:
        return d
    K1, K2, gcols = c["K1"], c["K2"], c["group_cols"]
    n0, n1 = g * gcols, (g + 1) * gcols
    a = torch.cat([d["a"][:, :K1], d["a"][:, K1 + g * K2:K1 + (g + 1) * K2]], dim=1)
    return dict(a=a, w=d["w"][n0:n1, :K1 + K2].contiguous(), bias=None if d["bias"] is None else d["bias"][n0:n1].contiguous(),
                rows_per_group=1)


def call_args(c, d):
    """(kwargs for ops.gemm / ops.gemm_kernel_id with the second pair, out_buf, out): ``gemm_cases.call_args`` on the first
    pair -- the output a view inside a sentinel-filled buffer -- plus a2 / w2 / a2_group_cols."""
    a1, w1, a2, w2 = split(c, d)
    kw, out_buf, out = gc.call_args(c, d, a=a1)
    kw.update(w=w1, a2=a2, w2=w2, a2_group_cols=c["group_cols"])
    return kw, out_buf, out


def empty_inputs(c):
    return gc.empty_inputs(c)


# ------------------------------------------------------------------------------------------- the entry check's refusals
# (what, overrides, status): overrides of the ltxmi_gemm_args / ltxmi_gemm_pair built by ``geometry`` (pointer-valued ones are
# byte offsets from a 64-byte aligned fake base, None = NULL; "pair": None = a NULL pair).  M x N x K1 + K2 = 300 x 768 x 128 + 64.
REFUSALS = [
    ("accepted", {}, 3),
    ("accepted_groups", dict(group_cols=256, lda2=192), 3),
    ("accepted_groups128", dict(group_cols=128, lda2=384), 3),
    ("algo256", dict(algo=256), 4),
    ("algo256_groups256", dict(algo=256, group_cols=256, lda2=192), 4),
    ("null_args", dict(args=None), -1),
    ("null_pair", dict(pair=None), -1),
    ("null_A2", dict(A2=None), -1),
    ("null_W2", dict(W2=None), -1),
    ("K2_zero", dict(K2=0), -1),
    ("K2_negative", dict(K2=-64), -1),
    ("K2_mod64", dict(K2=96, lda2=96, ldw2=96), -1),
    ("group_cols_negative", dict(group_cols=-256), -1),
    ("group_cols_mod128", dict(group_cols=192, lda2=256), -1),
    ("group_cols_not_dividing", dict(group_cols=512, lda2=128), -1),
    ("algo256_groups128", dict(algo=256, group_cols=128, lda2=384), -1),
    ("algo7", dict(algo=7), -1),
    ("a_kblock", dict(a_kblock=64, a_kblock_stride=300 * 64, lda=64), -2),
    ("A2_plus8", dict(A2=8), -2),
    ("W2_plus8", dict(W2=8), -2),
    ("lda2_mod8", dict(lda2=68), -2),
    ("ldw2_mod8", dict(ldw2=68), -2),
    ("ldw2_below_K2", dict(ldw2=56), -2),
    ("lda2_below_groups_K2", dict(group_cols=256, lda2=128), -2),
    ("lda2_2p31", dict(lda2=1 << 22), -2),
    # the first pair's checks are ltxmi_gemm_bf16's
    ("K1_mod64", dict(K=100, lda=128, ldw=128), -2),
    ("N12", dict(N=12, ldc=12), -2),
    ("M0", dict(M=0), -1),
    ("a_plus8", dict(A=8), -2),
    ("epilogue99", dict(epilogue=99), -1),
    ("gate_without_residual", dict(epilogue=3), -1),
]


def geometry(over):
    """(args or None, pair or None) on fake addresses: nothing is dereferenced by the entry check."""
    from ltxmi import _lib
    over = dict(over)
    base = 1 << 30
    a, p = _lib.GemmArgs(), _lib.GemmPair()
    a.A = a.W = a.C = base
    a.M, a.N, a.K = 300, 768, 128
    a.lda = a.ldw = 128
    a.ldc = 768
    a.rows_per_group = 1
    p.A2 = p.W2 = base
    p.K2, p.lda2, p.ldw2 = 64, 64, 64
    keep_args, keep_pair = over.pop("args", True), over.pop("pair", True)
    for k, v in over.items():
        tgt = p if hasattr(p, k) else a
        if k in ("A", "W", "C", "A2", "W2", "bias", "residual"):
            v = None if v is None else base + v
        setattr(tgt, k, v)
    return (a if keep_args is not None else None), (p if keep_pair is not None else None)


def kernel_id(a, p):
    from ltxmi import _lib
    return _lib.lib.ltxmi_gemm_pair2_kernel_id(ctypes.byref(a) if a is not None else None, ctypes.byref(p) if p is not None else None)
