"""Shapes, inputs, float64 truths and metrics for the bf16 GEMM -- TEST INFRASTRUCTURE ONLY (plain module, no GPU).

Shared by tests/test_gemm_cases.py (CPU) and tests/test_gpu_gemm_paths.py (MI355X).

INPUT FAMILIES (``make``): seeded, rounded to bf16 before anything is computed from them; no NaN, no infinity, nothing
near fp32 overflow.
  plain       A ~ randn, W ~ randn * K^-1/2, bias ~ randn
  cancel      plain, then the bias is the bf16 rounding of MINUS the float64 accumulator of one chosen row per column
              (row (7 n + 3) mod M for column n), so a band of outputs is the rounding residue of its own accumulator: near
              zero against the sum of magnitudes.  With the gated epilogue the residual is the bf16 rounding of
              -gate * (acc + bias) for EVERY element.  An epilogue that rounds to bf16 before its last addition fails it.
  large       A * 1e3
  row_scales  row r of A multiplied by 10 ** u_r, u_r uniform in [-3, 3]
The gate is the DiT's: gate_table [N] + a column slice [groups, N] of a [groups, 6 N] table (gate_ld = 6 N), values * 0.5;
the residual ~ randn.

TRUTH (``gemm_op``): the formula of include/ltxmi.h, generic over the dtype it runs in -- float64 is the truth, float32
followed by ONE rounding to bf16 (``restate``) is what a correct fp32-accumulating implementation gives.  It includes the
gate ``gate_table[n] + gate_temb[r // rows_per_group, n]`` and the K-blocked gather (the indexing of
tests/cpu_ops_double.py::gemm).  It returns (value, mag) with, per element,
  mag = sum_k |a| |w| + |bias|          (GELU / SiLU: the same, pre-activation -- their slope is at most 1.13)
  gated:  mag * (|gate_table| + |gate_temb|) + |residual|;   plain residual add: mag + |residual|.

METRICS (``compare``): a case must meet all three.
  (a) ``check`` of tests/test_gpu_kernels.py on the whole tensor (REL_L2 3e-3, MAXREL 1.6e-2; imported, not copied).
  (b) The same two figures per output row and per 256-column block of each row, for rows / blocks of at least 64 values.
      One wrong 16 x 16 fragment moves a 256-value block's L2 by a sixteenth of its norm.
  (c) Per element |out - truth| <= 2^-7 |truth| + SLACK * mag; elements with |truth| < 1e-30 are skipped.

SLACK.  Measured on the CPU (``measure_excess``; tests/test_gemm_cases.py re-measures and pins it) as the largest
(|restate - truth| - 2^-8 |truth|) / mag over every (family, epilogue, K) the GPU file uses (``SLACK_CASES``), at
M x N = 200 x 264: the error of an element depends on K, not on M or N.  Per epilogue, in units of 2^-24 = 5.96e-8:
  none 0.19, gelu 0.27, silu 0.093, gate 0.98, residual 0.29      (MEASURED_EXCESS_BY_EPI below)
so the largest is 5.9e-8 (MEASURED_EXCESS) and SLACK = 4 x 5.9e-8 = 2.36e-7 for every epilogue: 4 times, because the GPU
sums K in another order (32-wide MFMA steps) than torch's fp32 matmul, and its exp / tanh / rcp are good to about one fp32
ulp.  Nothing in it comes from a kernel.

CONDITION on the cases: the fp32 restatement alone meets all three metrics on every (family, epilogue, K) used on the GPU.
What cannot is listed in ``DROPPED`` with the figure it misses (at most one family per epilogue): nothing is -- the closest
figure of the restatement is the per-block L2 at 0.74 of its limit (two or three bf16 roundings of rms 1.1e-3 each)."""
import torch

BF = torch.bfloat16
F64 = torch.float64

FAMILIES = ["plain", "cancel", "large", "row_scales"]
EPIS = ["none", "gelu", "silu", "gate", "residual"]          # "residual": GATE_RESIDUAL without a gate table

# largest (|restate - truth| - 2^-8 |truth|) / mag per epilogue over SLACK_CASES (measure_excess); SLACK = 4 x the largest
MEASURED_EXCESS_BY_EPI = {"none": 1.12e-8, "gelu": 1.6e-8, "silu": 5.6e-9, "gate": 5.9e-8, "residual": 1.76e-8}
MEASURED_EXCESS = max(MEASURED_EXCESS_BY_EPI.values())
SLACK_TIMES = 4.0
SLACK = SLACK_TIMES * MEASURED_EXCESS

# (family, epilogue) pairs the fp32 restatement itself cannot pass, with the metric it misses
DROPPED = {}

# ------------------------------------------------------------------------------------------------------ GPU cases
# Every case of tests/test_gpu_gemm_paths.py: dict(M, N, K, epi, family, bias, id, algo, + operand-form keys).  The CPU
# file pins the kernel id of each and measures the slack over their (family, epilogue, K).
BIG = (5000, 4104, 192)          # 20 x 17 = 340 tiles: workgroups with one and with two tiles, nk = 3 (odd)
SMALL = (300, 264, 128)          # the 128x128 kernel: 3 x 3 tiles, ragged both ways


def _case(shape, epi="none", family="plain", bias=True, want=2, algo=0, **form):
    M, N, K = shape
    return dict(M=M, N=N, K=K, epi=epi, family=family, bias=bias, id=want, algo=algo, **form)


def case_id(c):
    s = f"{c['M']}x{c['N']}x{c['K']}-{c['epi']}-{c['family']}"
    if not c["bias"]:
        s += "-nobias"
    if c["algo"]:
        s += f"-algo{c['algo']}"
    for k in ("P", "rows_per_group", "in_place", "ldr_pad", "res_off", "ldc_pad", "c_off", "cols"):
        if k in c:
            s += f"-{k}{c[k]}"
    return s + f"-id{c['id']}"


PATH_CASES = (
    # one tile per workgroup (153 tiles); grid not a multiple of 8; last N band one tile wide and 8 columns wide; last M
    # tile one row; nk = 2 -- and some workgroups two tiles, some one; nk odd: consecutive tiles start in alternating stages
    [_case(s, epi=e, bias=b) for s in ((4097, 2056, 128), BIG) for e in ("none", "gelu", "silu", "gate") for b in (True, False)]
    + [_case((5000, 4104, 320)),
       _case((8200, 4360, 256), epi="gelu"),                 # 33 x 18 = 594 tiles: three tiles for some workgroups
       _case((2048, 4096, 128)),                             # exactly 128 tiles
       _case((2048, 3840, 128), want=0),                     # 120 tiles
       _case((2048, 4096, 8192)), _case((2048, 4096, 8192), family="cancel"),          # long K, the FF2 form
       _case((4097, 2056, 64), epi="silu", want=1),          # K = 64 at a persistent-sized shape
       _case((1, 8, 64), want=0), _case((129, 136, 64), epi="gelu", want=0), _case((767, 4096, 128), epi="gate", want=0),
       _case((1, 8, 64), want=1, algo=256), _case((129, 136, 64), epi="gelu", want=1, algo=256)]
    + [_case(BIG, epi=e, family=f) for f in ("cancel", "large", "row_scales") for e in ("none", "gelu", "silu", "gate")]
    + [_case((129, 136, 64), epi=e, family=f, want=0) for f in ("cancel", "large", "row_scales") for e in ("none", "gate")]
)

FORM_CASES = []
for _shape, _want in ((BIG, 2), (SMALL, 0)):
    _M, _N, _K = _shape
    # K-blocked A: [P][M][K/P] exactly, P in {2, 3}; a_kblock must be a multiple of 64, so K = 384 serves both P (blocks
    # of 192 and 128) and K = 192 / 128 give a_kblock = 64, one block per k-tile
    FORM_CASES += [_case((_M, _N, 384), want=_want, P=2), _case((_M, _N, 384), epi="gate", want=_want, P=3),
                   _case(_shape, epi="gate", want=_want, P=_K // 64)]
    # gate + residual: several groups inside one 16-row fragment / groups on tile boundaries / one group; in place and not
    FORM_CASES += [_case(_shape, epi="gate", want=_want, rows_per_group=r, in_place=ip)
                   for r in (37, 256, _M + 5) for ip in (True, False)]
    FORM_CASES += [_case(_shape, epi="residual", want=_want, in_place=ip) for ip in (True, False)]
# a residual the persistent kernel refuses: ldr % 8 == 4, or a base at +8 bytes -> the non-persistent 256x256 kernel
FORM_CASES += [_case(BIG, epi="gate", want=1, rows_per_group=256, in_place=False, ldr_pad=4),
               _case(BIG, epi="gate", want=1, rows_per_group=256, in_place=False, ldr_pad=8, res_off=4)]
# C with ldc % 8 == 4 and a base at +8 bytes on every kernel
FORM_CASES += [_case(SMALL, want=0, ldc_pad=12, c_off=4), _case(BIG, want=1, algo=256, ldc_pad=12, c_off=4),
               _case(BIG, want=2, ldc_pad=12, c_off=4)]

ROWSUMSQ_SHAPE = (4097, 4104, 128)       # ragged M, 17 x 17 tiles
ROWSUMSQ_COLS = [64, 192, 320]

# The two tile kernels (ids 0 and 1) share one epilogue with the two-pair kernels: its edges on both, at shapes of a few
# tiles.  M = 129 / 257 / 17: the last 16-row fragment partly out of range and the last tile partly empty; N = 136 (and 8):
# N % 16 = 8, the last fragment's columns clamped on the loads and masked on the stores; K = 64 / 128 / 192: no refill, the
# first refill, a refill into either stage.  No bias with every epilogue (a zero page with stride 0 stands in for it).
EDGE_MN = (129, 136)
EDGE_CASES = []
for _want, _algo in ((0, 0), (1, 256)):
    EDGE_CASES += [_case(EDGE_MN + (64,), epi=e, bias=False, want=_want, algo=_algo) for e in ("none", "gelu", "silu")]
    EDGE_CASES += [_case(EDGE_MN + (128,), epi=e, bias=False, want=_want, algo=_algo) for e in ("gate", "residual")]
    EDGE_CASES += [_case((257, 136, 192), want=_want, algo=_algo), _case((257, 136, 128), epi="gelu", want=_want, algo=_algo),
                   _case((17, 136, 192), epi="gate", want=_want, algo=_algo), _case((17, 8, 128), want=_want, algo=_algo)]
ROWSUMSQ_EDGE = (EDGE_MN + (64,), 64)    # (shape, rowsumsq_cols): the sums stop inside the one ragged N tile

GPU_CASES = PATH_CASES + FORM_CASES + EDGE_CASES
SLACK_MN = (200, 264)
SLACK_CASES = sorted({(c["family"], c["epi"], c["K"]) for c in GPU_CASES} | {("plain", "none", ROWSUMSQ_SHAPE[2])})


# ----------------------------------------------------------------------------------------------------- inputs
def make(family, M, N, K, epi="none", bias=True, rows_per_group=None, device="cpu", seed=0):
    """dict(a, w, bias, [gate_table, gate_temb, temb_full, residual], rows_per_group) of bf16 tensors on ``device``."""
    g = torch.Generator(device=device).manual_seed(8000 + 131 * FAMILIES.index(family) + seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    a = rn(M, K)
    if family == "large":
        a = a * 1e3
    elif family == "row_scales":
        a = a * 10.0 ** (torch.rand(M, 1, generator=g, device=device) * 6 - 3)
    d = dict(a=a.to(BF), w=(rn(N, K) * K ** -0.5).to(BF), bias=rn(N).to(BF) if bias else None, rows_per_group=1)
    if epi in ("gate", "residual"):
        d["residual"] = rn(M, N).to(BF)
    if epi == "gate":
        rpg = rows_per_group or max(1, (M + 2) // 3)
        groups = (M + rpg - 1) // rpg
        d["rows_per_group"] = rpg
        d["gate_table"] = (rn(N) * 0.5).to(BF)
        d["temb_full"] = (rn(groups, 6 * N) * 0.5).to(BF)
        d["gate_temb"] = d["temb_full"][:, 2 * N:3 * N]
    if family == "cancel":
        assert bias, "the cancel family is made through the bias"
        acc = d["a"].to(F64) @ d["w"].to(F64).T
        cols = torch.arange(N, device=device)
        rows = (7 * cols + 3) % M
        d["bias"] = (-acc[rows, cols]).to(BF)
        if epi in ("gate", "residual"):
            v = acc + d["bias"].to(F64)
            if epi == "gate":
                v = v * gate_rows(d, M, F64)
            d["residual"] = (-v).to(BF)
    return d


def empty_inputs(c):
    """Host tensors with the shapes and strides of ``make`` for case ``c``, never written: the geometry of the call."""
    M, N, K = c["M"], c["N"], c["K"]
    e = lambda *s: torch.empty(*s, dtype=BF)
    d = dict(a=e(M, K), w=e(N, K), bias=e(N) if c["bias"] else None, rows_per_group=1)
    if c["epi"] in ("gate", "residual"):
        d["residual"] = e(M, N)
    if c["epi"] == "gate":
        rpg = c.get("rows_per_group") or max(1, (M + 2) // 3)
        d.update(rows_per_group=rpg, gate_table=e(N), temb_full=e((M + rpg - 1) // rpg, 6 * N))
        d["gate_temb"] = d["temb_full"][:, 2 * N:3 * N]
    return d


SENTINEL = 7.0
PAD_ROWS = 2


def call_args(c, d, a=None):
    """(kwargs for ops.gemm / ops.gemm_kernel_id, out_buf, out) for case ``c`` on inputs ``d``.  The output is a view inside
    a sentinel-filled buffer: PAD_ROWS rows before and after, ldc - N pad columns (ldc = N + 8 unless the case sets ldc_pad),
    c_off elements past a 16-byte boundary.  In place: the view starts as the residual.  Out of place: the residual is a
    view of its own with ldr = N + 16 (or N + ldr_pad), res_off elements past a 16-byte boundary."""
    from ltxmi import ops
    M, N, K = c["M"], c["N"], c["K"]
    dev = d["a"].device
    ldc = N + c.get("ldc_pad", 8)
    out_buf = torch.full(((M + 2 * PAD_ROWS) * ldc + 16,), SENTINEL, dtype=BF, device=dev)
    out = torch.as_strided(out_buf, (M, N), (ldc, 1), PAD_ROWS * ldc + c.get("c_off", 0))
    epi = c["epi"]
    kw = dict(a=d["a"] if a is None else a, w=d["w"], bias=d["bias"], out=out, algo=c["algo"],
              epilogue={"none": ops.EPI_NONE, "gelu": ops.EPI_GELU_TANH, "silu": ops.EPI_SILU, "gate": ops.EPI_GATE_RESIDUAL,
                        "residual": ops.EPI_GATE_RESIDUAL}[epi])
    if "P" in c and a is None:
        P = c["P"]
        blocked = block_a(d["a"], P)
        kw.update(a=blocked[0], a_kblock=K // P, a_kblock_stride=M * (K // P))
    if epi in ("gate", "residual"):
        if c.get("in_place", True):
            out.copy_(d["residual"])
            kw["residual"] = out
        else:
            ldr = N + c.get("ldr_pad", 16)
            res_buf = torch.zeros(M * ldr + 16, dtype=BF, device=dev)
            res = torch.as_strided(res_buf, (M, N), (ldr, 1), c.get("res_off", 0))
            res.copy_(d["residual"])
            kw["residual"] = res
    if epi == "gate":
        kw.update(gate_table=d["gate_table"], gate_temb=d["gate_temb"], rows_per_group=d["rows_per_group"])
    return kw, out_buf, out


def sentinels_intact(out_buf, out):
    b = out_buf.clone()
    torch.as_strided(b, out.shape, out.stride(), out.storage_offset()).fill_(SENTINEL)
    return bool((b == SENTINEL).all())


def block_a(a, P):
    """[M, K] -> the receive buffer of the Ulysses return exchange [P][M][K/P] (contiguous, exactly that large)."""
    M, K = a.shape
    return a.view(M, P, K // P).permute(1, 0, 2).contiguous()


def gather_a(block0, K, a_kblock, a_kblock_stride):
    """The [M, K] operand a K-blocked A stands for: element k of row m at (k // a_kblock) * stride + m * lda + k % a_kblock."""
    M = block0.shape[0]
    blocks = torch.as_strided(block0, (K // a_kblock, M, a_kblock), (a_kblock_stride, block0.stride(0), 1))
    return blocks.permute(1, 0, 2).reshape(M, K)


def gate_rows(d, M, dt):
    """[M, N]: gate_table[n] + gate_temb[r // rows_per_group, n]."""
    idx = torch.arange(M, device=d["gate_temb"].device) // d["rows_per_group"]
    return d["gate_table"].to(dt)[None, :] + d["gate_temb"].to(dt)[idx]


# ------------------------------------------------------------------------------------- operation (dtype-generic)
def gemm_op(d, epi, dt=F64, a=None):
    """include/ltxmi.h: C = epilogue(A . W^T + bias) -> (value, mag) in dtype ``dt``.  ``a``: the [M, K] operand when it is
    not d["a"] (a gathered K-blocked A)."""
    a = (d["a"] if a is None else a).to(dt)
    w = d["w"].to(dt)
    M = a.shape[0]
    acc = a @ w.T
    mag = a.abs() @ w.abs().T
    if d.get("bias") is not None:
        acc = acc + d["bias"].to(dt)
        mag = mag + d["bias"].to(dt).abs()
    if epi == "gelu":
        acc = torch.nn.functional.gelu(acc, approximate="tanh")
    elif epi == "silu":
        acc = torch.nn.functional.silu(acc)
    elif epi == "gate":
        acc = acc * gate_rows(d, M, dt)
        idx = torch.arange(M, device=a.device) // d["rows_per_group"]
        mag = mag * (d["gate_table"].to(dt).abs()[None, :] + d["gate_temb"].to(dt).abs()[idx])
    if epi in ("gate", "residual"):
        acc = acc + d["residual"].to(dt)
        mag = mag + d["residual"].to(dt).abs()
    return acc, mag


def restate(d, epi, a=None):
    """fp32 arithmetic, one rounding to bf16: what a correct implementation of the header gives."""
    return gemm_op(d, epi, torch.float32, a)[0].to(BF)


# ----------------------------------------------------------------------------------------------------- metrics
def _check():
    from test_gpu_kernels import MAXREL, REL_L2, check
    return check, REL_L2, MAXREL


def _group_figures(err, truth):
    """(worst rel L2, worst max err / max |truth|) over the last axis."""
    tn = truth.norm(dim=-1)
    tm = truth.abs().amax(dim=-1)
    l2 = err.norm(dim=-1) / tn.clamp_min(1e-300)
    mx = err.abs().amax(dim=-1) / tm.clamp_min(1e-300)
    return float(l2.max()), float(mx.max())


def figures(out, truth, mag, slack=None):
    """The figures of metrics (b) and (c) as fractions of their limits (float64 arithmetic, on ``out``'s device)."""
    _, REL_L2, MAXREL = _check()
    slack = SLACK if slack is None else slack
    o, t = out.to(F64), truth.to(F64)
    M, N = t.shape
    err = o - t
    f = {}
    if N >= 64:
        l2, mx = _group_figures(err, t)
        f["row_l2"], f["row_max"] = l2 / REL_L2, mx / MAXREL
    nb = N // 256
    if nb:
        l2, mx = _group_figures(err[:, :nb * 256].reshape(M, nb, 256), t[:, :nb * 256].reshape(M, nb, 256))
        f["blk_l2"], f["blk_max"] = l2 / REL_L2, mx / MAXREL
    if N - nb * 256 >= 64:
        l2, mx = _group_figures(err[:, nb * 256:], t[:, nb * 256:])
        f["blk_l2"], f["blk_max"] = max(f.get("blk_l2", 0.0), l2 / REL_L2), max(f.get("blk_max", 0.0), mx / MAXREL)
    lim = 2.0 ** -7 * t.abs() + slack * mag.to(F64)
    ratio = torch.where(t.abs() >= 1e-30, err.abs() / lim.clamp_min(1e-300), torch.zeros_like(err))
    f["elem"] = float(ratio.max())
    return f


def compare(out, truth, mag, what="", slack=None):
    """All three metrics; returns the figures as fractions of their limits (the whole-tensor ones included)."""
    check, REL_L2, MAXREL = _check()
    assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    f = figures(out, truth, mag, slack)
    o, t = out.to(F64), truth.to(F64)
    f["all_l2"] = float((o - t).norm() / t.norm().clamp_min(1e-300)) / REL_L2
    f["all_max"] = float((o - t).abs().max() / t.abs().max().clamp_min(1e-300)) / MAXREL
    print(f"{what}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(f.items())))
    bad = {k: round(v, 4) for k, v in f.items() if not v <= 1.0}
    assert not bad, f"{what}: over the limit (fraction of it): {bad}"
    check(out, truth, what=what)
    return f


def measure_excess(cases=None):
    """{epilogue: largest (|restate - truth| - 2^-8 |truth|) / mag} over SLACK_CASES at M x N = SLACK_MN (CPU)."""
    M, N = SLACK_MN
    worst = {}
    for family, epi, K in (SLACK_CASES if cases is None else cases):
        if (family, epi) in DROPPED:
            continue
        d = make(family, M, N, K, epi)
        t, mag = gemm_op(d, epi)
        r = restate(d, epi).to(F64)
        ex = float((((r - t).abs() - 2.0 ** -8 * t.abs()) / mag).max())
        worst[epi] = max(worst.get(epi, 0.0), ex)
    return worst
