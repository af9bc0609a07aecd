"""The MX-FP8 format restated, the float64 GEMM truth on de-quantised operands, and the case tables -- TEST INFRASTRUCTURE ONLY
(plain module, no GPU).  Shared by tests/test_mx8_cases.py (CPU) and tests/test_gpu_mx8_kernels.py (MI355X).

FORMAT (include/ltxmi_mx.h), restated here with integer arithmetic on the bit patterns plus torch's float8_e4m3fn cast:
  block     32 consecutive elements along K of one row; one E8M0 byte per block, byte = e + 127;
  e         the smallest integer with amax * 2^-e <= 448: amax = m * 2^k, m in [1, 2): e = k - 8 if m <= 1.75 else k - 7
            (448 = 1.75 * 2^8), clamped to [-127, 127]; an all-zero block has byte 0;
  elements  q = RNE(x * 2^-e) to OCP e4m3fn.  x * 2^-e is formed in float64 (exact: a power-of-two product) and is at most
            448 in magnitude, so torch's cast (RNE, no saturation) is the format's rounding.
``scale_bytes_bf16`` reads k and m from bf16 bits (subnormals normalised by hand), ``scale_bytes_real`` from any real tensor
through frexp (the MX-output epilogue quantises fp32 values; the truth it is held against is float64).

GEMM.  ``make`` draws bf16 operands as tests/gemm_cases.py draws them (families plain, cancel, row_scales), quantises BOTH with
the restatement and keeps the quantised forms: the truth is the float64 product of the DE-QUANTISED operands, so the
quantisation itself is not part of the error -- what is left is accumulation order and the epilogue's rounding, the bf16 GEMM's
figures.  ``cancel`` takes its bias (and residual) from that float64 accumulator.  ``epilogue_op`` is gemm_cases.gemm_op after
the product (the product and mag are computed once per (family, shape) and shared by the epilogues).

SLACK as tests/gemm_cases.py defines it: 4 x the largest (|restate - truth| - 2^-8 |truth|) / mag of an fp32 restatement (fp32
matmul of the de-quantised operands, one rounding to bf16) over every (family, epilogue, K) the GPU file uses, at
M x N = 200 x 288.  Nothing in it comes from a kernel; tests/test_mx8_cases.py re-measures and pins it, and holds the
restatement alone to every metric of every GPU case's (family, epilogue, K).

TRUNC.  The block-scaled MFMA does not sum its products as an fp32 fma chain.  Exact witness (``witness_truncation``, asserted on
the device by tests/test_gpu_mx8_kernels.py): 256 * 256 = 2^16 at k = 0 and n products 1 * 1 from k = 1 on, the 2^16 cancelled by
the residual, gives max(0, n - 7) -- the seven ones that share the large product's group of 8 consecutive k are lost, every later
one is kept; one product v at k = 1 gives 8 floor(v / 8); beside 2^13 instead of 2^16 nothing is lost; in another block, or from
k = 8 on, nothing is lost.  So inside a group of 8 consecutive k each product is cut (towards zero) at 2^-13 of the power of two of
the group's largest product, and the groups are summed far more finely (a term survives 2^-27 below the largest).  Per output
that is an error below 7 * 2^-13 * sum over groups of the group's largest |a w|; with GELU's slope (at most 1.13) below
TRUNC * tmag, TRUNC = 8 * 2^-13 = 2^-10 and tmag = sum_g max_g |a| * max_g |w| (``trunc_mag``, one [M, K/8] x [K/8, N] product).
The per-element limit of the GPU file is therefore 2^-7 |truth| + SLACK mag + TRUNC tmag (``eff_mag`` folds the last term into
the mag that gemm_cases.compare takes, so the gate scales it as it scales mag).  The figure is reasoned from the witness (the worst case of
the cut), not fitted to what the random families give.

SHAPES.  (300, 288, 256): ragged against the 256 x 256 tile both ways, N = 256 + one block, two K-tiles.  (The issue wrote
300 x 264 x 256; 264 is no multiple of 32 and the entry refuses it, so N is the next multiple that keeps the shape ragged.)
(2048, 4096, 8192): the FF2 form, 64 K-tiles, 128 tiles.  (1, 288, 256) and (1, 4096, 8192): M = 1.
(257, 32, 128), (300, 2336, 128) and, for cancel + gate, (300, 288, 128): the random families where the GELU instances meet one
K-tile, one column block and the narrow last band (``WALK_SHAPES`` gives the tile counts).  Re-measured with K = 128 among
SLACK_CASES the excess figures did not move (their largest are at K = 8192), and no new case had to be dropped.

EXACT WITNESSES (no tolerance anywhere; the device must give the bits of the float64 value).
  probe        ``scales="flat"``: every scale 2^0, the outputs are the integers -7 .. 7.  ``scales="wide"``: the A bytes run over
               1 .. 253 with the block index (plus r mod 6), the W bytes are the complement (minus c mod 6), so ea + ew = r mod 6 -
               c mod 6 and every output is a bf16 normal although each scale alone is as far as 2^+-126 from 1.
               ``geometry="strided"``: the same numbers as views with lda = K + 16, lda_s = K / 32 + 4 from byte 4 of its buffer,
               the weight and its scales as rows [5, 5 + N) of arrays of N + 9 rows, NaN bytes (0x7f / 0xff) around every view.
  tile walk    ``WALK_SHAPES`` at one K-tile, ``KTILE_SHAPES`` at 1, 4, 5, 7 K-tiles; with PROBE_SHAPES' 2 and 3 every path of the
               kernel's prologue and K loop (``TRUTH_KTILES``), which the skinny suite's chain to a truth rests on.
  epilogues    ``exact``: the flat probe with an integer bias (-8 .. 8), an integer residual (-32 .. 32) and a gate sum in
               {0, +-0.5, +-1, +-2}.  CONDITION (``exact_ok``, asserted for every case on the CPU): every partial result is a multiple
               of 0.5 below 2^24 in magnitude -- exact in fp32 in any order and association -- and the result is representable in
               the output format (bf16; for the MX output the integers of magnitude <= 15 survive quantise -> de-quantise).
  threshold    ``witness_mx_out_threshold``: fp32 accumulators exactly at, just above and just below 1.75 * 2^k.
  outputs      ``guarded``: the output view lies in a buffer filled with a pattern no result can be (a bf16 / fp32 NaN, the e4m3 NaN
               0x7f, the E8M0 NaN 0xff); ``guard_figures`` counts the patterns left inside the view and the changes outside it."""
import torch

import gemm_cases

BF, F64 = torch.bfloat16, torch.float64
E4M3 = torch.float8_e4m3fn
BLOCK = 32

FAMILIES = ["plain", "cancel", "row_scales"]
EPIS = ["none", "gelu", "gate", "residual"]           # "residual": GATE_RESIDUAL without a gate table
MX_EPIS = ["none", "gelu"]                            # the MX-output forms

SMALL, BIG = (300, 288, 256), (2048, 4096, 8192)
GEMM_CASES = ([dict(shape=s, family=f, epi=e) for s in (SMALL, BIG) for f in FAMILIES for e in EPIS]
              + [dict(shape=(1,) + s[1:], family="plain", epi=e) for s in (SMALL, BIG) for e in EPIS])
MXOUT_CASES = ([dict(shape=s, family=f, epi=e) for s in (SMALL, BIG) for f in FAMILIES for e in MX_EPIS]
               + [dict(shape=(1,) + SMALL[1:], family="plain", epi="gelu")])
# Tiles are 256 x 256 x 128 and walked in bands of 8 N-tiles, M-major inside a band.  (M, N, K): tiles_m x tiles_n, K-tiles.
EDGE_1, EDGE_NARROW = (257, 32, 128), (300, 2336, 128)
WALK_SHAPES = [(256, 256, 128),        # 1 x 1, 1: an exact tile with nothing masked
               EDGE_1,                 # 2 x 1, 1: one valid row in the second M-tile; 224 of 256 weight rows clamped; one column block
               EDGE_NARROW,            # 2 x 10, 1: the second band is 2 tiles wide; the last tile is 32 columns
               (520, 2848, 128)]       # 3 x 12, 1: the last band is 4 tiles wide
# 2 x 2 tiles; nk = 1: no second stage and no ktile with `more`; 4, 5, 7: two, three and five refills, into either stage twice over
KTILE_SHAPES = [(300, 288, 128 * t) for t in (1, 4, 5, 7)]
# the first two: 2 x 2 tiles, two K-tiles (no refill); 3 x 3 tiles, three K-tiles (one refill)
PROBE_SHAPES = [SMALL, (520, 544, 384)] + WALK_SHAPES + KTILE_SHAPES
TRUTH_KTILES = sorted({s[2] // 128 for s in PROBE_SHAPES})             # the K-tile counts ltxmi_gemm_mx8 is held to a truth at
PROBE_VARIANTS = [dict(shape=(300, 288, 512), scales="wide", geometry="contiguous"),     # 2 x 2 tiles, 4 K-tiles = 16 blocks
                  dict(shape=(257, 32, 512), scales="wide", geometry="contiguous"),      # 2 x 1
                  dict(shape=(300, 288, 384), scales="varied", geometry="strided"),      # 2 x 2, three K-tiles
                  dict(shape=EDGE_NARROW, scales="varied", geometry="strided")]          # 2 x 10, one K-tile
GEMM_CASES += ([dict(shape=s, family="plain", epi=e) for s in (EDGE_1, EDGE_NARROW) for e in EPIS]
               + [dict(shape=(300, 288, 128), family="cancel", epi="gate")])
MXOUT_CASES += [dict(shape=s, family="plain", epi=e) for s in (EDGE_1, EDGE_NARROW) for e in MX_EPIS]


def _exact(shape, epi="none", bias=True, out="bf16", in_place=False, rpg=None, one_hot="a"):
    return dict(shape=shape, epi=epi, bias=bias, out=out, in_place=in_place, rpg=rpg, one_hot=one_hot)


# every exact epilogue case at the narrow band and at the one column block; rpg 1, 7 (a group ends inside a tile, the last group
# is partial: 7 divides neither 300 nor 257) and M + 3 (a single group)
EXACT_CASES = [c for s in (EDGE_NARROW, EDGE_1) for c in (
    _exact(s), _exact(s, bias=False),
    _exact(s, "residual"), _exact(s, "residual", in_place=True), _exact(s, "residual", bias=False),
    _exact(s, "gate", rpg=1), _exact(s, "gate", rpg=7, in_place=True), _exact(s, "gate", rpg=s[0] + 3),
    _exact(s, "gate", bias=False, rpg=7),
    _exact(s, out="mx"), _exact(s, out="mx", bias=False))]
# one of each at five K-tiles (2 x 2 tiles), the weight taking the one-hot role
EXACT_CASES += [_exact((300, 288, 640), one_hot="w"), _exact((300, 288, 640), "residual", in_place=True, one_hot="w"),
                _exact((300, 288, 640), "gate", rpg=7, one_hot="w"), _exact((300, 288, 640), out="mx", one_hot="w")]


def exact_id(c):
    return ("x".join(map(str, c["shape"])) + f"-{c['epi']}-{'bias' if c['bias'] else 'nobias'}-{c['out']}"
            + ("-inplace" if c["in_place"] else "") + (f"-rpg{c['rpg']}" if c["rpg"] else ""))


QUANT_ROWS, QUANT_K = (1, 37, 300), (32, 64, 2080)
QUANT_FAMILIES = ["plain", "row_scales", "witnesses"]

# largest (|restate - truth| - 2^-8 |truth|) / mag per epilogue over SLACK_CASES (measure_excess); SLACK = 4 x the largest
# (with K = 128: at most 9.3e-9 (gate), 8.6e-9 (gelu) and 0 there; the largest stay those of K = 8192).  The fp32 matmul's order
# of summation at K = 8192 follows the CPU BLAS's blocking, so "none" and "residual" move with the thread count: re-measured
# with 1, 4, 8 and 16 threads on two hosts, none 1.133e-9 .. 1.366e-9, residual 6.93e-9 .. 8.25e-9 (gate 1.515e-8 and gelu 1.375e-8
# on all of them); the figures are the largest.  SLACK rests on the gate's, which did not move.
MEASURED_EXCESS_BY_EPI = {"none": 1.37e-9, "gelu": 1.38e-8, "gate": 1.52e-8, "residual": 8.25e-9}
MEASURED_EXCESS = max(MEASURED_EXCESS_BY_EPI.values())
SLACK = 4.0 * MEASURED_EXCESS
SLACK_MN = (200, 288)
SLACK_CASES = sorted({(c["family"], c["epi"], c["shape"][2]) for c in GEMM_CASES + MXOUT_CASES})


def case_id(c):
    return "x".join(map(str, c["shape"])) + f"-{c['family']}-{c['epi']}"


# ----------------------------------------------------------------------------------------------- the format
def _e_from_k_m(k, m_le_175, zero):
    e = torch.where(m_le_175, k - 8, k - 7).clamp(-127, 127)
    return torch.where(zero, torch.zeros_like(e), e + 127).to(torch.uint8)


def scale_bytes_bf16(x):
    """x [rows, K] bf16 -> uint8 [rows, K / 32], from the bit patterns alone."""
    rows, K = x.shape
    assert x.dtype == BF and K % BLOCK == 0
    bits = (x.contiguous().view(torch.int16).to(torch.int32) & 0x7fff).reshape(rows, K // BLOCK, BLOCK).amax(dim=-1)
    E, frac = bits >> 7, bits & 0x7f
    # a subnormal (E = 0, frac > 0) is frac * 2^-133: its leading bit p gives k = p - 133 and the mantissa frac << (7 - p)
    p = torch.zeros_like(frac)
    for b in range(1, 7):
        p = torch.where(frac >= (1 << b), torch.full_like(p, b), p)
    sub = E == 0
    k = torch.where(sub, p - 133, E - 127)
    mant = torch.where(sub, (frac << (7 - p)) & 0x7f, frac)
    return _e_from_k_m(k, mant <= 0x60, bits == 0)


def scale_bytes_real(v):
    """v [rows, N] of any real dtype -> uint8 [rows, N / 32]: the same rule through frexp (amax = f * 2^x, f in [0.5, 1))."""
    rows, N = v.shape
    amax = v.to(F64).abs().reshape(rows, N // BLOCK, BLOCK).amax(dim=-1)
    f, x = torch.frexp(amax)
    return _e_from_k_m(x.to(torch.int32) - 1, f <= 0.875, amax == 0)


def quantize_elements(v, scales):
    """v [rows, K] real, scales uint8 [rows, K / 32] -> float8_e4m3fn [rows, K] = RNE(v * 2^-e)."""
    e = (scales.to(torch.int32) - 127).repeat_interleave(BLOCK, dim=-1)
    return torch.ldexp(v.to(F64), -e).to(torch.float32).to(E4M3)


def quantize(x):
    """bf16 [rows, K] -> (q float8_e4m3fn [rows, K], scales uint8 [rows, K / 32]): what ltxmi_quantize_mx8_bf16 must give."""
    s = scale_bytes_bf16(x)
    return quantize_elements(x, s), s


def dequantize(q, scales, dt=F64):
    e = (scales.to(torch.int32) - 127).repeat_interleave(BLOCK, dim=-1)
    return torch.ldexp(q.view(E4M3).to(dt), e)


# the exponent-rule witnesses: (block amax as a bf16 value, e, the element that value becomes)
WITNESSES = [(448.0, 0, 448.0), (450.0, 1, 224.0), (1.0, -8, 256.0), (0.0, -127, 0.0), (2.0 ** -130, -127, 2.0 ** -3),
             (3e38, 120, 224.0), (1.75, -8, 448.0), (1.7578125, -7, 224.0), (2.0 ** -126, -127, 2.0), (2.0 ** -120, -127, 128.0)]


def witness_rows(K):
    """bf16 [len(WITNESSES) + 2, K]: row i holds witness i as the amax of every block, among smaller values of both signs; the
    last two rows are element-rounding rows (ties and e4m3 subnormals under amax 256 -> e = 0)."""
    rows = []
    for amax, _, _ in WITNESSES:
        r = torch.tensor(amax).to(BF).to(F64) * torch.linspace(-0.9, 0.9, K, dtype=F64)
        r[5::BLOCK] = amax
        r[9::BLOCK] = -amax / 2
        rows.append(r)
    ties = torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -9, 0.0009765625 * 0.99, 17.0, 19.0, 21.0, 1.0625, 1.1875,
                         -1.0625, -1.1875, 240.0, 232.0, 248.0, -0.0], dtype=F64)
    for sign in (1.0, -1.0):
        r = (sign * ties).repeat((K + 15) // 16)[:K].clone()
        r[7::BLOCK] = 256.0
        rows.append(r)
    return torch.stack(rows).to(BF)


def quant_input(family, rows, K, seed=0):
    g = torch.Generator().manual_seed(4100 + seed)
    if family == "witnesses":
        w = witness_rows(K)
        return w.repeat((rows + w.shape[0] - 1) // w.shape[0], 1)[:rows].contiguous()     # (rows = 1: the amax-448 row alone)
    x = torch.randn(rows, K, generator=g)
    if family == "row_scales":
        x = x * 10.0 ** (torch.rand(rows, 1, generator=g) * 6 - 3)
    return x.to(BF)


# ----------------------------------------------------------------------------------------------- GEMM inputs and truth
def make(family, M, N, K, epi="none", device="cpu", seed=0):
    """gemm_cases.make's tensors with ``a`` and ``w`` quantised: dict(aq, a_scales, wq, w_scales, a, w (the de-quantised operands,
    float64), bias, [gate_table, gate_temb, residual], rows_per_group) on ``device``."""
    d = gemm_cases.make("plain" if family == "cancel" else family, M, N, K, epi, bias=True, device=device, seed=seed)
    for n in ("a", "w"):
        d[n + "q"], d[n + "_scales"] = quantize(d[n])
        d[n] = dequantize(d[n + "q"], d[n + "_scales"])
    if family == "cancel":
        acc = d["a"] @ d["w"].T
        cols = torch.arange(N, device=device)
        d["bias"] = (-acc[(7 * cols + 3) % M, cols]).to(BF)
        if epi in ("gate", "residual"):
            v = acc + d["bias"].to(F64)
            if epi == "gate":
                v = v * gemm_cases.gate_rows(d, M, F64)
            d["residual"] = (-v).to(BF)
    return d


def product(d, dt=F64):
    """(acc, mag) = (a . w^T, |a| . |w|^T) of the de-quantised operands in ``dt``: shared by the epilogues of a (family, shape)."""
    a, w = d["a"].to(dt), d["w"].to(dt)
    return a @ w.T, a.abs() @ w.abs().T


TRUNC = 2.0 ** -10


def trunc_mag(d):
    """[M, N] float64: sum over the groups of 8 consecutive k of max |a| * max |w| in the group (see TRUNC)."""
    g = lambda t: t.abs().reshape(t.shape[0], -1, 8).amax(dim=-1)
    return g(d["a"]) @ g(d["w"]).T


def eff_mag(mag, tmag):
    """The mag to hand to gemm_cases.compare with slack=SLACK: SLACK * eff_mag = SLACK * mag + TRUNC * tmag."""
    return mag + (TRUNC / SLACK) * tmag


def witness_truncation():
    """Exact rows for the scaled MFMA's in-group cut -> (aq, a_scales, wq, w_scales, residual bf16, expected [rows] after the
    cancellation as the hardware gives it, exact [rows] as real arithmetic gives it).  K = 128, N = 32, all scales 2^0;
    w[n, 0] = 256, w = 1 elsewhere.  Rows: n ones at k = 1..n beside a[0] = 256 (n = 0..31); 8 ones at k = 8..15; 31 ones in
    block 1; 31 ones beside a[0] = 32 (2^13)."""
    K, N = 128, 32
    rows, hw, exact, big = [], [], [], []
    def add(a0, ks, want):
        r = torch.zeros(K, dtype=F64)
        r[0] = a0
        r[ks] = 1.0
        rows.append(r); hw.append(float(want)); exact.append(float(len(ks))); big.append(a0 * 256.0)
    for n in range(32):
        add(256.0, list(range(1, 1 + n)), max(0, n - 7))
    add(256.0, list(range(8, 16)), 8)
    add(256.0, list(range(32, 63)), 31)
    add(32.0, list(range(1, 32)), 31)
    a = torch.stack(rows)
    w = torch.ones(N, K, dtype=F64)
    w[:, 0] = 256.0
    ones = lambda n: torch.full((n, K // BLOCK), 127, dtype=torch.uint8)
    resid = (-torch.tensor(big, dtype=F64))[:, None].expand(len(rows), N).to(BF).contiguous()
    return (a.to(torch.float32).to(E4M3), ones(len(rows)), w.to(torch.float32).to(E4M3), ones(N), resid,
            torch.tensor(hw, dtype=F64), torch.tensor(exact, dtype=F64))


def witness_mx_out_threshold():
    """fp32 accumulators at the thresholds of the MX-output scale rule (mx8_scale_byte on fp32 bits switches on
    mantissa > 0x600000, that is amax > 1.75 * 2^k) -> dict(aq, a_scales, wq, w_scales, residual bf16 [rows, N] that cancels the
    large term, values float64 [rows] (what every output of the row is), after float64 [rows] (values + residual, exact in bf16),
    scales uint8 [rows, 1] and q float8_e4m3fn [rows, N]: the restated rule on the float64 values).  K = 128, N = 32, all input scales
    2^0, w[n, 0] = 1 and w[n, 8] = 2^-4 for every n.  A row is one product a[0] * 1 plus, for the addend, a[8] * 2^-4: k = 8 lies in
    another group of 8, where ``witness_truncation`` establishes that nothing is cut.  Rows: 448, 448.5, 447.5, 1.75, 1.75 + 2^-7,
    and an all-zero row."""
    K, N = 128, 32
    rows = [(448.0, 0.0), (448.0, 8.0), (448.0, -8.0), (1.75, 0.0), (1.75, 0.125), (0.0, 0.0)]
    a = torch.zeros(len(rows), K, dtype=F64)
    a[:, 0] = torch.tensor([r[0] for r in rows], dtype=F64)
    a[:, 8] = torch.tensor([r[1] for r in rows], dtype=F64)
    w = torch.zeros(N, K, dtype=F64)
    w[:, 0], w[:, 8] = 1.0, 2.0 ** -4
    aq, wq = a.to(torch.float32).to(E4M3), w.to(torch.float32).to(E4M3)
    assert bool((aq.to(F64) == a).all()) and bool((wq.to(F64) == w).all())
    ones = lambda n: torch.full((n, K // BLOCK), 127, dtype=torch.uint8)
    values = (a @ w.T)[:, 0].clone()
    resid = (-a[:, :1] * w[:1, 0]).expand(len(rows), N).to(BF).contiguous()
    after = values + resid[:, 0].to(F64)
    full = values[:, None].expand(len(rows), N).contiguous()
    scales = scale_bytes_real(full)
    return dict(aq=aq, a_scales=ones(len(rows)), wq=wq, w_scales=ones(N), residual=resid, values=values, after=after,
                scales=scales, q=quantize_elements(full, scales))


def epilogue_op(d, epi, acc, mag):
    """tests/gemm_cases.py::gemm_op from the product on, in the product's dtype -> (value, mag)."""
    dt, M = acc.dtype, acc.shape[0]
    acc, mag = acc + d["bias"].to(dt), mag + d["bias"].to(dt).abs()
    if epi == "gelu":
        acc = torch.nn.functional.gelu(acc, approximate="tanh")
    elif epi == "gate":
        acc = acc * gemm_cases.gate_rows(d, M, dt)
        idx = torch.arange(M, device=acc.device) // d["rows_per_group"]
        mag = mag * (d["gate_table"].to(dt).abs()[None, :] + d["gate_temb"].to(dt).abs()[idx])
    if epi in ("gate", "residual"):
        acc, mag = acc + d["residual"].to(dt), mag + d["residual"].to(dt).abs()
    return acc, mag


def restate(d, epi):
    """fp32 arithmetic on the de-quantised operands, one rounding to bf16."""
    return epilogue_op(d, epi, *product(d, torch.float32))[0].to(BF)


def measure_excess(cases=None):
    """{epilogue: largest (|restate - truth| - 2^-8 |truth|) / mag} over SLACK_CASES at M x N = SLACK_MN (CPU)."""
    M, N = SLACK_MN
    worst = {}
    for family, epi, K in (SLACK_CASES if cases is None else cases):
        d = make(family, M, N, K, epi)
        t, mag = epilogue_op(d, epi, *product(d))
        r = restate(d, epi).to(F64)
        worst[epi] = max(worst.get(epi, 0.0), float((((r - t).abs() - 2.0 ** -8 * t.abs()) / mag).max()))
    return worst


# ----------------------------------------------------------------------------------------------- the MX-output metric
THRESHOLD_REL = 2.0 ** -7


def mx_out_figures(q, scales, truth, mag, slack=SLACK):
    # (mag: eff_mag(...) on the device, plain mag for the CPU restatement)
    """The MX-output epilogue against the float64 truth g (after the activation).
      scales  the stored byte equals ``scale_bytes_real(truth)``, or differs from it by one where the truth's block amax is within
              2^-7 (relative) of a threshold 1.75 * 2^k of the rule;
      values  |dequantize(q, scales) - g| <= max(2^-4 |g|, 2^(e - 10)) + slack * mag with e the STORED exponent (half an e4m3 ulp of
              a normal, half the subnormal spacing 2^-9, both times 2^e).
    -> dict(scale_bad: blocks outside the first rule, elem: the worst value error as a fraction of its limit)."""
    t = truth.to(F64)
    want = scale_bytes_real(t).to(torch.int32)
    got = scales.to(torch.int32)
    amax = t.abs().reshape(t.shape[0], -1, BLOCK).amax(dim=-1)
    f, _ = torch.frexp(amax)
    near = ((f / 0.875 - 1).abs() <= THRESHOLD_REL) & (amax > 0)
    ok = (got == want) | (((got - want).abs() == 1) & near)
    e = (got - 127).repeat_interleave(BLOCK, dim=-1)
    lim = torch.maximum(2.0 ** -4 * t.abs(), torch.ldexp(torch.ones_like(t), e - 10)) + slack * mag.to(F64)
    err = (dequantize(q, scales) - t).abs()
    return dict(scale_bad=int((~ok).sum()), elem=float((err / lim).max()))


# ----------------------------------------------------------------------------------------------- the layout probe
def strided_operands(aq, a_s, wq, w_s, device="cpu"):
    """The four operands as views inside NaN-filled buffers (elements 0x7f, scales 0xff) -> (views, buffers):
      aq        lda = K + 16, a guard row before and after;
      a_scales  lda_s = K / 32 + 4, from byte 4 of its buffer: 4-byte but not 16-byte aligned;
      wq, w_s   rows [5, 5 + N) of arrays of N + 9 rows.
    The element views are float8_e4m3fn, the buffers uint8."""
    M, K = aq.shape
    N, kb = wq.shape[0], K // BLOCK
    u8 = lambda t: t.view(torch.uint8).to(device)
    lda, lda_s = K + 16, kb + 4
    abuf = torch.full(((M + 2) * lda,), 0x7f, dtype=torch.uint8, device=device)
    torch.as_strided(abuf, (M, K), (lda, 1), lda).copy_(u8(aq))
    asbuf = torch.full((4 + (M + 1) * lda_s,), 0xff, dtype=torch.uint8, device=device)
    a_sv = torch.as_strided(asbuf, (M, kb), (lda_s, 1), 4)
    a_sv.copy_(u8(a_s))
    wbuf = torch.full((N + 9, K), 0x7f, dtype=torch.uint8, device=device)
    wbuf[5:5 + N].copy_(u8(wq))
    wsbuf = torch.full((N + 9, kb), 0xff, dtype=torch.uint8, device=device)
    wsbuf[5:5 + N].copy_(u8(w_s))
    views = (torch.as_strided(abuf.view(E4M3), (M, K), (lda, 1), lda), a_sv, wbuf.view(E4M3)[5:5 + N], wsbuf[5:5 + N])
    return views, (abuf, asbuf, wbuf, wsbuf)


def probe(M, N, K, one_hot="a", scales="varied", geometry="contiguous", device="cpu"):
    """Exact data for the lane maps: one operand one-hot per row (a 1 at k = (37 r + 11) mod K), the other asymmetric small
    integers ((7 r + 3 k) mod 15 - 7), and power-of-two scales:
      "varied"  a different one in every block of every row on both sides, exponents -6 .. 6 and -5 .. 5;
      "flat"    2^0 everywhere: every output is an integer in -7 .. 7;
      "wide"    A byte 1 + floor(247 b / (K / 32 - 1)) + r mod 6 for block b (1 .. 253), W byte 253 - that floor - c mod 6
                (1 .. 253): ea + ew = r mod 6 - c mod 6.  K >= 512, so that at least 16 blocks spread the bytes.  Byte 255 (the
                E8M0 NaN) is left out.
    Every output is one product +-int * 2^(ea + ew), exact in bf16.  ``geometry="strided"``: the same operands as the views
    of ``strided_operands``.  -> (aq, a_scales, wq, w_scales, expected bf16 [M, N]) on ``device``."""
    def hot(R):
        x = torch.zeros(R, K, dtype=F64)
        x[torch.arange(R), (37 * torch.arange(R) + 11) % K] = 1.0
        return x

    def ints(R):
        r, k = torch.arange(R)[:, None], torch.arange(K)[None, :]
        return ((7 * r + 3 * k) % 15 - 7).to(F64)

    def varied(R, mul, mod, off):
        r, b = torch.arange(R)[:, None], torch.arange(K // BLOCK)[None, :]
        return ((mul * r + 5 * b) % mod - off + 127).to(torch.uint8)

    def wide(R, side):
        assert K // BLOCK >= 16
        r, b = torch.arange(R)[:, None], torch.arange(K // BLOCK)[None, :]
        base = (247 * b) // (K // BLOCK - 1)
        return (1 + base + r % 6 if side == "a" else 253 - base - r % 6).to(torch.uint8)

    a, w = (hot(M), ints(N)) if one_hot == "a" else (ints(M), hot(N))
    aq, wq = a.to(torch.float32).to(E4M3), w.to(torch.float32).to(E4M3)
    if scales == "varied":
        a_s, w_s = varied(M, 3, 13, 6), varied(N, 1, 11, 5)
    elif scales == "flat":
        a_s, w_s = (torch.full((R, K // BLOCK), 127, dtype=torch.uint8) for R in (M, N))
    else:
        assert scales == "wide"
        a_s, w_s = wide(M, "a"), wide(N, "w")
    exp = dequantize(aq, a_s) @ dequantize(wq, w_s).T
    assert bool((exp.to(BF).to(F64) == exp).all())
    if geometry == "strided":
        return strided_operands(aq, a_s, wq, w_s, device)[0] + (exp.to(BF).to(device),)
    assert geometry == "contiguous"
    return tuple(t.to(device) for t in (aq, a_s, wq, w_s, exp.to(BF)))


# ----------------------------------------------------------------------------------------------- exact epilogue cases
GATE_SUMS = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)


def exact(c, device="cpu"):
    """An EXACT_CASES entry -> dict(aq, a_scales, wq, w_scales, bias | None, [residual], [gate_table, temb_full, gate_temb],
    rows_per_group, truth float64 [M, N], partials: every intermediate value in float64) on ``device``.  The operands are the
    flat probe's; bias[n] = 5 n mod 17 - 8; residual[r, n] = (11 r + 7 n) mod 65 - 32; the gate sum of (group g, column n) is
    GATE_SUMS[(3 g + 5 n) mod 7], split into gate_table[n] = (n mod 3 - 1) / 2 and the rest in columns [2 N, 3 N) of a
    [groups, 6 N] array whose other columns hold 64."""
    M, N, K = c["shape"]
    aq, a_s, wq, w_s, want = probe(M, N, K, c["one_hot"], scales="flat")
    d = dict(aq=aq, a_scales=a_s, wq=wq, w_scales=w_s, bias=None, rows_per_group=c["rpg"] or 1)
    r, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    v = want.to(F64)
    partials = [v]
    if c["bias"]:
        d["bias"] = ((5 * n[0]) % 17 - 8).to(BF)
        v = v + d["bias"].to(F64)
        partials.append(v)
    if c["epi"] == "gate":
        rpg = c["rpg"]
        groups = (M + rpg - 1) // rpg
        g = torch.arange(groups)[:, None]
        sums = torch.tensor(GATE_SUMS, dtype=F64)[(3 * g + 5 * n) % 7]
        d["gate_table"] = ((n[0] % 3 - 1) / 2).to(BF)
        d["temb_full"] = torch.full((groups, 6 * N), 64.0, dtype=BF)
        d["temb_full"][:, 2 * N:3 * N] = (sums - d["gate_table"].to(F64)).to(BF)
        d["gate_temb"] = d["temb_full"][:, 2 * N:3 * N]
        gate = gemm_cases.gate_rows(d, M, F64)
        v = v * gate
        partials += [gate, v]
    if c["epi"] in ("gate", "residual"):
        d["residual"] = ((11 * r + 7 * n) % 65 - 32).to(BF)
        v = v + d["residual"].to(F64)
        partials.append(v)
    d = {k: (t.to(device) if torch.is_tensor(t) else t) for k, t in d.items()}
    if "temb_full" in d:
        d["gate_temb"] = d["temb_full"][:, 2 * N:3 * N]
    d.update(truth=v, partials=partials)
    return d


def exact_ok(d, out="bf16"):
    """The exact cases' condition: every partial result a multiple of 0.5 below 2^24 in magnitude, the gate sums among GATE_SUMS,
    and the truth representable in the output format."""
    t = d["truth"]
    ok = all(bool((p * 2 == (p * 2).round()).all()) and float(p.abs().max()) < 2.0 ** 24 for p in d["partials"])
    if "gate_temb" in d:
        ok = ok and set(gemm_cases.gate_rows(d, t.shape[0], F64).unique().tolist()) <= set(GATE_SUMS)
    if out == "mx":
        s = scale_bytes_real(t)
        return ok and bool((t == t.round()).all()) and float(t.abs().max()) <= 15 and \
            bool((dequantize(quantize_elements(t, s), s) == t).all())
    return ok and bool((t.to(BF).to(F64) == t).all())


# ----------------------------------------------------------------------------------------------- guarded outputs
# kind -> (the dtype the pattern is written in, the pattern, the dtype of the view handed to the kernel)
GUARDS = {"bf16": (torch.int16, 0x7fa5, BF),                  # a bf16 NaN
          "e4m3": (torch.uint8, 0x7f, torch.uint8),           # the e4m3fn NaN
          "scale": (torch.uint8, 0xff, torch.uint8),          # the E8M0 NaN
          "f32": (torch.int32, 0x7fc05a5a, torch.float32)}    # an fp32 NaN


def guarded(rows, cols, pad, kind, device):
    """A [rows, cols] view with row stride cols + pad inside a buffer filled with the kind's pattern, a guard row before and after
    -> (buf: the flat buffer in the pattern's integer dtype, view)."""
    bits, pattern, dtype = GUARDS[kind]
    ld = cols + pad
    buf = torch.full(((rows + 2) * ld,), pattern, dtype=bits, device=device)
    return buf, torch.as_strided(buf.view(dtype), (rows, cols), (ld, 1), ld)


def guard_figures(buf, view, kind):
    """-> (patterns left inside the view, elements changed outside it)."""
    pattern = GUARDS[kind][1]
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    torch.as_strided(inside, view.shape, view.stride(), view.storage_offset()).fill_(True)
    hit = buf == pattern
    return int((hit & inside).sum()), int((~hit & ~inside).sum())
