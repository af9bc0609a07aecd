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
(2048, 4096, 8192): the FF2 form, 64 K-tiles, 128 tiles.  (1, 288, 256) and (1, 4096, 8192): M = 1."""
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
PROBE_SHAPES = [SMALL, (520, 544, 384)]               # the second: 3 x 3 tiles, three K-tiles (a refill into either stage)

QUANT_ROWS, QUANT_K = (1, 37, 300), (32, 64, 2080)
QUANT_FAMILIES = ["plain", "row_scales", "witnesses"]

# largest (|restate - truth| - 2^-8 |truth|) / mag per epilogue over SLACK_CASES (measure_excess); SLACK = 4 x the largest
MEASURED_EXCESS_BY_EPI = {"none": 1.14e-9, "gelu": 1.38e-8, "gate": 1.52e-8, "residual": 6.93e-9}
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
def probe(M, N, K, one_hot="a"):
    """Exact data for the lane maps: one operand one-hot per row (a 1 at k = (37 r + 11) mod K), the other asymmetric small
    integers ((7 r + 3 k) mod 15 - 7), and a different power-of-two scale in every block of every row on both sides.  Every
    output is one product +-int * 2^(ea + ew), exact in bf16.  -> (aq, a_scales, wq, w_scales, expected bf16 [M, N])."""
    def hot(R):
        x = torch.zeros(R, K, dtype=F64)
        x[torch.arange(R), (37 * torch.arange(R) + 11) % K] = 1.0
        return x

    def ints(R):
        r, k = torch.arange(R)[:, None], torch.arange(K)[None, :]
        return ((7 * r + 3 * k) % 15 - 7).to(F64)

    def scales(R, mul, mod, off):
        r, b = torch.arange(R)[:, None], torch.arange(K // BLOCK)[None, :]
        return ((mul * r + 5 * b) % mod - off + 127).to(torch.uint8)

    a, w = (hot(M), ints(N)) if one_hot == "a" else (ints(M), hot(N))
    aq, wq = a.to(torch.float32).to(E4M3), w.to(torch.float32).to(E4M3)
    a_s, w_s = scales(M, 3, 13, 6), scales(N, 1, 11, 5)
    exp = dequantize(aq, a_s) @ dequantize(wq, w_s).T
    assert bool((exp.to(BF).to(F64) == exp).all())
    return aq, a_s, wq, w_s, exp.to(BF)
