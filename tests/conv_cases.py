"""Shapes, inputs, float64 truths and metrics for ltxmi_conv3d_ndhwc_bf16 -- TEST INFRASTRUCTURE ONLY (plain module, no GPU).

Shared by tests/test_conv_cases.py (CPU) and tests/test_gpu_conv_paths.py (MI355X).

CASES.  Every case names the route it must take (``want``: route, epilogue, ksplit, swap_hw, finalize_blocks of
ltxmi_conv3d_route_info, include/ltxmi.h); the CPU file pins each through ``ops.conv3d_route`` and the GPU file asserts it
before it launches.  The shapes are the smallest found with the route query that reach each path: see the comments at the lists.

TRUTH (``conv_op``): generic over the dtype it runs in -- float64 is the truth, float32 followed by ONE rounding to bf16
(``restate``) is what a correct fp32-accumulating implementation of the header gives.  Padding as oracle/vae.py::causal_conv3d
and oracle/vae_encoder.py::strided_causal_conv3d / space_to_depth_downsample have it: ``front`` frames in front of the input
(tpad, or 2 causal / 1 otherwise), behind it what the output frames need (1 when not causal), the first / last frame repeated or
zeros (time_pad_zeros); space padded by 1, zeros or replicate; nn.Conv3d arithmetic with the strides.  kernel_t = 1 is F.conv2d
per frame and the plain time_pad_zeros call is F.conv3d(padding=1 in time).  The depth-to-space store is oracle/vae.py::
depth_to_space_upsample on weight rows in the packed (p1 p2 p3, c') order.  It returns (value, mag), NDHWC, with
  mag = conv(|x|, |w|) + |bias| + |add|     (depth-to-space: + |residual|).
tests/test_conv_cases.py pins its indexing against an element-by-element loop for every mode.
post_norm: ``norm_op`` is tests/norm_cases.py::pixelnorm_op (value and mag taken through the norm).  As the ONLY output it is
computed from the unrounded result; as the SECOND output (y_norm) it is the norm of the raw output's own bf16 values, which are
judged by themselves.

INPUT FAMILIES (``make``): seeded, rounded to bf16 before anything is computed from them.
  plain       x ~ randn, w ~ randn * K^-1/2, bias ~ randn, add ~ randn, scale / shift ~ 0.3 randn
  exact       x, bias integers in -4 .. 4, add in -8 .. 8; w ternary: for output channel co, tap and 32-channel chunk q with
              (co + tap + q) mod S == 0 one weight +-1 at channel 32 q + (7 co + 3 tap + 5 q) mod 32 -- every tap and every chunk
              contributes, through a different input channel; S keeps an output at <= 48 terms.  CONDITION (``exact_ok``,
              asserted on the CPU for every case of the family): every element of the float64 truth is an integer of magnitude
              <= 256.  Then every product and partial sum is an integer below 2^24, any fp32 summation order is exact, bf16 holds
              the result exactly, and the GPU output must EQUAL the truth bit for bit: a dropped chunk, a wrong halo row, a wrong
              pad mode at one corner, a channel range summed twice or not at all -- zero tolerance.  (Computed in fp32 on the CPU.)
  cancel      `add` only: add = bf16(-(conv + bias)) from float64, so the output is the rounding residue of the accumulator.
              An epilogue that rounds to bf16 before it adds fails it.
  row_scales  position p of x multiplied by 10 ** u_p, u_p uniform in [-3, 3]

METRICS (``compare``): a case must meet all three.
  (a) ``check`` of tests/test_gpu_kernels.py on the whole tensor (REL_L2 3e-3, MAXREL 1.6e-2; imported, not copied).
  (b) The same two figures per (sample, frame, 8 x 16 spatial tile, 128-channel block) in both orientations (8 along H and 16
      along W, and the other way round), for blocks of at least 64 values: one wrong tile stands out.
  (c) Per element |out - truth| <= 2^-7 |truth| + SLACK * mag; elements with |truth| < 1e-30 are skipped.

SLACK.  Measured on the CPU (``measure_excess``; tests/test_conv_cases.py re-measures and pins it) as the largest
(|restate - truth| - 2^-8 |truth|) / mag over every (family, epilogue, K = 9 kt Cin) the GPU file uses (``SLACK_CASES``) at
2 x 3 x 5 x 7 positions: per epilogue MEASURED_EXCESS_BY_EPI below, the largest 1.8e-7 (3 x 2^-24: `add` in the cancel family at
K = 27648, where fp32 rounds the accumulator the residue is taken from), so SLACK = 4 x 1.8e-7 = 7.2e-7 for every epilogue: 4 times, because the GPU sums K in another order (taps and 32-wide MFMA steps)
than torch's fp32 convolution, and its exp / rsqrt / rcp are good to about one fp32 ulp -- the margin and the reasoning of
tests/gemm_cases.py.  Nothing in it comes from a kernel.

CONDITION on the cases: the fp32 restatement alone meets all three metrics on every (family, epilogue, K) used on the GPU.
What cannot is listed in ``DROPPED`` with the figure it misses (at most one family per epilogue, never ``exact``): nothing is."""
import functools

import torch
import torch.nn.functional as F

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

FAMILIES = ["plain", "exact", "cancel", "row_scales"]
# epilogues as the truth sees them; "only" / "second": the activated result as the only / as a second output
EPIS = ["none", "add", "d2s", "d2s_res"]
GEMM128, GEMM256, DIRECT8, DIRECT4 = 0, 1, 2, 3

# largest (|restate - truth| - 2^-8 |truth|) / mag per epilogue over SLACK_CASES (measure_excess); SLACK = 4 x the largest
MEASURED_EXCESS_BY_EPI = {"none": 3.7e-8, "add": 1.8e-7, "d2s": 3.8e-8, "d2s_res": 4.1e-8,
                          "none+only": 8.8e-9, "add+second": 2.0e-8, "d2s+second": 0.0, "d2s_res+second": 1.1e-8}
MEASURED_EXCESS = max(MEASURED_EXCESS_BY_EPI.values())
SLACK_TIMES = 4.0
SLACK = SLACK_TIMES * MEASURED_EXCESS

# (family, epilogue) pairs the fp32 restatement itself cannot pass, with the metric it misses
DROPPED = {}


# ---------------------------------------------------------------------------------------------------------- cases
def _case(grid, cin, cout, want, epi="none", family="exact", causal=True, replicate=True, tzero=False, stride=(1, 1, 1),
          tpad=0, out_T=0, kernel_t=3, bias=True, algo=0, norm=None, judge="whole", versus=None):
    """grid = (B, T, H, W); want = (route, epilogue, ksplit, swap_hw, finalize_blocks); norm: None / "only" / "second";
    judge: "whole" (float64 truth of the whole tensor) or "crops" (float64 corner crops; the whole tensor against the call with
    algo = versus where another route takes the shape)."""
    B, T, H, W = grid
    return dict(B=B, T=T, H=H, W=W, Cin=cin, Cout=cout, epi=epi, family=family, causal=causal, replicate=replicate, tzero=tzero,
                stride=stride, tpad=tpad, out_T=out_T, kernel_t=kernel_t, bias=bias, algo=algo, norm=norm, judge=judge,
                versus=versus, want=dict(zip(("route", "epilogue", "ksplit", "swap_hw", "finalize_blocks"), want)))


def case_id(c):
    s = f"{c['B']}x{c['T']}x{c['H']}x{c['W']}-{c['Cin']}to{c['Cout']}-{c['epi']}-{c['family']}"
    s += ("-causal" if c["causal"] else "") + ("-repl" if c["replicate"] else "-zeros") + ("-tzero" if c["tzero"] else "")
    if c["stride"] != (1, 1, 1):
        s += "-s" + "".join(map(str, c["stride"]))
    for k in ("tpad", "out_T"):
        if c[k]:
            s += f"-{k}{c[k]}"
    if c["kernel_t"] != 3:
        s += "-kt1"
    if not c["bias"]:
        s += "-nobias"
    if c["norm"]:
        s += "-" + c["norm"]
    if c["judge"] != "whole":
        s += "-" + c["judge"]
    w = c["want"]
    return s + f"-algo{c['algo']}-r{w['route']}e{w['epilogue']}k{w['ksplit']}s{w['swap_hw']}f{w['finalize_blocks']}"


def _families(fams, *a, **k):
    return [_case(*a, family=f, **k) for f in fams]


EP = ("exact", "plain")
ADD = ("exact", "plain", "cancel", "row_scales")
G128 = (GEMM128, 0, 1, 0, 0)

# The implicit GEMM with 128 x 128 tiles: what the direct convolution does not take (strides, tpad / out_T, kernel_t 1, no
# bias, depth-to-space off 1024 channels) and grids of fewer than 128 direct tiles.  105 positions: M ragged against 128.
GEMM128_CASES = (
    [c for co in (8, 136, 264) for c in _families(EP, (1, 3, 5, 7), 64, co, G128, causal=co != 136, replicate=co != 264)]
    + [_case((2, T, H, W), 64, 136, G128, stride=s, replicate=r)
       for s in ((2, 1, 1), (1, 2, 2), (2, 2, 2)) for (T, H, W), r in (((5, 7, 9), True), ((4, 6, 8), False))]
    + [_case((2, 5, 7, 9), 128, 136, G128, stride=s, family="plain", replicate=False) for s in ((2, 1, 1), (1, 2, 2), (2, 2, 2))]
    # SpaceToDepthDownsample's form: the first frame once more in front (tpad 3 causal / 2 otherwise), T + 1 output frames
    + _families(EP, (2, 4, 5, 7), 64, 72, G128, tpad=3, out_T=5)
    + _families(EP, (1, 4, 5, 7), 64, 72, G128, causal=False, tpad=2, out_T=5, replicate=False)
    + _families(EP, (2, 3, 5, 7), 128, 136, G128, kernel_t=1, causal=False)
    + _families(EP, (2, 3, 5, 7), 64, 264, G128, kernel_t=1, causal=False, replicate=False)
    + _families(EP, (2, 3, 5, 7), 64, 136, G128, tzero=True, causal=False, replicate=False)
    + _families(EP, (1, 2, 4, 6), 128, 136, G128, tzero=True, causal=False)
    + _families(EP, (2, 3, 5, 7), 64, 136, G128, bias=False)                      # the zero page stands in for the bias
    + _families(ADD, (2, 3, 5, 7), 128, 136, (GEMM128, 1, 1, 0, 0), epi="add", causal=False)
    + _families(EP, (2, 3, 5, 7), 64, 320, (GEMM128, 2, 1, 0, 0), epi="d2s")       # 40 channels out: (p1 p2 p3) blocks off every tile edge
    + _families(EP, (2, 3, 5, 7), 64, 320, (GEMM128, 2, 1, 0, 0), epi="d2s_res", causal=False, replicate=False)
    + _families(EP, (1, 2, 4, 6), 64, 128, (GEMM128, 2, 1, 0, 0), epi="d2s_res")   # reduction 4: every residual channel used twice
)

# The implicit GEMM with 256 x 256 tiles: Cout >= 256 and ceil(M / 256) ceil(Cout / 256) >= 384 on a call the direct convolution
# does not take.  Cout 264 / 320: the last column tile is 8 / 64 wide; M = 3 x 129 x 127 = 49149 = 191 x 256 + 253: the last row
# tile is partial (192 x 2 = 384 tiles exactly).
BIG = (1, 3, 129, 127)
G256 = (GEMM256, 0, 1, 0, 0)
GEMM256_CASES = (
    [_case(BIG, 64, 264, G256, algo=1), _case(BIG, 64, 264, G256, algo=1, family="plain", judge="crops", versus=4),
     _case(BIG, 64, 264, (GEMM256, 1, 1, 0, 0), algo=1, epi="add", causal=False),
     _case(BIG, 64, 264, (GEMM256, 1, 1, 0, 0), algo=1, epi="add", causal=False, family="plain", judge="crops", versus=4),
     _case(BIG, 64, 320, (GEMM256, 2, 1, 0, 0), algo=1, epi="d2s_res", replicate=False),
     _case(BIG, 64, 320, (GEMM256, 2, 1, 0, 0), algo=1, epi="d2s_res", replicate=False, family="plain", judge="crops"),
     _case((1, 3, 257, 254), 64, 264, G256, stride=(1, 2, 2)),                   # 3 x 129 x 127 positions out
     _case((1, 3, 257, 254), 64, 264, G256, stride=(1, 2, 2), family="plain", judge="crops"),
     _case(BIG, 64, 264, G256, kernel_t=1, causal=False),
     _case(BIG, 64, 264, G256, kernel_t=1, causal=False, family="plain", judge="crops")]
)

# The eight-wave direct convolution (2 x 8 x 16 tiles, 64-channel chunks): algo 4 at any grid, algo 0 from 128 tiles up where
# Cout is no multiple of 128.  One-position tiles, exact tiles, one over; 1 .. 3 chunks; B = 2 so that a halo must stay inside
# its sample.
D8 = lambda e=0: (DIRECT8, e, 1, 0, 0)
_D8_GRIDS = [((2, 1, 1, 1), 64, 8), ((2, 2, 7, 15), 128, 128), ((2, 3, 8, 16), 192, 136), ((2, 3, 9, 17), 64, 136),
             ((2, 1, 8, 17), 128, 8), ((2, 2, 9, 1), 192, 128), ((2, 3, 1, 16), 64, 128), ((2, 2, 7, 16), 128, 136)]
_MODES = [(True, True, False), (True, False, False), (False, True, False), (False, False, False), (False, False, True),
          (False, True, True), (True, True, True), (True, False, True)]           # causal, replicate, time_pad_zeros
DIRECT8_CASES = (
    [_case(g, ci, co, D8(), algo=4, causal=m[0], replicate=m[1], tzero=m[2]) for (g, ci, co), m in zip(_D8_GRIDS, _MODES)]
    + [_case(g, ci, co, D8(), algo=4, family="plain", causal=m[0], replicate=m[1], tzero=m[2])
       for (g, ci, co), m in list(zip(_D8_GRIDS, _MODES[3:] + _MODES[:3]))[1:4]]
    + [c for (g, ci, co), m in list(zip(_D8_GRIDS, _MODES[1:] + _MODES[:1]))[1:4]
       for c in _families(ADD, g, ci, co, D8(1), algo=4, epi="add", causal=m[0], replicate=m[1], tzero=m[2])]
    + _families(EP, (2, 3, 9, 17), 128, 1024, D8(2), algo=4, epi="d2s_res", causal=False)
    + _families(EP, (2, 2, 7, 15), 64, 1024, D8(2), algo=4, epi="d2s", replicate=False)
    # by shape: 2 x 2 x 2 x 4 x 4 = 128 tiles
    + [_case((2, 4, 32, 64), 64, 136, D8(), algo=0), _case((2, 3, 32, 64), 64, 136, D8(1), algo=0, epi="add", family="cancel")]
)

# The four-wave direct convolution (Cout % 128 == 0; 32-channel chunks): algo 3 at any grid, algo 0 from 768 tiles up.
# Epilogues 0 .. 5; the tiles' 16-position rows along H where that takes fewer rounds of the chip's 512 slots.
D4 = lambda e=0, s=0: (DIRECT4, e, 1, s, 0)
_D4_GRIDS = [((2, 1, 1, 1), 64, 128), ((2, 2, 7, 15), 128, 128), ((2, 3, 8, 16), 192, 256), ((2, 3, 9, 17), 64, 128),
             ((2, 1, 8, 17), 128, 256), ((2, 2, 9, 1), 192, 128), ((2, 3, 1, 16), 64, 128), ((2, 2, 7, 16), 128, 256)]
DIRECT4_CASES = (
    [_case(g, ci, co, D4(), algo=3, causal=m[0], replicate=m[1], tzero=m[2]) for (g, ci, co), m in zip(_D4_GRIDS, _MODES)]
    + [_case(g, ci, co, D4(), algo=3, family="plain", causal=m[0], replicate=m[1], tzero=m[2])
       for (g, ci, co), m in list(zip(_D4_GRIDS, _MODES[3:] + _MODES[:3]))[1:4]]
    + [c for (g, ci, co), m in list(zip(_D4_GRIDS, _MODES[1:] + _MODES[:1]))[1:4]
       for c in _families(ADD, g, ci, co, D4(1), algo=3, epi="add", causal=m[0], replicate=m[1], tzero=m[2])]
    + _families(EP, (2, 3, 9, 17), 128, 1024, D4(2), algo=3, epi="d2s_res", causal=False)
    + _families(EP, (2, 2, 7, 15), 64, 1024, D4(2), algo=3, epi="d2s", replicate=False)
    + _families(EP, (2, 3, 9, 17), 192, 128, D4(3), algo=3, norm="only", causal=False)
    + _families(EP, (2, 2, 7, 15), 64, 128, D4(3), algo=3, norm="only", replicate=False)
    + _families(ADD, (2, 3, 9, 17), 128, 128, D4(4), algo=3, epi="add", norm="second")
    + _families(EP, (2, 3, 9, 17), 128, 1024, D4(5), algo=3, epi="d2s_res", norm="second", causal=False)
    + _families(EP, (2, 2, 7, 15), 64, 1024, D4(5), algo=3, epi="d2s", norm="second", replicate=False)
    # rows along H outside the split: 130 x 2 x 2 = 520 tiles are two rounds, 130 x 3 x 1 = 390 swapped are one (H 16: exact
    # tiles; H 13, W 20: partial tiles on both axes of the swapped layout)
    + [_case((1, 130, 16, 24), 64, 256, D4(0, 1), algo=3), _case((2, 130, 13, 20), 64, 128, D4(0, 1), algo=3, replicate=False),
       _case((2, 130, 13, 20), 64, 128, D4(1, 1), algo=3, epi="add", causal=False),
       _case((2, 130, 13, 20), 64, 128, D4(0, 1), algo=3, family="plain", judge="crops", versus=4, replicate=False),
       # by shape: 16 x 8 x 6 = 768 tiles
       _case((1, 32, 64, 96), 64, 128, D4(), algo=0), _case((1, 32, 64, 96), 64, 128, D4(), algo=0, family="plain", judge="crops", versus=4)]
)

# The split over the input channels (Cin >= 1024; Cin 512 only with a norm the unsplit form cannot fuse), with a workspace of
# exactly ltxmi_conv3d_workspace_bytes: 2, 3 and 4 ranges; every instantiation of the finalising pass (Cout / 256 = 2, 4, 8, 12,
# 16); its epilogues.  Few positions: the truth is a CPU convolution.
SP = lambda k, s, f: (DIRECT4, 6, k, s, f)
SPLIT_CASES = []          # filled below from _SPLIT (the route of each is pinned there)
_SPLIT = [
    # grid, Cin, Cout, (ksplit, swap_hw, finalize_blocks), epi, norm, families
    ((2, 1, 17, 16), 1024, 1024, (4, 0, 4), "none", None, EP),
    ((1, 5, 17, 17), 1024, 1024, (3, 0, 4), "none", None, ("exact",)),
    ((2, 1, 16, 17), 1024, 1024, (4, 1, 4), "add", None, ADD),
    ((1, 1, 16, 17), 1024, 2048, (4, 1, 8), "d2s_res", None, EP),
    ((2, 1, 9, 15), 1024, 2048, (4, 0, 8), "d2s", None, EP),
    ((1, 1, 17, 17), 1024, 3072, (3, 0, 12), "none", None, EP),
    ((1, 1, 9, 15), 1024, 4096, (4, 0, 16), "d2s_res", "second", EP),
    ((2, 1, 17, 16), 1024, 1024, (4, 0, 4), "none", "only", EP),
    ((2, 1, 16, 17), 1024, 1024, (4, 1, 4), "add", "second", ADD),
    ((2, 3, 13, 25), 512, 512, (2, 0, 2), "none", "only", EP),
    ((2, 3, 13, 24), 512, 512, (2, 1, 2), "add", "second", EP),
]


# -------------------------------------------------------------------------------------------------------- geometry
def geometry(c, T=None, H=None, W=None):
    """(front, back, oT, oH, oW) of case ``c`` (on a T x H x W input when given: the crops)."""
    T, H, W = c["T"] if T is None else T, c["H"] if H is None else H, c["W"] if W is None else W
    st, sh, _ = c["stride"]
    kt = c["kernel_t"]
    if kt == 1:
        return 0, 0, T, (H - 1) // sh + 1, (W - 1) // sh + 1
    front = c["tpad"] if c["tpad"] > 0 else (2 if c["causal"] else 1)
    back0 = 0 if (c["tpad"] > 0 or c["causal"]) else 1
    oT = c["out_T"] if c["out_T"] > 0 else (T + front + back0 - kt) // st + 1
    back = max(0, (oT - 1) * st + kt - T - front)
    return front, back, oT, (H - 1) // sh + 1, (W - 1) // sh + 1


def out_shape(c):
    _, _, oT, oH, oW = geometry(c)
    if c["epi"].startswith("d2s"):
        return (c["B"], 2 * c["T"] - 1, 2 * c["H"], 2 * c["W"], c["Cout"] // 8)
    return (c["B"], oT, oH, oW, c["Cout"])


def norm_channels(c):
    return c["Cout"] // 8 if c["epi"].startswith("d2s") else c["Cout"]


# ---------------------------------------------------------------------------------------------------------- inputs
def _input_key(c):
    return tuple((k, c[k]) for k in ("B", "T", "H", "W", "Cin", "Cout", "epi", "family", "causal", "replicate", "tzero", "stride",
                                     "tpad", "out_T", "kernel_t", "bias", "norm"))


def exact_weights(cout, taps, cin, g):
    """[cout, taps, cin] ternary (see the module docstring) and S."""
    nq = cin // 32
    S = max(1, -(-taps * nq // 48))
    co, tp, q = torch.arange(cout)[:, None, None], torch.arange(taps)[None, :, None], torch.arange(nq)[None, None, :]
    on = ((co + tp + q) % S == 0).to(F32)
    ch = q * 32 + (7 * co + 3 * tp + 5 * q) % 32
    sign = (torch.randint(0, 2, (cout, taps, nq), generator=g) * 2 - 1).to(F32)
    return torch.zeros(cout, taps, cin).scatter_(2, ch, on * sign), S


def make(c):
    """dict(x [B,T,H,W,Cin], w [Cout, 9 kt Cin] packed tap-major (depth-to-space: rows in (p1 p2 p3, c') order), bias, add,
    scale, shift) on the CPU: bf16 but the fp32 scale / shift.  The depth-to-space residual is x itself."""
    return _make(_input_key(c))


@functools.lru_cache(maxsize=8)
def _make(key):
    c = dict(key)
    fam, (B, T, H, W, cin, cout) = c["family"], (c[k] for k in ("B", "T", "H", "W", "Cin", "Cout"))
    g = torch.Generator().manual_seed(9100 + 131 * FAMILIES.index(fam))
    rn = lambda *s: torch.randn(*s, generator=g)
    ri = lambda lim, *s: torch.randint(-lim, lim + 1, s, generator=g).to(F32)
    taps = 9 * c["kernel_t"]
    _, _, oT, oH, oW = geometry(c)
    add_shape = (B, oT, oH, oW, cout)
    if fam == "exact":
        x, w, bias, add = ri(4, B, T, H, W, cin), exact_weights(cout, taps, cin, g)[0], ri(4, cout), ri(8, *add_shape)
    else:
        x, w, bias, add = rn(B, T, H, W, cin), rn(cout, taps, cin) * (taps * cin) ** -0.5, rn(cout), rn(*add_shape)
        if fam == "row_scales":
            x = x * 10.0 ** (torch.rand(B, T, H, W, 1, generator=g) * 6 - 3)
    d = dict(x=x.to(BF), w=w.reshape(cout, taps * cin).to(BF), bias=bias.to(BF) if c["bias"] else None,
             add=add.to(BF) if c["epi"] == "add" else None, scale=None, shift=None)
    if c["norm"]:
        d["scale"], d["shift"] = rn(B, norm_channels(c)) * 0.3, rn(B, norm_channels(c)) * 0.3
    if fam == "cancel":
        assert c["epi"] == "add", "the cancel family is made through `add`"
        d["add"] = (-conv_op(dict(d, add=None), dict(c, epi="none"))[0]).to(BF)
    return d


def empty_inputs(c):
    """Host tensors with the shapes of ``make`` for case ``c``, never written: the geometry of the call."""
    B, T, H, W, cin, cout = (c[k] for k in ("B", "T", "H", "W", "Cin", "Cout"))
    _, _, oT, oH, oW = geometry(c)
    e = lambda *s: torch.empty(*s, dtype=BF)
    d = dict(x=e(B, T, H, W, cin), w=e(cout, 9 * c["kernel_t"] * cin), bias=e(cout) if c["bias"] else None,
             add=e(B, oT, oH, oW, cout) if c["epi"] == "add" else None, scale=None, shift=None)
    if c["norm"]:
        d["scale"], d["shift"] = torch.empty(B, norm_channels(c)), torch.empty(B, norm_channels(c))
    return d


SENTINEL = 7.0
GUARD = 4096             # elements of sentinel before and after every output (8 KiB: offsets a multiple of 16 bytes)
POST_EPS = 1e-8


def guarded(shape, device, dtype=BF):
    """(flat sentinel-filled buffer, contiguous view of ``shape`` inside it with GUARD elements before and after)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def workspace_bytes(c):
    """What ltxmi_conv3d_workspace_bytes gives for a case that runs split (pinned through the route: a byte less is unsplit)."""
    k = c["want"]["ksplit"]
    return k * c["B"] * c["T"] * c["H"] * c["W"] * c["Cout"] * 4 if k > 1 else 0


def call_args(c, d, launch=True, algo=None):
    """(kwargs for ops.conv3d / ops.conv3d_route, bufs) for case ``c`` on inputs ``d`` (on the device of d["x"]).  The output, the
    second output and the workspace are views inside sentinel-filled buffers (``bufs``: name -> (flat buffer, view)); the
    workspace is EXACTLY as large as the split asks for, and empty for a case that runs unsplit."""
    dev = d["x"].device
    kw = dict(x=d["x"], w_packed=d["w"], bias=d["bias"], causal=c["causal"], pad_replicate=c["replicate"],
              d2s=c["epi"].startswith("d2s"), residual=d["x"] if c["epi"] == "d2s_res" else None, add=d["add"], stride=c["stride"],
              tpad=c["tpad"], out_T=c["out_T"], kernel_t=c["kernel_t"], time_pad_zeros=c["tzero"],
              algo=c["algo"] if algo is None else algo)
    bufs = {}
    if launch:
        bufs["y"] = guarded(out_shape(c), dev)
        kw["out"] = bufs["y"][1]
    if c["norm"]:
        kw.update(post_norm=(d["scale"], d["shift"], POST_EPS), keep_raw=c["norm"] == "second")
        if launch and c["norm"] == "second":
            bufs["y_norm"] = guarded(out_shape(c), dev)
            kw["out_norm"] = bufs["y_norm"][1]
    nws = workspace_bytes(c) if algo is None else 0
    if launch:
        bufs["workspace"] = guarded((nws,), dev, torch.uint8)
        kw["workspace"] = bufs["workspace"][1]
    else:
        kw["workspace"] = torch.empty(nws, dtype=torch.uint8)
    return kw, bufs


# --------------------------------------------------------------------------------------- operation (dtype-generic)
def _conv(x, w, c):
    """x [B, Cin, T, H, W], w [Cout, Cin, kt, 3, 3] -> [B, Cout, oT, oH, oW] with the padding of case ``c``."""
    st, sh, _ = c["stride"]
    mode = "replicate" if c["replicate"] else "constant"
    B, C, T, H, W = x.shape
    if c["kernel_t"] == 1:                                      # a 3 x 3 nn.Conv2d on every frame
        x2 = F.pad(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W), (1, 1, 1, 1), mode=mode)
        y = F.conv2d(x2, w[:, :, 0], stride=sh)
        return y.view(B, T, *y.shape[1:]).permute(0, 2, 1, 3, 4)
    front, back, oT, _, _ = geometry(c, T, H, W)
    xs = F.pad(x.reshape(B, C * T, H, W), (1, 1, 1, 1), mode=mode).view(B, C, T, H + 2, W + 2)
    if c["tzero"] and not c["causal"] and not c["tpad"] and not c["out_T"]:
        return F.conv3d(xs, w, stride=(st, sh, sh), padding=(1, 0, 0))            # nn.Conv3d(padding=1)
    edge = (lambda f, n: torch.zeros_like(f).repeat(1, 1, n, 1, 1)) if c["tzero"] else (lambda f, n: f.repeat(1, 1, n, 1, 1))
    xs = torch.cat([edge(xs[:, :, :1], front), xs] + ([edge(xs[:, :, -1:], back)] if back else []), dim=2)
    return F.conv3d(xs, w, stride=(st, sh, sh))[:, :, :oT]


def _shuffle(y):
    """pixel_shuffle_3d on ((p1 p2 p3) c')-major channels, first frame dropped: [B, 8 C', T, H, W] -> [B, C', 2T-1, 2H, 2W]."""
    B, C8, T, H, W = y.shape
    y = y.view(B, 2, 2, 2, C8 // 8, T, H, W).permute(0, 4, 5, 1, 6, 2, 7, 3)
    return y.reshape(B, C8 // 8, 2 * T, 2 * H, 2 * W)[:, :, 1:]


def _shuffle_input(x, cp):
    """DepthToSpaceUpsample's x_in: pixel_shuffle_3d of x (channels (c p1 p2 p3)) repeated to cp channels, first frame dropped."""
    B, C, T, H, W = x.shape
    y = x.view(B, C // 8, 2, 2, 2, T, H, W).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(B, C // 8, 2 * T, 2 * H, 2 * W)
    return y.repeat(1, cp // (C // 8), 1, 1, 1)[:, :, 1:]


def conv_op(d, c, dt=F64):
    """include/ltxmi.h: y = conv(x, w) + bias (+ add | depth-to-space store (+ residual)) -> (value, mag), NDHWC, in ``dt``."""
    cout, cin, kt = c["Cout"], c["Cin"], c["kernel_t"]
    x = d["x"].to(dt).permute(0, 4, 1, 2, 3)
    w = d["w"].to(dt).view(cout, kt, 3, 3, cin).permute(0, 4, 1, 2, 3)
    acc, mag = _conv(x, w, c), _conv(x.abs(), w.abs(), c)
    if d.get("bias") is not None:
        b = d["bias"].to(dt)[None, :, None, None, None]
        acc, mag = acc + b, mag + b.abs()
    if c["epi"].startswith("d2s"):
        acc, mag = _shuffle(acc), _shuffle(mag)
        if c["epi"] == "d2s_res":
            r = _shuffle_input(x, cout // 8)
            acc, mag = acc + r, mag + r.abs()
    acc, mag = acc.permute(0, 2, 3, 4, 1), mag.permute(0, 2, 3, 4, 1)
    if d.get("add") is not None:
        a = d["add"].to(dt)
        acc, mag = acc + a, mag + a.abs()
    return acc.contiguous(), mag.contiguous()


def norm_op(y, d, dt=F64, ymag=None):
    """PixelNorm -> (1 + scale[b]) y + shift[b] -> SiLU over the channels of NDHWC ``y`` -> (value, mag): pixelnorm_op of
    tests/norm_cases.py.  ``ymag``: the sum of magnitudes behind ``y`` where y is itself a result (the ONLY-output form); it goes
    through the norm in |y|'s place: mag = ymag rstd (1 + |scale|) + |shift|."""
    from norm_cases import pixelnorm_op
    sc = sh = None
    if d["scale"] is not None:
        sc, sh = (t.to(y.device)[:, None, None, None, :].expand(y.shape) for t in (d["scale"], d["shift"]))
    v, mag = pixelnorm_op(y, POST_EPS, sc, sh, True, dt)
    if ymag is not None:
        m = ymag.to(dt) * torch.rsqrt((y.to(dt) ** 2).mean(-1, keepdim=True) + POST_EPS)
        mag = m if sc is None else m * (1 + sc.to(dt).abs()) + sh.to(dt).abs()
    return v, mag


def restate(d, c):
    """fp32 arithmetic, one rounding to bf16: what a correct implementation of the header gives.  -> raw, or (raw, activated)
    with ``norm`` "second", or the activated result alone with "only"."""
    raw = conv_op(d, c, F32)[0]
    if c["norm"] == "only":
        return norm_op(raw, d, F32)[0].to(BF)
    raw = raw.to(BF)
    return (raw, norm_op(raw, d, F32)[0].to(BF)) if c["norm"] == "second" else raw


def truth(c):
    """(value, mag) of the case's one output in float64 ("second": of the RAW output; the activated one is norm_op of the raw
    output under test) -- fp32 for the exact family, where it is exact."""
    return _truth(_input_key(c))


@functools.lru_cache(maxsize=4)
def _truth(key):
    c = dict(key)
    d = _make(key)
    t, mag = conv_op(d, c, F32 if c["family"] == "exact" else F64)
    if c["norm"] == "only":
        t, mag = norm_op(t, d, F64, mag)
    return t, mag


def exact_ok(t):
    """The exact family's condition: every element an integer of magnitude <= 256."""
    return bool((t == t.round()).all()) and float(t.abs().max()) <= 256.0


# ---------------------------------------------------------------------------------------------------------- crops
CROP = (6, 12, 20)          # input positions per axis of a corner crop


def crops(c):
    """For judge == "crops": [(input slices, output slices of the full result, output slices of the crop's result)] for the near
    and the far corner of the grid.  A crop keeps the volume's own borders on its corner's side, so the padding acts on it as on
    the full tensor; the outputs compared are those whose receptive field lies inside the crop.  Per axis, with stride s and
    ``front`` positions of padding in front: output o reads inputs o s - front .. o s - front + k - 1."""
    assert not c["tpad"] and not c["out_T"]
    st, sh, _ = c["stride"]
    front, _, oT, oH, oW = geometry(c)
    near, far_in, far_full, far_crop = [], [], [], []
    for n, n_out, s, fr, k, size in ((c["T"], oT, st, front, c["kernel_t"], CROP[0]), (c["H"], oH, sh, 1, 3, CROP[1]),
                                     (c["W"], oW, sh, 1, 3, CROP[2])):
        m = min(size, n)
        hi = n_out if m == n else (m - 1 - (k - 1 - fr)) // s + 1          # outputs 0 .. hi-1 read inputs < m
        near.append((slice(0, m), slice(0, hi), slice(0, hi)))
        a = (n - m) // s * s                                               # the far crop starts at a multiple of the stride
        lo = 0 if a == 0 else -(-fr // s)                                  # its outputs lo .. read inputs >= a
        far_in.append(slice(a, n))
        far_full.append(slice(a // s + lo, n_out))
        far_crop.append(slice(lo, n_out - a // s))
    return [tuple(zip(*near)), (tuple(far_in), tuple(far_full), tuple(far_crop))]


def crop_truth(c, d, slices):
    """float64 (value, mag) of the crop's valid outputs, and the slices that take the same outputs from the full result."""
    ins, full, crop = slices
    dc = dict(d, x=d["x"][(slice(None),) + tuple(ins)].contiguous())
    dc["add"] = None                                      # (added below, from the full tensor's positions)
    t, mag = conv_op(dc, dict(c, epi="none" if c["epi"] == "add" else c["epi"]), F64)
    if c["epi"].startswith("d2s"):
        up = lambda s, n: slice(max(0, 2 * s.start - (1 if n == 0 else 0)), 2 * s.stop - (1 if n == 0 else 0))
        full, crop = tuple(up(s, i) for i, s in enumerate(full)), tuple(up(s, i) for i, s in enumerate(crop))
    sel_c, sel_f = (slice(None),) + tuple(crop), (slice(None),) + tuple(full)
    t, mag = t[sel_c], mag[sel_c]
    if c["epi"] == "add":
        a = d["add"][sel_f].to(F64)
        t, mag = t + a, mag + a.abs()
    return t, mag, sel_f


# --------------------------------------------------------------------------------------------------------- metrics
def _check():
    from test_gpu_kernels import MAXREL, REL_L2, check
    return check, REL_L2, MAXREL


def _block_figures(err, t, bh, bw):
    """(worst rel L2, worst max err / max |truth|) over the (sample, frame, bh x bw tile, 128-channel block)s of >= 64 values."""
    B, T, H, W, C = t.shape
    ph, pw, pc = -H % bh, -W % bw, -C % 128

    def blocks(z):
        z = F.pad(z, (0, pc, 0, pw, 0, ph))
        z = z.view(B, T, (H + ph) // bh, bh, (W + pw) // bw, bw, (C + pc) // 128, 128)
        return z.permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(-1, bh * bw * 128)

    e, tt = blocks(err), blocks(t)
    keep = blocks(torch.ones_like(t)).sum(-1) >= 64
    if not bool(keep.any()):
        return None
    l2 = (e.norm(dim=-1) / tt.norm(dim=-1).clamp_min(1e-300))[keep]
    mx = (e.abs().amax(-1) / tt.abs().amax(-1).clamp_min(1e-300))[keep]
    return float(l2.max()), float(mx.max())


def figures(out, t, mag, slack=None):
    """The figures of metrics (b) and (c) as fractions of their limits (float64 arithmetic, on ``out``'s device)."""
    _, REL_L2, MAXREL = _check()
    slack = SLACK if slack is None else slack
    o, t, mag = out.to(F64), t.to(out.device, F64), mag.to(out.device, F64)
    err = o - t
    f = {}
    for name, (bh, bw) in (("hw", (8, 16)), ("wh", (16, 8))):
        r = _block_figures(err, t, bh, bw)
        if r:
            f[f"blk_{name}_l2"], f[f"blk_{name}_max"] = r[0] / REL_L2, r[1] / MAXREL
    lim = 2.0 ** -7 * t.abs() + slack * mag
    f["elem"] = float(torch.where(t.abs() >= 1e-30, err.abs() / lim.clamp_min(1e-300), torch.zeros_like(err)).max())
    return f


def compare(out, t, mag, what="", slack=None):
    """All three metrics; returns the figures as fractions of their limits (the whole-tensor ones included)."""
    check, REL_L2, MAXREL = _check()
    assert out.shape == t.shape, (what, out.shape, t.shape)
    assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    f = figures(out, t, mag, slack)
    o, tt = out.to(F64), t.to(out.device, F64)
    f["all_l2"] = float((o - tt).norm() / tt.norm().clamp_min(1e-300)) / REL_L2
    f["all_max"] = float((o - tt).abs().max() / tt.abs().max().clamp_min(1e-300)) / MAXREL
    print(f"{what}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(f.items())))
    bad = {k: round(v, 4) for k, v in f.items() if not v <= 1.0}
    assert not bad, f"{what}: over the limit (fraction of it): {bad}"
    check(out, t, what=what)
    return f


SLACK_GRID = (2, 3, 5, 7)


def slack_key(c):
    return (c["family"], c["epi"] + ("+" + c["norm"] if c["norm"] else ""), 9 * c["kernel_t"] * c["Cin"])


def slack_case(family, epi, K):
    """The case the slack of (family, epilogue, K) is measured on: SLACK_GRID positions, 264 channels out (depth-to-space: 5 Cin;
    with a norm 128 / 1024): the error of an element depends on K, not on the grid."""
    kt = next(c["kernel_t"] for c in GPU_CASES if slack_key(c) == (family, epi, K))
    epi, _, norm = epi.partition("+")
    cin = K // (9 * kt)
    cout = (1024 if epi.startswith("d2s") else 128) if norm else (5 * cin if epi.startswith("d2s") else 264)
    return _case(SLACK_GRID, cin, cout, (0, 0, 1, 0, 0), epi=epi, family=family, norm=norm or None, kernel_t=kt,
                 causal=kt == 3)


def restated_outputs(c):
    """[(name, restated output, truth, mag)] of case ``c`` on the CPU: what ``compare`` must accept."""
    d = make(c)
    r = restate(d, c)
    t, mag = truth(c)
    if c["norm"] == "second":
        ta, maga = norm_op(r[0], d, F64)
        return [("raw", r[0], t, mag), ("activated", r[1], ta, maga)]
    return [("activated" if c["norm"] else "raw", r, t, mag)]


def measure_excess(cases=None):
    """{epilogue: largest (|restate - truth| - 2^-8 |truth|) / mag} over SLACK_CASES (CPU); of the activated output with a norm."""
    worst = {}
    for family, epi, K in (SLACK_CASES if cases is None else cases):
        if (family, epi) in DROPPED or family == "exact":
            continue
        name, r, t, mag = restated_outputs(slack_case(family, epi, K))[-1]
        ex = float((((r.to(F64) - t).abs() - 2.0 ** -8 * t.abs()) / mag).max())
        worst[epi] = max(worst.get(epi, 0.0), ex)
    return worst


for _g, _ci, _co, (_k, _s, _f), _e, _n, _fams in _SPLIT:
    SPLIT_CASES += _families(_fams, _g, _ci, _co, SP(_k, _s, _f), epi=_e, norm=_n, causal=_e != "none", replicate=_e != "add")

GPU_CASES = GEMM128_CASES + GEMM256_CASES + DIRECT8_CASES + DIRECT4_CASES + SPLIT_CASES
SLACK_CASES = sorted({slack_key(c) for c in GPU_CASES if c["family"] != "exact"})
