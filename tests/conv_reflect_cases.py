"""Cases, inputs and float64 truths for ltxmi_conv3d_ndhwc_bf16 with spatial padding mode 2 (reflect) -- TEST INFRASTRUCTURE ONLY
(plain module, no GPU).  Shared by tests/test_conv_reflect_cases.py (CPU) and tests/test_gpu_conv_reflect.py (MI355X).

Everything but the padding is tests/conv_cases.py: the case dictionaries (``_case``), the input families (``make``), the metrics
(``compare``, ``SLACK``), the sentinel-guarded buffers, the geometry.  A case here is the dictionary of its REPLICATE TWIN: its
``want`` is the route that twin takes, because the mode takes no part in the plan (include/ltxmi.h); ``call_args`` hands the
library mode 2 in the twin's place.

TRUTH.  conv_cases._conv knows a boolean ``replicate`` only, so the reflect truth is written out here (``_conv``, with the pad mode
as an argument so that the CPU file can put the three modes side by side): F.pad(mode="reflect") by one in H and W -- index -1
reads index 1, index L reads index L - 2, a corner mirrors on both axes -- and the time axis exactly as conv_cases has it
(replicated frames, or zeros with time_pad_zeros).  ``conv_op`` returns (value, mag), mag = conv(|x|, |w|) + |bias| + |add|
(+ |residual|), as there.  The exact family's condition (an integer truth of magnitude <= 256) holds under any padding: a padded
element is an input element or zero, so an output still has at most 48 terms of magnitude <= 4 (asserted all the same).  The
cancel family's `add` is made from the REFLECT truth, so that the output is the accumulator's rounding residue in this mode."""
import functools

import torch
import torch.nn.functional as F

import conv_cases as cc
from conv_cases import SLACK, compare, exact_ok, geometry, guarded, guards_intact, make as _make_twin, out_shape  # noqa: F401

BF, F32, F64 = cc.BF, cc.F32, cc.F64
PAD_REFLECT = 2                 # include/ltxmi.h: ltxmi_conv3d_args.pad_replicate
PAD_NAMES = {"zeros": "constant", "replicate": "replicate", "reflect": "reflect"}


# ---------------------------------------------------------------------------------------------------------- cases
def _c(*a, **k):
    return cc._case(*a, replicate=True, **k)


def _fam(fams, *a, **k):
    return [_c(*a, family=f, **k) for f in fams]


EP, ADD, G128 = cc.EP, cc.ADD, cc.G128
D8, D4, SP = cc.D8, cc.D4, cc.SP

# The smallest shapes at which each path can get the mirror wrong.  2 x 2: both neighbours of a position mirror onto the
# opposite row / column.  Odd grids under a stride of 2 read the far pad, even ones do not.  9 x 17 in the direct forms: the
# one-row / one-column last tile's halo mirrors into the rows of the tile before it.
GEMM128_CASES = (
    _fam(EP, (1, 3, 5, 7), 64, 136, G128, causal=False)
    + _fam(EP, (2, 2, 2, 2), 64, 8, G128)
    + [_c((2, T, H, W), 64, 136, G128, stride=s, causal=ca)
       for s, ca in (((2, 1, 1), True), ((1, 2, 2), False), ((2, 2, 2), True)) for (T, H, W) in ((5, 7, 9), (4, 6, 8))]
    + [_c((2, 5, 7, 9), 64, 136, G128, stride=(2, 2, 2), family="plain")]
    + _fam(EP, (2, 4, 5, 7), 64, 72, G128, tpad=3, out_T=5)
    + _fam(EP, (2, 3, 5, 7), 128, 136, G128, kernel_t=1, causal=False)
    + _fam(EP, (2, 3, 5, 7), 64, 136, G128, tzero=True, causal=False)
    + _fam(EP, (2, 3, 5, 7), 64, 136, G128, bias=False)
    + _fam(ADD, (2, 3, 5, 7), 128, 136, (cc.GEMM128, 1, 1, 0, 0), epi="add", causal=False)
    + _fam(EP, (2, 3, 5, 7), 64, 320, (cc.GEMM128, 2, 1, 0, 0), epi="d2s_res")
    + _fam(EP, (2, 3, 5, 7), 64, 320, (cc.GEMM128, 2, 1, 0, 0), epi="d2s", causal=False)
)
GEMM256_CASES = [_c(cc.BIG, 64, 264, cc.G256, algo=1), _c(cc.BIG, 64, 264, cc.G256, algo=1, causal=False, tzero=True)]
DIRECT8_CASES = (
    _fam(EP, (2, 2, 7, 15), 128, 128, D8(), algo=4)
    + _fam(EP, (2, 3, 8, 16), 192, 136, D8(), algo=4, causal=False)
    + _fam(EP, (2, 3, 9, 17), 64, 136, D8(), algo=4)
    + _fam(EP, (2, 3, 9, 17), 64, 136, D8(), algo=4, causal=False, tzero=True)
    + _fam(EP, (2, 2, 2, 2), 64, 8, D8(), algo=4, causal=False)
    + _fam(ADD, (2, 3, 9, 17), 64, 136, D8(1), algo=4, epi="add", causal=False)
    + _fam(EP, (2, 3, 9, 17), 128, 1024, D8(2), algo=4, epi="d2s_res")
)
DIRECT4_CASES = (
    _fam(EP, (2, 2, 7, 15), 128, 128, D4(), algo=3)
    + _fam(EP, (2, 3, 8, 16), 192, 256, D4(), algo=3, causal=False)
    + _fam(EP, (2, 3, 9, 17), 64, 128, D4(), algo=3)
    + _fam(EP, (2, 3, 9, 17), 64, 128, D4(), algo=3, causal=False, tzero=True)
    + _fam(EP, (2, 2, 2, 2), 64, 128, D4(), algo=3, causal=False)
    + [_c((2, 130, 13, 20), 64, 128, D4(0, 1), algo=3)]                           # rows along H: partial tiles on both axes
    + _fam(EP, (2, 3, 9, 17), 192, 128, D4(3), algo=3, norm="only", causal=False)
    + _fam(ADD, (2, 3, 9, 17), 128, 128, D4(4), algo=3, epi="add", norm="second")
    + _fam(EP, (2, 3, 9, 17), 128, 1024, D4(5), algo=3, epi="d2s_res", norm="second", causal=False)
)
SPLIT_CASES = (
    _fam(EP, (2, 1, 17, 16), 1024, 1024, SP(4, 0, 4))
    + _fam(EP, (2, 1, 16, 17), 1024, 1024, SP(4, 1, 4), epi="add", causal=False)
    + _fam(EP, (2, 3, 13, 25), 512, 512, SP(2, 0, 2), norm="only", causal=False)
)
GPU_CASES = GEMM128_CASES + GEMM256_CASES + DIRECT8_CASES + DIRECT4_CASES + SPLIT_CASES


def case_id(c):
    return cc.case_id(c).replace("-repl", "-reflect")


def call_args(c, d, launch=True):
    """conv_cases.call_args with the mode in the twin's place."""
    kw, bufs = cc.call_args(c, d, launch=launch)
    kw["pad_replicate"] = PAD_REFLECT
    return kw, bufs


# ------------------------------------------------------------------------------------ operation (dtype-generic)
def _conv(x, w, c, pad):
    """x [B, Cin, T, H, W], w [Cout, Cin, kt, 3, 3] -> [B, Cout, oT, oH, oW]; space padded by 1 in ``pad`` ("zeros", "replicate",
    "reflect": F.pad's), time as conv_cases._conv."""
    st, sh, _ = c["stride"]
    B, C, T, H, W = x.shape
    pad2 = lambda z: F.pad(z, (1, 1, 1, 1), mode=PAD_NAMES[pad])                   # z [N, C, H, W]
    if c["kernel_t"] == 1:
        y = F.conv2d(pad2(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)), w[:, :, 0], stride=sh)
        return y.view(B, T, *y.shape[1:]).permute(0, 2, 1, 3, 4)
    front, back, oT, _, _ = geometry(c, T, H, W)
    xs = pad2(x.reshape(B, C * T, H, W)).view(B, C, T, H + 2, W + 2)
    edge = (lambda f, n: torch.zeros_like(f).repeat(1, 1, n, 1, 1)) if c["tzero"] else (lambda f, n: f.repeat(1, 1, n, 1, 1))
    xs = torch.cat([edge(xs[:, :, :1], front), xs] + ([edge(xs[:, :, -1:], back)] if back else []), dim=2)
    return F.conv3d(xs, w, stride=(st, sh, sh))[:, :, :oT]


def conv_op(d, c, dt=F64, pad="reflect"):
    """conv_cases.conv_op with the spatial padding mode ``pad`` -> (value, mag), NDHWC, in ``dt``."""
    cout, cin, kt = c["Cout"], c["Cin"], c["kernel_t"]
    x = d["x"].to(dt).permute(0, 4, 1, 2, 3)
    w = d["w"].to(dt).view(cout, kt, 3, 3, cin).permute(0, 4, 1, 2, 3)
    acc, mag = _conv(x, w, c, pad), _conv(x.abs(), w.abs(), c, pad)
    if d.get("bias") is not None:
        b = d["bias"].to(dt)[None, :, None, None, None]
        acc, mag = acc + b, mag + b.abs()
    if c["epi"].startswith("d2s"):
        acc, mag = cc._shuffle(acc), cc._shuffle(mag)
        if c["epi"] == "d2s_res":
            r = cc._shuffle_input(x, cout // 8)
            acc, mag = acc + r, mag + r.abs()
    acc, mag = acc.permute(0, 2, 3, 4, 1), mag.permute(0, 2, 3, 4, 1)
    if d.get("add") is not None:
        a = d["add"].to(dt)
        acc, mag = acc + a, mag + a.abs()
    return acc.contiguous(), mag.contiguous()


def make(c):
    """conv_cases.make's inputs; the cancel family's `add` remade from the reflect truth."""
    return _make(cc._input_key(c))


@functools.lru_cache(maxsize=8)
def _make(key):
    c = dict(key)
    d = dict(_make_twin(c))
    if c["family"] == "cancel":
        d["add"] = (-conv_op(dict(d, add=None), dict(c, epi="none"))[0]).to(BF)
    return d


def truth(c):
    """(value, mag) of the case's one output under reflect, as conv_cases.truth: float64 (fp32 in the exact family, where it is
    exact); with norm "second" of the RAW output."""
    return _truth(cc._input_key(c))


@functools.lru_cache(maxsize=4)
def _truth(key):
    c = dict(key)
    d = _make(key)
    t, mag = conv_op(d, c, F32 if c["family"] == "exact" else F64)
    if c["norm"] == "only":
        t, mag = cc.norm_op(t, d, F64, mag)
    return t, mag


def border_mask(c):
    """bool [oT', oH', oW'] over the output grid (the depth-to-space grid where the case stores that way): True where the
    position's 3 x 3 window touches the spatial padding, i.e. where the modes can differ at all."""
    _, sh, _ = c["stride"]
    _, _, oT, oH, oW = geometry(c)
    touches = lambda n_out, n: torch.tensor([o * sh - 1 < 0 or o * sh + 1 > n - 1 for o in range(n_out)])
    m = touches(oH, c["H"])[:, None] | touches(oW, c["W"])[None, :]
    if c["epi"].startswith("d2s"):
        return m.repeat_interleave(2, 0).repeat_interleave(2, 1)[None].expand(2 * c["T"] - 1, -1, -1)
    return m[None].expand(oT, -1, -1)
