"""Cases for the two-pair MX-FP8 GEMM of include/ltxmi_mx_lora.h -- TEST INFRASTRUCTURE ONLY (plain module, no GPU), built on
tests/mx8_cases.py (the format, the operands, the truth and its bounds).  Shared by tests/test_mxl_cases.py (CPU) and
tests/test_gpu_mxl_kernels.py (MI355X).

A two-pair call is ltxmi_gemm_mx8 on the materialised concatenation, bit for bit, so a case is DRAWN as that concatenation:
``make`` is mx8_cases.make at K = K1 + K2 (one draw per group of the second pair, so that the groups' A2 slices hold different
data), ``split`` cuts it at K1 -- element bytes at byte K1 of a row, scale bytes at K1 / 32 -- into the operands of the call, and
``concatenation`` puts group g's slices back together.  The first pair stays VIEWS into the drawn arrays (lda = K1 + K2,
lda_s = (K1 + K2) / 32: strides longer than the rows), the second pair is copied out ([M, groups * K2] and [N, K2], contiguous).

  shapes      (300, 288), (520, 544): ragged against the 256 x 256 tile both ways, 2 x 2 and 3 x 3 tiles; (1, 288): M = 1;
  (K1, K2)    K-tiles of 128.  (128, 128): the two prologue stages come from different pairs, no refill; (128, 256): the first
              refill (tile 2) is the second pair's second tile; (256, 128): the only refill is the switch; (384, 128): the switch
              lies in the last refill, whose tile is the last peeled one; (256, 256): the switch in a refill, both peeled tiles from
              the second pair; (2048, 128): a long first pair (16 + 1 tiles);
  families    plain and row_scales: with a scale of its own per row and block a pair that read the other pair's scale words
              (or another group's) gives other bits;
  groups      N 768 with group_cols 256 (the packed q/k/v form: three groups, row sums over the first 256 columns) and N 1024
              with group_cols 512 (a group spans two tiles).

Totals K1 + K2 that mx8_cases.SLACK_CASES does not hold are measured by tests/test_mxl_cases.py and held to what its SLACK
rests on, so the GPU file brings no tolerance of its own."""
import torch

import mx8_cases as mc

BF, F64 = mc.BF, mc.F64

SHAPES = [(300, 288), (520, 544), (1, 288)]
K_PAIRS = [(128, 128), (128, 256), (256, 128), (384, 128), (256, 256), (2048, 128)]
FAMILIES = ["plain", "row_scales"]
# (epilogue, MX output): every instance behind ltxmi_gemm_mx8
FORMS = [(e, False) for e in mc.EPIS] + [(e, True) for e in mc.MX_EPIS]
CASES = [dict(M=M, N=N, K1=k1, K2=k2, family=f, groups=1) for (M, N) in SHAPES for (k1, k2) in K_PAIRS for f in FAMILIES]
RSS_CASES = [dict(M=300, N=288, K1=256, K2=128, family=f, groups=1, cols=c) for c in (64, 256) for f in FAMILIES]
GROUP_CASES = [dict(M=300, N=768, K1=256, K2=128, family=f, groups=3, cols=256) for f in FAMILIES] + \
              [dict(M=300, N=1024, K1=256, K2=128, family="row_scales", groups=2, cols=0)]
SLACK_CASES = sorted({(c["family"], e, c["K1"] + c["K2"]) for c in CASES for e, _ in FORMS})


def case_id(c):
    return f"{c['M']}x{c['N']}-K{c['K1']}+{c['K2']}-{c['family']}" + (f"-g{c['groups']}" if c["groups"] > 1 else "") + \
        (f"-cols{c['cols']}" if c.get("cols") else "")


def group_cols(c):
    return c["N"] // c["groups"] if c["groups"] > 1 else 0


def make(c, epi="none", device="cpu"):
    """One mx8_cases.make dict per group at K = K1 + K2.  Group 0's is the case's own (its weights, bias, gate and residual are
    the call's); the others lend only the second part of their activations."""
    return [mc.make(c["family"], c["M"], c["N"], c["K1"] + c["K2"], epi, device=device, seed=g) for g in range(c["groups"])]


def split(c, ds):
    """``make``'s dicts -> dict(a, w: the first pair as (q, scales) views; a2 = (q [M, groups * K2], scales [M, groups * K2 / 32]),
    w2 = (q [N, K2], scales [N, K2 / 32]): the second pair, contiguous copies)."""
    k1, b1 = c["K1"], c["K1"] // mc.BLOCK
    d = ds[0]
    a2q = torch.cat([g["aq"].view(torch.uint8)[:, k1:] for g in ds], dim=1).contiguous().view(mc.E4M3)
    a2s = torch.cat([g["a_scales"][:, b1:] for g in ds], dim=1).contiguous()
    return dict(a=(d["aq"][:, :k1], d["a_scales"][:, :b1]), w=(d["wq"][:, :k1], d["w_scales"][:, :b1]),
                a2=(a2q, a2s), w2=(d["wq"][:, k1:].contiguous(), d["w_scales"][:, b1:].contiguous()))


def concatenation(c, s, g):
    """``split``'s operands and a group -> (aq, a_scales, wq, w_scales) at K1 + K2, materialised: bytes and scale bytes
    concatenated along K, with group g's K2 columns of the second activation."""
    k2, b2 = c["K2"], c["K2"] // mc.BLOCK
    u8 = lambda t: t.view(torch.uint8)
    aq = torch.cat([u8(s["a"][0]), u8(s["a2"][0])[:, g * k2:(g + 1) * k2]], dim=1).contiguous().view(mc.E4M3)
    a_s = torch.cat([s["a"][1], s["a2"][1][:, g * b2:(g + 1) * b2]], dim=1).contiguous()
    wq = torch.cat([u8(s["w"][0]), u8(s["w2"][0])], dim=1).contiguous().view(mc.E4M3)
    w_s = torch.cat([s["w"][1], s["w2"][1]], dim=1).contiguous()
    return aq, a_s, wq, w_s


def two_pair_truth(c, s, g):
    """float64 (x W^T + T_g B^T, |x| |W|^T + |T_g| |B|^T) of the de-quantised operands of a two-pair call, each pair
    de-quantised on its own."""
    k2, b2 = c["K2"], c["K2"] // mc.BLOCK
    a, w = mc.dequantize(*s["a"]), mc.dequantize(*s["w"])
    t = mc.dequantize(s["a2"][0][:, g * k2:(g + 1) * k2], s["a2"][1][:, g * b2:(g + 1) * b2])
    b = mc.dequantize(*s["w2"])
    return a @ w.T + t @ b.T, a.abs() @ w.abs().T + t.abs() @ b.abs().T


def pad_rank(down, up, to=128):
    """down [r, K], up [N, r] -> the same with r padded by zero rows / columns to the next multiple of ``to``."""
    r = down.shape[0]
    R = (r + to - 1) // to * to
    dp = torch.zeros(R, down.shape[1], dtype=down.dtype)
    dp[:r] = down
    upad = torch.zeros(up.shape[0], R, dtype=up.dtype)
    upad[:, :r] = up
    return dp, upad
