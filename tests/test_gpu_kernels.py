"""Kernel-level parity on a real MI355X: every libltxmi entry point (called through the C ABI
via ltxmi.ops) against the CPU oracle / an fp32 restatement of the same op on the same seeded
bf16 inputs.

Tolerances (written once here): outputs are bf16, so a correct kernel differs from the fp32
truth by one bf16 rounding (relative 2^-9 worst case, ~1.1e-3 rms); accumulation is fp32.
  REL_L2: relative L2 error of the whole tensor   <= 3e-3
  MAXABS: max |err| <= 1.6e-2 * max|truth|        (two bf16 ulps at the top of the range)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

REL_L2 = 3e-3
MAXREL = 1.6e-2
DEV = "cuda"
BF = torch.bfloat16


def check(out, truth, rel_l2=REL_L2, maxrel=MAXREL, what=""):
    out = out.detach().float().cpu()
    truth = truth.detach().float().cpu()
    assert out.shape == truth.shape, (what, out.shape, truth.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out - truth).norm() / truth.norm().clamp_min(1e-12)
    mx = (out - truth).abs().max() / truth.abs().max().clamp_min(1e-12)
    assert err <= rel_l2, f"{what}: rel L2 {err:.3e} > {rel_l2}"
    assert mx <= maxrel, f"{what}: max err {mx:.3e} of range > {maxrel}"
    return float(err)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


# ------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (1000, 136, 256), (128, 128, 64), (3, 768, 256),
                                   (6144, 4096, 256),        # the persistent 256x256 kernel (24 x 16 tiles)
                                   (6145, 4104, 128)])       # ... with ragged M and N (25 x 17 tiles)
def test_gemm_bias(M, N, K):
    from ltxmi import ops
    a, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    assert ops.gemm_kernel_id(a.to(DEV), w.to(DEV), b.to(DEV)) == (2 if M >= 6144 else 0)
    out = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV))
    truth = a.float() @ w.float().T + b.float()
    check(out, truth, what=f"gemm {M}x{N}x{K}")


def test_gemm_asymmetric_identity():
    """A = I with an ASYMMETRIC W catches a transposed C write (cdna guide, section 3)."""
    from ltxmi import ops
    K = 128
    a = torch.eye(K).to(BF)
    w = (torch.arange(200 * K).reshape(200, K) % 251).float().sub(125).div(16).to(BF)
    out = ops.gemm(a.to(DEV), w.to(DEV))
    assert torch.equal(out.cpu(), w.T.contiguous())


@pytest.mark.parametrize("epi", ["gelu", "silu"])
def test_gemm_activation_epilogues(epi):
    from ltxmi import ops
    M, N, K = 515, 384, 192
    a, w, b = rnd(M, K, seed=4), rnd(N, K, seed=5, scale=K ** -0.5), rnd(N, seed=6)
    pre = a.float() @ w.float().T + b.float()
    if epi == "gelu":
        out = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), epilogue=ops.EPI_GELU_TANH)
        truth = torch.nn.functional.gelu(pre, approximate="tanh")
    else:
        out = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), epilogue=ops.EPI_SILU)
        truth = torch.nn.functional.silu(pre)
    check(out, truth, what=epi)


def test_gemm_gate_residual_in_place_per_frame():
    from ltxmi import ops
    B, F, hw, D, K = 2, 3, 50, 256, 128
    N = F * hw
    a, w, b = rnd(B * N, K, seed=7), rnd(D, K, seed=8, scale=K ** -0.5), rnd(D, seed=9)
    res = rnd(B * N, D, seed=10)
    table = rnd(6, D, seed=11)
    temb = rnd(B * F, 6 * D, seed=12)
    gate = (table[2].float()[None] + temb[:, 2 * D:3 * D].float())               # [B*F, D]
    truth = res.float() + gate.repeat_interleave(hw, dim=0) * (a.float() @ w.float().T + b.float())
    r = res.to(DEV).clone()
    td, ed = table.to(DEV), temb.to(DEV)
    ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), out=r, epilogue=ops.EPI_GATE_RESIDUAL, residual=r,
             gate_table=td[2], gate_temb=ed[:, 2 * D:3 * D], rows_per_group=hw)
    check(r, truth, what="gate_residual")
    # gate == NULL -> plain residual add
    r2 = res.to(DEV).clone()
    ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), out=r2, epilogue=ops.EPI_GATE_RESIDUAL, residual=r2)
    check(r2, res.float() + a.float() @ w.float().T + b.float(), what="residual")


def test_gemm_strided_views():
    from ltxmi import ops
    M, K, N = 200, 128, 64
    big = rnd(M, 3 * K, seed=13)
    w = rnd(N, K, seed=14, scale=K ** -0.5)
    out_big = torch.zeros(M, 2 * N, dtype=BF, device=DEV)
    ops.gemm(big.to(DEV)[:, K:2 * K], w.to(DEV), out=out_big[:, N:])
    check(out_big[:, N:], big[:, K:2 * K].float() @ w.float().T, what="strided")
    assert (out_big[:, :N] == 0).all()


# -------------------------------------------------------------------------- attention
def attn_truth(q, k, v, bias=None, scale=None):
    from oracle import dit
    mask = None
    if bias is not None:
        mask = bias[:, None, None, :].float()          # [B, 1, 1, Lk] in the seam's NHD mask layout
    if scale is not None:
        q = (q.float() * (scale * math.sqrt(q.shape[-1]))).float()
    return dit.sdpa_nhd(q.float(), k.float(), v.float(), mask)


@pytest.mark.parametrize("B,H,Lq,Lk,dh", [(2, 3, 200, 333, 64), (1, 2, 128, 128, 64), (1, 4, 1, 65, 64),
                                          (2, 2, 257, 64, 128), (1, 3, 77, 200, 128), (1, 2, 640, 1024, 64),
                                          (2, 32, 2100, 333, 64),    # enough work for the 64-rows-per-wave path
                                          (1, 64, 2049, 192, 64)])
def test_attention_self(B, H, Lq, Lk, dh):
    from ltxmi import ops
    q, k, v = rnd(B, Lq, H, dh, seed=20), rnd(B, Lk, H, dh, seed=21), rnd(B, Lk, H, dh, seed=22)
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    check(out, attn_truth(q, k, v), what=f"attn {B},{H},{Lq},{Lk},{dh}")


@pytest.mark.parametrize("dh", [64, 128])
def test_attention_key_bias_cross(dh):
    """T5 cross-attention shape: Lk = 256 with a padded tail masked by a -10000 bias."""
    from ltxmi import ops
    B, H, Lq, Lk = 3, 4, 300, 256
    q, k, v = rnd(B, Lq, H, dh, seed=23), rnd(B, Lk, H, dh, seed=24), rnd(B, Lk, H, dh, seed=25)
    bias = torch.zeros(B, Lk)
    bias[0, 96:] = -10000.0
    bias[1, 10:] = -10000.0
    bias[2, :] = torch.randn(Lk, generator=torch.Generator().manual_seed(1))     # a soft bias
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), key_bias=bias.to(DEV))
    check(out, attn_truth(q, k, v, bias), what="cross")


@pytest.mark.parametrize("B,H,Lq,Lk,bias", [(3, 32, 4992, 256, True),       # the DiT's cross-attention (5 row groups per (batch, head))
                                            (2, 8, 1500, 200, True),        # ragged last key tile, ragged last iteration
                                            (1, 5, 1024, 1, False), (2, 3, 2049, 64, False), (1, 4, 1100, 130, True),
                                            (1, 40, 9000, 256, False)])     # more (batch, head) pairs than fit at once
def test_attention_short_key_sequences_kernel(B, H, Lq, Lk, bias):
    """attention_cross.hip (kernel id 7): head_dim 64, <= 256 keys resident in LDS, every query row's scores in registers at
    once, single-pass softmax.  Against the fp32 oracle on the same bf16 inputs: hard (-10000) and soft key biases, key
    counts that are not multiples of 64 (keys past Lk must not contribute), row counts that are not multiples of 128, k / v as
    strided halves of one [B, Lk, 2, H, dh] projection buffer (how the DiT hands them over), a segmented output, q finished
    on load (RMSNorm factor per row + weight) against the two-pass form."""
    from ltxmi import ops
    dh = 64
    assert ops.attention_kernel_id(B, H, Lq, Lk, dh, bias, 2 * H * dh, 2 * H * dh) == 7
    q = rnd(B, Lq, H, dh, seed=70)
    kv = rnd(B, Lk, 2, H, dh, seed=71)
    k, v = kv[:, :, 0], kv[:, :, 1]
    kb = None
    if bias:
        kb = torch.zeros(B, Lk)
        kb[0, Lk - Lk // 3:] = -10000.0                                     # the padded tail of a prompt
        if B > 1:
            kb[1] = torch.randn(Lk, generator=torch.Generator().manual_seed(2))        # a soft bias
    kvd = kv.to(DEV)
    out = ops.attention(q.to(DEV), kvd[:, :, 0], kvd[:, :, 1], key_bias=None if kb is None else kb.to(DEV))
    rows = torch.cat([torch.arange(0, min(Lq, 160)), torch.arange(Lq - 140, Lq)]).unique()     # first rows, last (ragged) rows
    truth = attn_truth(q[:, rows], k, v, kb)
    check(out[:, rows], truth, what=f"short-key attention B{B} H{H} Lq{Lq} Lk{Lk}")
    if Lq <= 2100:
        check(out, attn_truth(q, k, v, kb), what=f"short-key attention, whole tensor, Lq{Lq} Lk{Lk}")
    # segmented output (the Ulysses return exchange's send buffer): tokens in segments of Lq / 4
    if Lq % 4 == 0:
        seg = Lq // 4
        buf = torch.zeros(4, B, seg, H, dh, dtype=BF, device=DEV)
        ops.attention(q.to(DEV), kvd[:, :, 0], kvd[:, :, 1], key_bias=None if kb is None else kb.to(DEV), out=buf[0],
                      out_segments=(seg, B * seg * H * dh))
        assert torch.equal(buf.permute(1, 0, 2, 3, 4).reshape(B, Lq, H, dh), out)
    # q finished on load: raw projection rows + one RMSNorm factor per row + weight
    D = H * dh
    g = torch.Generator(device=DEV).manual_seed(72)
    qraw = (torch.randn(B * Lq, D, generator=g, device=DEV) * 1.7).to(BF)
    wq = (1.0 + 0.1 * torch.randn(D, generator=g, device=DEV)).to(BF)
    ss = qraw.float().reshape(B * Lq, D // 64, 64).pow(2).sum(-1).contiguous()
    rstd = ops.rowsumsq_rstd(ss, D, 1e-6)
    ref = qraw.clone()
    ops.rmsnorm_rope_(ref, wq, 1e-6)
    kbd = None if kb is None else kb.to(DEV)
    two_pass = ops.attention(ref.view(B, Lq, H, dh), kvd[:, :, 0], kvd[:, :, 1], key_bias=kbd)
    fused = ops.attention(qraw.view(B, Lq, H, dh), kvd[:, :, 0], kvd[:, :, 1], key_bias=kbd, q_norm=(rstd, wq, 1e-6))
    check(fused, two_pass.float(), rel_l2=2e-3, maxrel=1.6e-2, what="short-key attention, q finished on load vs two passes")
    fused_ss = ops.attention(qraw.view(B, Lq, H, dh), kvd[:, :, 0], kvd[:, :, 1], key_bias=kbd, q_norm=(ss, wq, 1e-6))
    check(fused_ss, fused.float(), rel_l2=5e-4, maxrel=8e-3, what="short-key attention, partial sums vs row factor")


def test_attention_fused_qkv_views_and_scale():
    """q/k/v as strided slices of one [B, N, 3, H, dh] projection buffer, custom softmax scale."""
    from ltxmi import ops
    B, N, H, dh = 2, 190, 2, 64
    qkv = rnd(B, N, 3, H, dh, seed=26).to(DEV)
    out = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], softmax_scale=0.07)
    c = qkv.cpu()
    check(out, attn_truth(c[:, :, 0], c[:, :, 1], c[:, :, 2], scale=0.07), what="fused views")


def test_attention_online_softmax_rescale_branch():
    """Force the running max to jump late in the key sequence (guide rule 26): one key row is
    strongly aligned with the queries in the LAST tile, so every earlier tile's O/l must be
    rescaled exactly once."""
    from ltxmi import ops
    B, H, Lq, Lk, dh = 1, 2, 96, 448, 64
    q, k, v = rnd(B, Lq, H, dh, seed=27), rnd(B, Lk, H, dh, seed=28), rnd(B, Lk, H, dh, seed=29)
    k[:, 400] = q[:, 5] * 3.0          # spike in tile 6 of 7
    k[:, 70] = q[:, 40] * 2.0          # and an earlier, smaller one
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    check(out, attn_truth(q, k, v), what="rescale branch")


@pytest.mark.parametrize("Lq,Lk,spike", [(256, 1, False), (256, 64, False), (300, 65, False), (257, 130, False),
                                         (256, 200, False), (512, 448, True), (256, 1029, True)])
def test_attention_pipelined_kernel_edges(Lq, Lk, spike):
    """Shapes with >= 192 query tiles of 256 rows take the software-pipelined LDS-DMA kernel
    (attention_pipe.hip).  Its edges: a single (ragged) key tile, exactly one full tile, one full + a ragged
    tile, key tiles whose ring slots are never filled, ragged query tiles, and the rescale branch with the
    running max jumping late (block A and block B of a wave at different tiles)."""
    from ltxmi import ops
    B, H, dh = 8, 64 if Lq <= 256 else 32, 64
    q, k, v = rnd(B, Lq, H, dh, seed=40), rnd(B, Lk, H, dh, seed=41), rnd(B, Lk, H, dh, seed=42)
    if spike:
        k[:, Lk - 30] = q[:, 5] * 3.0           # last tile, hits rows of block A (rows 0..31 of wave 0)
        k[:, Lk // 2] = q[:, 40] * 2.0          # block B
        k[:, 70] = q[:, 100] * 2.5
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    check(out, attn_truth(q, k, v), what=f"pipelined attention Lq{Lq} Lk{Lk}")


@pytest.mark.parametrize("Lq,Lk,spike", [(256, 1, False), (256, 200, False), (512, 448, "redo"), (256, 1029, "redo"), (300, 1029, "late"),
                                         (256, 1029, "low"), (512, 448, "edge")])
def test_attention_pipelined_kernel_steady_form_and_redo(Lq, Lk, spike):
    """The head_dim-64 pipelined kernel's normal run is the "steady" form: P = 2^s against the reference 0 for every row (no
    tile maximum, no subtraction, no rescale); a workgroup in which a row sum / accumulator leaves [2^-100, 2^100) redoes
    its item with the exact online softmax.  Cases: one (ragged) key tile; a late maximum inside the steady range; scores
    far above the range in the last tile and in the middle (rows of block A and block B) -> redo, incl. rows around the
    +126 .. +128-bit edge where the sum stays finite but 1 / l would be denormal; "low": a row whose scores ALL lie
    ~115 bits below 0 (its sum underflows) -> redo; "edge": rows with maxima of about +-90 bits, inside the range."""
    from ltxmi import ops
    B, H, dh = 8, 64 if Lq <= 256 else 32, 64
    assert ops.attention_kernel_id(B, H, Lq, Lk, dh, False, H * dh, H * dh) == 3
    q, k, v = rnd(B, Lq, H, dh, seed=46), rnd(B, Lk, H, dh, seed=47), rnd(B, Lk, H, dh, seed=48)
    if spike == "late":
        k[:, Lk - 30] = q[:, 5] * 2.0           # ~ +16 nats in the last tile
        k[:, Lk // 2] = q[:, 40] * 1.5
    if spike == "redo":
        k[:, Lk - 30] = q[:, 5] * 40.0          # q.k c ~ 40 * 64 / 8 = 320 nats
        k[:, Lk // 2] = q[:, 40] * 11.0         # ~ +88 nats = 127 bits: around the denormal-reciprocal edge for its row
    if spike in ("low", "edge"):
        # every key gets a component along -q[5] (and, "edge", +q[40] on one key): row 5's scores all sit at
        # -(amount) * |q5| / 8 nats: "low" ~ -80 nats = -115 bits, "edge" ~ -62 nats = -90 bits
        qf = q.float()
        u = qf[:, 5] / qf[:, 5].norm(dim=-1, keepdim=True)                    # [B, H, dh]
        k = (k.float() - (80.0 if spike == "low" else 62.0) * u[:, None]).to(BF)
        if spike == "edge":
            k[:, Lk // 2] = (qf[:, 40] * 7.8).to(BF)                          # ~ +62 nats = +90 bits for row 40
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    check(out, attn_truth(q, k, v), what=f"pipelined attention (steady form) Lq{Lq} Lk{Lk} spike={spike}")


@pytest.mark.parametrize("Lq,Lk,spike", [(256, 1024, "none"), (300, 1029, "late"), (256, 1100, "redo"), (512, 1500, "redo")])
def test_attention_pipelined_kernel_head_dim_128(Lq, Lk, spike):
    """The head_dim-128 pipelined kernel (attention_pipe128.hip: >= 128 query tiles of 256 rows, >= 1024 keys).  Its
    first two key tiles run the exact online softmax (rescale whenever a row maximum grows); from then on every row keeps
    its reference ("steady" form, no rescale in the loop) and a workgroup in which a score outgrows its reference by more
    than 100 bits redoes its item in the exact form.  Cases: settled maxima; a maximum that jumps late but stays within the
    steady form's range (P > 1 against the old reference: rule 26, the branch that is wrong whenever taken needs its own
    test); and scores 400+ bits above everything before them in the LAST tile / in the middle -> the redo path, for block A
    and block B rows."""
    from ltxmi import ops
    B, H, dh = 4, 32, 128
    assert ops.attention_kernel_id(B, H, Lq, Lk, dh, False, H * dh, H * dh) == 6
    q, k, v = rnd(B, Lq, H, dh, seed=43), rnd(B, Lk, H, dh, seed=44), rnd(B, Lk, H, dh, seed=45)
    if spike == "late":
        k[:, Lk - 30] = q[:, 5] * 1.5           # ~ +17 nats in the last tile: block A rows of wave 0
        k[:, Lk // 2] = q[:, 40] * 1.2          # block B
    if spike == "redo":
        k[:, Lk - 30] = q[:, 5] * 30.0          # q.k c ~ 30 * 128 / sqrt(128) = 340 nats above the rest
        k[:, Lk // 2] = q[:, 40] * 25.0
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    check(out, attn_truth(q, k, v), what=f"head_dim-128 pipelined attention Lq{Lq} Lk{Lk} spike={spike}")


def _time_ms(fn, iters=10):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def test_attention_trained_like_logits_and_the_redo_counter():
    """the steady (reference-0) form is only ever TIMED on random-init logits of a few nats.  Here, at the
    workload's shape (B 3, H 32, N 4992, head_dim 64): (1) trained-like logits -- row maxima of 30-50 nats, softmax nearly
    one-hot -- must need NO redo (device counter) and sit inside the oracle band; (2) with a score of ~+85 nats planted in
    10 % of the (batch, head, query tile) items exactly those items are redone (counter), the result stays inside the band,
    and the time is printed next to the all-steady and the all-exact (``force_exact``) launches."""
    from ltxmi import ops
    B, H, N, dh = 3, 32, 4992, 64
    assert ops.attention_kernel_id(B, H, N, N, dh, False, H * dh, H * dh) == 3
    # "trained-like": every query has ONE key it is aligned with (its own token's: the diagonal of self-attention) at ~+40 nats,
    # all other pairs are noise of ~6 nats -- a softmax that is nearly one-hot, with its maximum anywhere in the key sequence.
    # (Plain N(0, sigma^2) q / k with the same typical maxima do not work as a NO-redo case: q.k is a sum of products of
    # normals, its far tail is much heavier than a Gaussian's, and among 2.4e9 scores one lands beyond +69 nats -- measured.)
    q, v = rnd(B, N, H, dh, seed=60, scale=2.0), rnd(B, N, H, dh, seed=62)
    qf = q.float()
    k = (rnd(B, N, H, dh, seed=61, scale=2.0).float() + qf * (40.0 * 8.0 / (qf * qf).sum(-1, keepdim=True))).to(BF)
    rows = torch.cat([torch.arange(0, 64), torch.arange(2500, 2564), torch.arange(N - 64, N)])      # a band of query rows
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)

    def band_truth(qq, kk):
        return attn_truth(qq[:, rows], kk, v)

    s = torch.einsum("bqhd,bkhd->bhqk", q[:1, rows].float(), k[:1].float()) / 8.0
    mx = s.amax(dim=-1)
    print(f"trained-like logits: row maxima {float(mx.min()):.1f} .. {float(mx.max()):.1f} nats (median {float(mx.median()):.1f})")
    assert 30.0 < float(mx.median()) < 50.0 and float(mx.max()) < 66.0
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.attention(qd, kd, vd, redo_counter=counter)
    assert int(counter.item()) == 0                                  # inside the steady form's range: nothing is redone
    check(out[:, rows], band_truth(q, k), what="trained-like logits, steady form")
    exact = ops.attention(qd, kd, vd, force_exact=True)
    check(exact[:, rows], band_truth(q, k), what="trained-like logits, exact form forced")
    t_steady = _time_ms(lambda: ops.attention(qd, kd, vd))
    t_exact = _time_ms(lambda: ops.attention(qd, kd, vd, force_exact=True))

    # ~10 % of the items beyond the range: per (batch, head) two query tiles get one row aligned with one key
    k2 = k.clone()
    tiles = (3, 11)                                                   # query tiles of 256 rows (of 20)
    for j, t in enumerate(tiles):
        row, key = 256 * t + 17 + 64 * j, 1000 + 2000 * j
        qrow = q[:, row].float()                                     # [B, H, dh]
        k2[:, key] = (qrow * (85.0 * 8.0 / (qrow * qrow).sum(-1, keepdim=True))).to(BF)       # score ~ +85 nats = 123 bits
    rows2 = torch.cat([rows, torch.tensor([256 * 3 + 17, 256 * 11 + 17 + 64, 256 * 3 + 100])])
    counter.zero_()
    k2d = k2.to(DEV)
    out2 = ops.attention(qd, k2d, vd, redo_counter=counter)
    n_items = B * H * ((N + 255) // 256)
    assert int(counter.item()) == len(tiles) * B * H, (int(counter.item()), n_items)
    check(out2[:, rows2], attn_truth(q[:, rows2], k2, v), what="10 % of the items redone")
    t_redo = _time_ms(lambda: ops.attention(qd, k2d, vd))
    qr, kr = rnd(B, N, H, dh, seed=63).to(DEV), rnd(B, N, H, dh, seed=64).to(DEV)
    t_rand = _time_ms(lambda: ops.attention(qr, kr, vd))
    print(f"attention B{B} H{H} N{N}: N(0,1) q / k (what random-init weights give) {t_rand:.3f} ms;  trained-like logits: all steady "
          f"{t_steady:.3f} ms, {len(tiles) * B * H}/{n_items} items redone {t_redo:.3f} ms, exact form forced {t_exact:.3f} ms")
    # (times are reported, not asserted, beyond their order: a redone item runs twice, the second time in the slower form)
    assert t_steady < t_redo < t_exact * 1.5


def test_pay_attention_seam_contract():
    from ltxmi import pay_attention
    B, L, H, dh = 2, 130, 2, 64
    q, k, v = rnd(B, L, H, dh, seed=30), rnd(B, 77, H, dh, seed=31), rnd(B, 77, H, dh, seed=32)
    lst = [q.to(DEV), k.to(DEV), v.to(DEV)]
    out = pay_attention(lst)
    assert lst == []                                     # the callee clears the list (:185-186)
    assert out.shape == (B, L, H, dh) and out.dtype == BF
    check(out, attn_truth(q, k, v), what="seam")
    with pytest.raises(NotImplementedError):
        pay_attention([q.to(DEV), k.to(DEV), v.to(DEV)], causal=True)
    with pytest.raises(TypeError):
        pay_attention([q.to(DEV).float(), k.to(DEV).float(), v.to(DEV).float()])
    # k_lens on a single sample: keys beyond k_lens are ignored, queries beyond q_lens are padding
    out = pay_attention([q[:1].to(DEV), k[:1].to(DEV), v[:1].to(DEV)], k_lens=torch.tensor([50]),
                        q_lens=torch.tensor([100]))
    assert out.shape == (1, L, H, dh)
    check(out[:, :100], attn_truth(q[:1, :100], k[:1, :50], v[:1, :50]), what="k_lens")


# -------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("D", [64, 128, 2048, 4096])
@pytest.mark.parametrize("kind", ["rms", "layer"])
def test_norm_modulate(D, kind):
    from ltxmi import ops
    B, F, hw = 2, 3, 37
    rows = B * F * hw
    x = rnd(rows, D, seed=40, scale=2.0)
    table, temb = rnd(6, D, seed=41, scale=0.3), rnd(B * F, 6 * D, seed=42, scale=0.3)
    xf = x.float()
    if kind == "rms":
        n = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)
    else:
        n = torch.nn.functional.layer_norm(xf, (D,), None, None, 1e-6)
    scale = (table[1].float()[None] + temb[:, D:2 * D].float()).repeat_interleave(hw, 0)
    shift = (table[0].float()[None] + temb[:, 0:D].float()).repeat_interleave(hw, 0)
    truth = n * (1 + scale) + shift
    y = torch.empty(rows, D, dtype=BF, device=DEV)
    td, ed = table.to(DEV), temb.to(DEV)
    ops.norm_modulate(x.to(DEV), y, 1e-6, ops.NORM_RMS if kind == "rms" else ops.NORM_LAYER,
                      td[1], ed[:, D:2 * D], td[0], ed[:, 0:D], hw)
    check(y, truth, what=f"norm_modulate {kind} {D}")


@pytest.mark.parametrize("D", [64, 128, 2048])
def test_rmsnorm_rope(D):
    from ltxmi import ops
    from oracle import dit, leaves
    B, N = 2, 75
    buf = rnd(B * N, 3 * D, seed=43)
    w = (1 + 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(1))).to(BF)
    cos = torch.cos(torch.randn(N, D, generator=torch.Generator().manual_seed(2))).to(BF)
    sin = torch.sin(torch.randn(N, D, generator=torch.Generator().manual_seed(3))).to(BF)
    d = buf.to(DEV).clone()
    ops.rmsnorm_rope_(d[:, D:2 * D], w.to(DEV), 1e-5, cos.to(DEV), sin.to(DEV), N)
    x = buf[:, D:2 * D].float().view(B, N, D)
    nrm = leaves.rms_norm(x, 1e-5, w.float())
    truth = dit.apply_rotary_emb(nrm, (cos.float()[None], sin.float()[None])).view(B * N, D)
    check(d[:, D:2 * D], truth, what="rmsnorm+rope")
    assert torch.equal(d[:, :D].cpu(), buf[:, :D]) and torch.equal(d[:, 2 * D:].cpu(), buf[:, 2 * D:])
    d2 = buf.to(DEV).clone()
    ops.rmsnorm_rope_(d2[:, :D], w.to(DEV), 1e-5)                                # no rope (cross-attention)
    check(d2[:, :D], leaves.rms_norm(buf[:, :D].float(), 1e-5, w.float()), what="rmsnorm only")


def test_small_pointwise():
    from ltxmi import ops
    from oracle import leaves
    x = rnd(5, 2048, seed=44, scale=3)
    check(ops.silu(x.to(DEV)), torch.nn.functional.silu(x.float()), what="silu")
    y = rnd(5, 2048, seed=45)
    check(ops.add(x.to(DEV), y.to(DEV)), x.float() + y.float(), what="add")
    t = torch.tensor([700.0, 50.0, 0.0, 999.0])
    emb = ops.timestep_embedding(t.to(DEV), 256)
    check(emb, leaves.get_timestep_embedding(t, 256, flip_sin_to_cos=True, downscale_freq_shift=0.0),
          rel_l2=4e-3, what="sinusoid")
    a, v = rnd(3, 20, 128, seed=46), rnd(3, 20, 128, seed=47)
    m = torch.tensor([1.0, 0.0, 0.25])
    d = a.to(DEV).clone()
    ops.stg_blend_(d, v.to(DEV), m.to(DEV))
    check(d, a.float() * m[:, None, None] + v.float() * (1 - m[:, None, None]), what="stg blend")


def test_timestep_embedding_kernel_against_the_references_own_sinusoid(golden):
    """G0: ``ltxmi_timestep_embedding_bf16`` against the reference's own ``get_timestep_embedding``
    (ltx_video/models/transformers/embeddings.py:10-50; golden generated by importing it untouched) on scaled, fractional,
    zero and per-frame timestep values -- bf16 outputs of values in [-1, 1]: one rounding (<= 2^-9) plus the kernel's fp32
    argument reduction at arguments up to 1000 rad."""
    from ltxmi import ops
    t, _ = golden("g0_timestep_embedding")
    emb = ops.timestep_embedding(t["timesteps"].to(DEV), 256)
    want = t["emb_256_flip_shift0"]
    assert emb.shape == want.shape and emb.dtype == BF
    err = (emb.float().cpu() - want).abs().max()
    assert float(err) <= 2.0 ** -8, float(err)
    check(emb, want, rel_l2=3e-3, what="sinusoid vs the reference's own")


# ------------------------------------------------------------------------------ VAE
def ndhwc(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def ncdhw(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("mode", ["zeros", "replicate"])
@pytest.mark.parametrize("cin,cout,shape", [(64, 128, (1, 3, 5, 7)), (128, 48, (2, 2, 4, 6)), (64, 264, (1, 1, 3, 3))])
def test_conv3d(causal, mode, cin, cout, shape):
    from ltxmi import ops
    from oracle import vae as ov
    B, T, H, W = shape
    x = rnd(B, cin, T, H, W, seed=50)
    w = rnd(cout, cin, 3, 3, 3, seed=51, scale=(27 * cin) ** -0.5)
    b = rnd(cout, seed=52)
    truth = ov.causal_conv3d(x.float(), {"conv.weight": w.float(), "conv.bias": b.float()}, "", causal, mode)
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()
    out = ops.conv3d(ndhwc(x).to(DEV), wp.to(DEV), b.to(DEV), causal, mode == "replicate")
    check(ncdhw(out.cpu()), truth, what=f"conv3d {causal} {mode} {cin}->{cout}")


def test_conv3d_big_tile_and_add():
    """The fused skip-add epilogue at 24576 positions x 256 channels: by shape (192 direct tiles) the eight-wave direct
    convolution.  (The implicit GEMM's 256 x 256 tile needs 384 of them: tests/test_gpu_conv_paths.py runs it.)"""
    from ltxmi import ops
    from oracle import vae as ov
    B, T, H, W, cin, cout = 1, 6, 64, 64, 64, 256
    x = rnd(B, cin, T, H, W, seed=53)
    w = rnd(cout, cin, 3, 3, 3, seed=54, scale=(27 * cin) ** -0.5)
    b = rnd(cout, seed=55)
    skip = rnd(B, cout, T, H, W, seed=56)
    truth = ov.causal_conv3d(x.float(), {"conv.weight": w.float(), "conv.bias": b.float()}, "", False, "replicate")
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()
    args = (ndhwc(x).to(DEV), wp.to(DEV), b.to(DEV), False, True)
    r = ops.conv3d_route(*args, add=ndhwc(skip).to(DEV))
    assert (r["route"], r["epilogue"], r["ksplit"]) == (ops.CONV_DIRECT8, 1, 1), r
    out = ops.conv3d(*args, add=ndhwc(skip).to(DEV))
    check(ncdhw(out.cpu()), truth + skip.float(), what="conv3d big + add")


@pytest.mark.parametrize("residual,red", [(True, 2), (False, 1), (True, 1)])
def test_conv3d_depth_to_space(residual, red):
    from ltxmi import autoencoder as ae
    from oracle import vae as ov
    cin = 64
    blk = ae.DepthToSpaceUpsample(3, cin, (2, 2, 2), residual=residual, out_channels_reduction_factor=red,
                                  spatial_padding_mode="replicate").to(BF)
    sd = {k: v.detach().float() for k, v in blk.state_dict().items()}
    x = rnd(1, cin, 3, 4, 5, seed=57)
    truth = ov.depth_to_space_upsample(x.float(), sd, "", dict(stride=(2, 2, 2), residual=residual, reduction=red),
                                       False, "replicate")
    out = blk.to(DEV)(ndhwc(x).to(DEV), causal=False)
    check(ncdhw(out.cpu()), truth, what=f"d2s res={residual} red={red}")


@pytest.mark.parametrize("C", [64, 128, 1024])
def test_pixelnorm_ada_silu_and_layernorm(C):
    from ltxmi import ops
    from oracle import vae as ov
    B, T, H, W = 2, 2, 3, 5
    x = rnd(B, C, T, H, W, seed=58, scale=2)
    g = torch.Generator().manual_seed(59)
    scale, shift = torch.randn(B, C, generator=g) * 0.3, torch.randn(B, C, generator=g) * 0.3
    xf = x.float()
    pn = ov.pixel_norm(xf)
    truth = torch.nn.functional.silu(pn * (1 + scale[:, :, None, None, None]) + shift[:, :, None, None, None])
    out = ops.pixelnorm_ada_silu(ndhwc(x).to(DEV), scale.to(DEV), shift.to(DEV), apply_silu=True)
    check(ncdhw(out.cpu()), truth, what="pixelnorm+ada+silu")
    out = ops.pixelnorm_ada_silu(ndhwc(x).to(DEV), None, None, apply_silu=False)
    check(ncdhw(out.cpu()), pn, what="pixelnorm")
    gamma, beta = rnd(C, seed=60), rnd(C, seed=61)
    out = ops.layernorm_affine(ndhwc(x).to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6)
    truth = torch.nn.functional.layer_norm(ndhwc(xf), (C,), gamma.float(), beta.float(), 1e-6)
    check(out, truth, what="layernorm affine")


def test_layout_kernels_bit_exact():
    from ltxmi import ops
    from oracle import vae as ov
    z = rnd(2, 16, 3, 4, 5, seed=62)
    out = ops.ncdhw_to_ndhwc(z.to(DEV))
    assert torch.equal(out.cpu(), ndhwc(z))
    std, mean = torch.rand(16) + 0.5, torch.randn(16)
    out = ops.ncdhw_to_ndhwc(z.to(DEV), std.to(DEV), mean.to(DEV))
    check(out, ndhwc(z.float() * std.view(1, -1, 1, 1, 1) + mean.view(1, -1, 1, 1, 1)), what="un-normalise")
    x = rnd(2, 48, 3, 4, 5, seed=63)
    out = ops.unpatchify_to_ncdhw(ndhwc(x).to(DEV), 3, 4)
    assert torch.equal(out.cpu(), ov.unpatchify(x, 4, 1))


# --------------------------------------------------------------------- guidance + Euler
@pytest.mark.parametrize("lat_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg,stg,resc", [(3.0, 1.0, 0.7), (1.0, 1.0, 0.7), (3.0, 0.0, 1.0), (3.0, 1.0, 1.0)])
def test_guidance_step(cfg, stg, resc, lat_dtype):
    from ltxmi import ops
    from oracle import sched
    N, C = 4992, 128
    do_cfg, do_stg = cfg > 1.0, stg > 0.0
    gs = cfg if cfg > 1.0 else 0.0
    nc = 1 + int(do_cfg) + int(do_stg)
    npred = rnd(nc, N, C, seed=70)
    lat = torch.randn(1, N, C, generator=torch.Generator().manual_seed(71)).to(lat_dtype)
    dt = 0.0371
    truth_v = sched.guidance(npred.float(), nc, gs, stg, resc, do_cfg, do_stg, resc != 1.0)
    truth = lat.float() - dt * truth_v
    d = lat.to(DEV).clone()
    ws = torch.empty(ops.GUIDANCE_WORKSPACE_FLOATS, device=DEV)
    ops.guidance_step_(npred.to(DEV), d, dt, gs, stg, resc, do_cfg, do_stg, resc != 1.0, ws)
    if lat_dtype == torch.float32:
        torch.testing.assert_close(d.cpu(), truth, rtol=2e-4, atol=2e-5)
    else:
        check(d, truth, what="guidance bf16 latents")


# ------------------------------------------------------------------- encoder-side kernels
@pytest.mark.parametrize("stride", [(2, 1, 1), (1, 2, 2), (2, 2, 2)])
@pytest.mark.parametrize("mode", ["zeros", "replicate"])
@pytest.mark.parametrize("cin,cout,shape", [(64, 128, (1, 5, 6, 8)), (128, 72, (2, 4, 5, 7))])
def test_conv3d_strided(stride, mode, cin, cout, shape):
    """Strided causal convolutions of the encoder's compress_* blocks (odd and even extents)."""
    from ltxmi import ops
    from oracle import vae_encoder as oe
    B, T, H, W = shape
    x = rnd(B, cin, T, H, W, seed=70)
    w = rnd(cout, cin, 3, 3, 3, seed=71, scale=(27 * cin) ** -0.5)
    b = rnd(cout, seed=72)
    truth = oe.strided_causal_conv3d(x.float(), {"conv.weight": w.float(), "conv.bias": b.float()}, "", stride, mode)
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()
    out = ops.conv3d(ndhwc(x).to(DEV), wp.to(DEV), b.to(DEV), True, mode == "replicate", stride=stride)
    assert ncdhw(out.cpu()).shape == truth.shape
    check(ncdhw(out.cpu()), truth, what=f"strided conv3d {stride} {mode} {cin}->{cout}")


@pytest.mark.parametrize("stride,cin,cout", [((2, 1, 1), 64, 128), ((1, 2, 2), 64, 128), ((2, 2, 2), 64, 128),
                                              ((2, 2, 2), 128, 128)])
def test_space_to_depth_downsample(stride, cin, cout):
    from ltxmi import autoencoder as ae
    from oracle import vae_encoder as oe
    blk = ae.SpaceToDepthDownsample(3, cin, cout, stride, "replicate").to(BF)
    sd = {k: v.detach().float() for k, v in blk.state_dict().items()}
    T = 5 if stride[0] == 2 else 4
    x = rnd(2, cin, T, 4, 6, seed=73)
    prod = stride[0] * stride[1] * stride[2]
    truth = oe.space_to_depth_downsample(x.float(), sd, "", dict(stride=stride, group=cin * prod // cout), "replicate")
    out = blk.to(DEV)(ndhwc(x).to(DEV))
    assert ncdhw(out.cpu()).shape == truth.shape
    check(ncdhw(out.cpu()), truth, what=f"space-to-depth {stride} {cin}->{cout}")


def test_patchify_and_ndhwc_to_ncdhw():
    """Layout kernels are exact (bit copies; the normalisation is one fp32 op)."""
    from ltxmi import ops
    from oracle import vae as ov
    x = rnd(2, 3, 3, 8, 12, seed=74)
    out = ops.patchify_to_ndhwc(x.to(DEV), 4, 64).cpu()
    truth = ov.patchify(x, 4, 1)                                   # [B,48,T,2,3]
    assert out.shape == (2, 3, 2, 3, 64)
    assert torch.equal(ncdhw(out)[:, :48], truth) and not out[..., 48:].any()
    y = rnd(2, 2, 3, 4, 136, seed=75)                              # NDHWC rows with a padded channel count
    std, mean = torch.rand(128) + 0.5, torch.randn(128) * 0.2
    got = ops.ndhwc_to_ncdhw(y.to(DEV), 0, 128).cpu()
    assert torch.equal(got, ncdhw(y)[:, :128])
    got = ops.ndhwc_to_ncdhw(y.to(DEV), 128, 1).cpu()
    assert torch.equal(got, ncdhw(y)[:, 128:129])
    got = ops.ndhwc_to_ncdhw(y.to(DEV), 0, 128, std.to(DEV), mean.to(DEV)).cpu()
    want = ((ncdhw(y)[:, :128].float() - mean.view(1, -1, 1, 1, 1)) / std.view(1, -1, 1, 1, 1))
    check(got, want, what="normalize_latents layout pass")


# ----------------------------------------------------------- conditioning (i2v) step kernels
@pytest.mark.parametrize("lat_dtype", [torch.float32, torch.bfloat16])
def test_guidance_step_with_conditioning_mask(lat_dtype):
    """denoising_step with a conditioning mask (pipeline_ltx_video.py:1309-1342): hard-conditioned
    tokens never move, soft ones start once t <= 1 - strength."""
    from ltxmi import ops
    from oracle import sched
    N, C = 1200, 128
    npred = rnd(3, N, C, seed=80)
    lat = torch.randn(1, N, C, generator=torch.Generator().manual_seed(81)).to(lat_dtype)
    mask = torch.zeros(1, N)
    mask[:, :200] = 1.0
    mask[:, 200:400] = 0.6        # 1 - 0.6 = 0.4 < t: frozen at this step
    mask[:, 400:600] = 0.2        # 0.8 >= t: moves
    tsch = sched.set_timesteps(8, (1, C, 3, 20, 20))
    t = tsch[4]
    dt = float(t - tsch[5])
    v = sched.guidance(npred.float(), 3, 3.0, 1.0, 0.7, True, True, True)
    cur_t = torch.min(t.expand(1).unsqueeze(-1), 1.0 - mask)
    truth = sched.denoising_step(tsch, lat.float(), v, cur_t, mask, t)
    d = lat.to(DEV).clone()
    ws = torch.empty(ops.GUIDANCE_WORKSPACE_FLOATS, device=DEV)
    ops.guidance_step_(npred.to(DEV), d, dt, 3.0, 1.0, 0.7, True, True, True, ws, cond_mask=mask.to(DEV), t=float(t))
    assert 0.4 < float(t) < 0.8, float(t)
    assert torch.equal(d.cpu()[:, :400], lat[:, :400])                      # frozen tokens are bit-identical
    if lat_dtype == torch.float32:
        torch.testing.assert_close(d.cpu(), truth, rtol=2e-4, atol=2e-5)
    else:
        check(d, truth, what="masked guidance step, bf16 latents")


@pytest.mark.parametrize("lat_dtype", [torch.float32, torch.bfloat16])
def test_image_cond_noise(lat_dtype):
    from ltxmi import ops
    from oracle import conditioning as oc
    N, C = 777, 128
    g = torch.Generator().manual_seed(82)
    lat, init, noise = [torch.randn(1, N, C, generator=g).to(lat_dtype) for _ in range(3)]
    mask = torch.zeros(1, N)
    mask[:, :100] = 1.0
    mask[:, 100:300] = 0.9
    truth = oc.add_noise_to_image_conditioning_latents(0.63, init.float(), lat.float(), 0.15, mask, noise.float())
    d = lat.to(DEV).clone()
    ops.image_cond_noise_(d, init.to(DEV), noise.to(DEV), mask.to(DEV), 0.15, 0.63)
    assert torch.equal(d.cpu()[:, 100:], lat[:, 100:])
    if lat_dtype == torch.float32:
        torch.testing.assert_close(d.cpu(), truth, rtol=1e-6, atol=1e-6)
    else:
        check(d, truth, what="image cond noise bf16")


# ------------------------------------------------------------ multi-scale bridge kernels
@pytest.mark.parametrize("kernel_t,tzero", [(3, True), (1, False)])
@pytest.mark.parametrize("cin,cout,shape", [(64, 128, (2, 3, 5, 7)), (128, 256, (1, 2, 4, 4))])
def test_conv3d_plain_zero_padded_and_2d(kernel_t, tzero, cin, cout, shape):
    """nn.Conv3d(padding=1) (zero padding on all three axes) and per-frame nn.Conv2d(padding=1)
    of LatentUpsampler (latent_upsampler.py:78-100)."""
    import torch.nn.functional as F
    from ltxmi import ops
    B, T, H, W = shape
    x = rnd(B, cin, T, H, W, seed=90)
    b = rnd(cout, seed=92)
    if kernel_t == 3:
        w = rnd(cout, cin, 3, 3, 3, seed=91, scale=(27 * cin) ** -0.5)
        truth = F.conv3d(x.float(), w.float(), b.float(), padding=1)
        wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()
    else:
        w = rnd(cout, cin, 3, 3, seed=91, scale=(9 * cin) ** -0.5)
        xf = x.float().permute(0, 2, 1, 3, 4).reshape(B * T, cin, H, W)
        truth = F.conv2d(xf, w.float(), b.float(), padding=1).view(B, T, cout, H, W).permute(0, 2, 1, 3, 4)
        wp = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()
    out = ops.conv3d(ndhwc(x).to(DEV), wp.to(DEV), b.to(DEV), False, False, kernel_t=kernel_t, time_pad_zeros=tzero)
    check(ncdhw(out.cpu()), truth, what=f"plain conv kt={kernel_t} {cin}->{cout}")


@pytest.mark.parametrize("C,per_frame,with_res", [(64, False, False), (512, False, True), (128, True, True),
                                                  (2048, False, False)])
def test_groupnorm_silu(C, per_frame, with_res):
    import torch.nn.functional as F
    from ltxmi import ops
    B, T, H, W = 2, 3, 5, 7
    x = rnd(B, C, T, H, W, seed=93, scale=2) + 0.3
    res = rnd(B, C, T, H, W, seed=94) if with_res else None
    gamma, beta = (1 + 0.1 * rnd(C, seed=95).float()).to(BF), rnd(C, seed=96, scale=0.1)
    xf = x.float()
    if per_frame:
        xf = xf.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
    gn = F.group_norm(xf, 32, gamma.float(), beta.float(), 1e-5)
    if per_frame:
        gn = gn.view(B, T, C, H, W).permute(0, 2, 1, 3, 4)
    truth = F.silu(gn + (res.float() if with_res else 0))
    out = ops.groupnorm_silu(ndhwc(x).to(DEV), gamma.to(DEV), beta.to(DEV), 32, 1e-5,
                             residual=ndhwc(res).to(DEV) if with_res else None,
                             samples=B * T if per_frame else B)
    check(ncdhw(out.cpu()), truth, what=f"groupnorm+silu C={C}")


def test_pixel_shuffle2d_is_exact():
    from ltxmi import ops
    from oracle import upsampler as up
    B, T, H, W, C = 2, 3, 4, 5, 64
    x = rnd(B * T, 4 * C, H, W, seed=97)                       # reference channel order (c p1 p2)
    truth = up.pixel_shuffle(x, 2).view(B, T, C, 2 * H, 2 * W).permute(0, 2, 1, 3, 4)
    xp = x.view(B * T, C, 4, H, W).transpose(1, 2).reshape(B, T, 4 * C, H, W)      # packed (p1 p2 c)
    out = ops.pixel_shuffle2d(xp.permute(0, 1, 3, 4, 2).contiguous().to(DEV))
    assert torch.equal(ncdhw(out.cpu()), truth)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_adain_filter(dtype):
    from ltxmi import ops
    from oracle import upsampler as up
    g = torch.Generator().manual_seed(98)
    lat = (torch.randn(2, 128, 3, 8, 10, generator=g) * 1.7 + 0.4).to(dtype)
    ref = (torch.randn(2, 128, 3, 4, 5, generator=g) * 0.6 - 0.2).to(dtype)
    for factor in (1.0, 0.25):
        truth = up.adain_filter_latent(lat.float(), ref.float(), factor)
        out = ops.adain_filter(lat.to(DEV), ref.to(DEV), factor)
        if dtype == torch.float32:
            torch.testing.assert_close(out.cpu(), truth, rtol=1e-4, atol=1e-5)
        else:
            check(out, truth, what="adain bf16")


# ------------------------------------------------------------------ randomised shape sweeps
def test_gemm_kernels_agree_bit_for_bit():
    """The dispatcher picks a kernel by shape (128x128 tiles / persistent 256x256; algo 128 / 256 force the 128x128 and the
    non-persistent 256x256 tile kernels: the ids are asserted).  All of them accumulate over K in
    the same order with the same MFMA shape and share the epilogue arithmetic, so a row's result does not depend on the
    choice -- which is what makes running a sub-batch of rows bit-identical to running them all (stg_alias_blocks)."""
    from ltxmi import ops
    # (id by shape: 64 / 144 / 640 / 96 tiles of 256x256 against the persistent kernel's floor of 128)
    for case, (M, N, K, by_shape) in enumerate([(2048, 2048, 2048, 0), (1500, 6144, 1024, 2), (4992, 8192, 2048, 2), (3000, 2048, 4096, 0)]):
        a, w, b = rnd(M, K, seed=40 + case).to(DEV), rnd(N, K, seed=50 + case, scale=K ** -0.5).to(DEV), rnd(N, seed=60 + case).to(DEV)
        res = rnd(M, N, seed=70 + case).to(DEV)
        gt, ge = rnd(N, seed=80 + case).to(DEV), rnd(3, N, seed=90 + case).to(DEV)
        for epi in (ops.EPI_NONE, ops.EPI_GELU_TANH, ops.EPI_SILU, ops.EPI_GATE_RESIDUAL):
            kw = dict(residual=res, gate_table=gt, gate_temb=ge, rows_per_group=(M + 2) // 3) if epi == ops.EPI_GATE_RESIDUAL else {}
            assert [ops.gemm_kernel_id(a, w, b, epilogue=epi, algo=al, **kw) for al in (0, 128, 256)] == [by_shape, 0, 1]
            outs = [ops.gemm(a, w, b, epilogue=epi, algo=al, **kw) for al in (0, 128, 256)]
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"gemm {M}x{N}x{K} epi {epi}: kernels differ"
        # the row sums of squares the QKV projection hands to the attention kernel (q's RMSNorm factor)
        sums = []
        for al in (0, 128, 256):
            ss = torch.zeros(M, N // 64, device=DEV)
            assert ops.gemm_kernel_id(a, w, b, algo=al, rowsumsq=ss, rowsumsq_cols=N) == {0: by_shape, 128: 0, 256: 1}[al]
            o = ops.gemm(a, w, b, algo=al, rowsumsq=ss, rowsumsq_cols=N)
            sums.append(ss)
        assert torch.equal(sums[0], sums[1]) and torch.equal(sums[0], sums[2]), f"gemm {M}x{N}x{K}: row sums of squares differ between kernels"
        # the same rows inside a taller problem (another tile choice, another tile position)
        tall = torch.cat([a, a[: M // 2]], 0)
        o_tall = ops.gemm(tall, w, b, epilogue=ops.EPI_GELU_TANH)
        assert torch.equal(o_tall[:M], ops.gemm(a, w, b, epilogue=ops.EPI_GELU_TANH))


def test_gemm_random_shapes_persistent_path():
    """Seeded random (M, N, K) on the persistent 256x256 kernel (whatever ops.gemm_kernel_id says is one; a third of the
    cases below 384 tiles, where workgroups have one tile or a mix of one and two): ragged last M/N tiles through the
    per-tile buffer descriptors, odd tile counts per workgroup, every epilogue, a result that must stay in bounds (guard
    columns/rows around the output are checked untouched)."""
    import random
    from ltxmi import ops
    rng = random.Random(1234)
    few = 0
    for case in range(14):
        K = 64 * rng.randrange(2, 17)
        while True:
            M = rng.randrange(768, 9000)
            N = 8 * rng.randrange(32, 800)
            if ops.gemm_kernel_id(torch.empty(M, K, dtype=BF), torch.empty(N, K, dtype=BF)) != 2:
                continue
            if (((M + 255) // 256) * ((N + 255) // 256) < 384) == (case % 3 == 0):
                break
        few += case % 3 == 0
        epi = [ops.EPI_NONE, ops.EPI_GELU_TANH, ops.EPI_SILU, ops.EPI_GATE_RESIDUAL][case % 4]
        a, w, b = rnd(M, K, seed=200 + case), rnd(N, K, seed=300 + case, scale=K ** -0.5), rnd(N, seed=400 + case)
        pre = a.float() @ w.float().T + b.float()
        guard = torch.full((M + 2, N + 16), 7.0, dtype=BF, device=DEV)
        out = guard[1:M + 1, 8:N + 8]
        if epi == ops.EPI_GATE_RESIDUAL:
            res = rnd(M, N, seed=500 + case)
            out.copy_(res.to(DEV))
            assert ops.gemm_kernel_id(a.to(DEV), w.to(DEV), b.to(DEV), out=out, epilogue=epi, residual=out) == 2
            ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), out=out, epilogue=epi, residual=out)
            truth = res.float() + pre
        else:
            assert ops.gemm_kernel_id(a.to(DEV), w.to(DEV), b.to(DEV), out=out, epilogue=epi) == 2
            ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), out=out, epilogue=epi)
            truth = {ops.EPI_NONE: pre, ops.EPI_GELU_TANH: torch.nn.functional.gelu(pre, approximate="tanh"),
                     ops.EPI_SILU: torch.nn.functional.silu(pre)}[epi]
        check(out, truth, what=f"random gemm {M}x{N}x{K} epi{epi}")
        g = guard.clone()
        g[1:M + 1, 8:N + 8] = 7.0
        assert (g == 7.0).all(), f"random gemm {M}x{N}x{K}: wrote outside the output"
    assert few == 5


def test_attention_random_shapes():
    import random
    from ltxmi import ops
    rng = random.Random(99)
    for case in range(10):
        dh = rng.choice([64, 128])
        B, H = rng.randrange(1, 3), rng.randrange(1, 40)
        Lq, Lk = rng.randrange(1, 1500), rng.randrange(1, 1200)
        q, k, v = rnd(B, Lq, H, dh, seed=600 + case), rnd(B, Lk, H, dh, seed=700 + case), rnd(B, Lk, H, dh, seed=800 + case)
        bias = None
        if case % 2:
            bias = torch.zeros(B, Lk)
            bias[:, rng.randrange(0, Lk):] = -10000.0
            bias[:, 0] = 0.0
        out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), key_bias=None if bias is None else bias.to(DEV))
        check(out, attn_truth(q, k, v, bias), what=f"random attention B{B} H{H} Lq{Lq} Lk{Lk} dh{dh}")


# ------------------------------------------------- full-size, size-independent properties
def test_attention_full_size_properties_98k():
    """BASELINE's sequence length (N = 98 304) cannot be checked against the CPU oracle in seconds; these
    properties hold for softmax attention at any size: (a) V = 1 gives exactly-normalised rows, (b) the
    output is linear in V, (c) permuting the keys (with their values) does not change it, (d) a sub-block of
    queries matches the oracle computed for just those queries."""
    from ltxmi import ops
    N, H, dh = 98304, 2, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    q = torch.randn(1, N, H, dh, generator=g, device=DEV).to(BF)
    k = torch.randn(1, N, H, dh, generator=g, device=DEV).to(BF)
    v1 = torch.randn(1, N, H, dh, generator=g, device=DEV).to(BF)
    v2 = torch.randn(1, N, H, dh, generator=g, device=DEV).to(BF)
    ones = torch.ones_like(v1)
    o = ops.attention(q, k, ones).float()
    assert (o - 1.0).abs().max() < 8e-3                          # sum_j p_ij = 1 (bf16 output rounding)
    o1, o2 = ops.attention(q, k, v1).float(), ops.attention(q, k, v2).float()
    v3 = (0.5 * v1.float() + 0.25 * v2.float()).to(BF)
    o3 = ops.attention(q, k, v3).float()
    lin = 0.5 * o1 + 0.25 * o2
    # Tolerances (round 3: the file's own, derived -- the 2e-2 / 6e-2 of round 2 were not).  The kernel's error against
    # fp32 is one bf16 rounding of P (independent per key: relative 2^-9 / sqrt(3) rms on a random-sign sum, whatever N)
    # plus one bf16 rounding of the output (the same again): ~1.6e-3 rms relative, i.e. REL_L2 = 3e-3 holds at ANY
    # sequence length.  Linearity compares three such renderings (+ the bf16 rounding of v3 itself), the permutation two
    # independent ones: sqrt(4) x 1.1e-3 and sqrt(2) x 1.6e-3 -> 4e-3 bounds both.
    e_lin = float((o3 - lin).norm() / lin.norm())
    perm = torch.randperm(N, generator=g, device=DEV)
    op = ops.attention(q, k[:, perm], v1[:, perm]).float()
    e_perm = float((op - o1).norm() / o1.norm())
    print(f"98k attention: linearity {e_lin:.3e}, key permutation {e_perm:.3e}")
    assert e_lin < 4e-3 and e_perm < 4e-3, (e_lin, e_perm)
    rows = slice(50000, 50064)
    truth = attn_truth(q[:, rows].cpu(), k.cpu(), v1.cpu())
    e = check(o1[:, rows], truth, what="98k attention, 64 query rows vs oracle")
    print(f"98k attention: 64 query rows vs the fp32 oracle: rel L2 {e:.3e}")


def test_gemm_full_size_linearity_ff1_shape():
    """FF up-projection shape of the bench (14976 x 8192 x 2048): linear in A, and a 128-row band matches fp32."""
    from ltxmi import ops
    M, N, K = 14976, 8192, 2048
    g = torch.Generator(device=DEV).manual_seed(6)
    a1 = torch.randn(M, K, generator=g, device=DEV).to(BF)
    a2 = torch.randn(M, K, generator=g, device=DEV).to(BF)
    w = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(BF)
    o1, o2 = ops.gemm(a1, w).float(), ops.gemm(a2, w).float()
    a3 = (a1.float() + a2.float()).to(BF)                        # exact in bf16? not always: compare via fp32 truth
    o3 = ops.gemm(a3, w).float()
    truth3 = (a3[7000:7128].float() @ w.float().T)
    check(o3[7000:7128], truth3, what="FF1-shape band")
    lin = o1 + o2
    exact = a3.float() == (a1.float() + a2.float())              # rows where the bf16 sum is exact
    rows = exact.all(dim=1)
    if rows.any():
        assert (o3[rows] - lin[rows]).norm() / lin[rows].norm() < 6e-3


# ---------------------------------------------------------------- direct convolution path
@pytest.mark.parametrize("causal,mode,tzero", [(True, "zeros", False), (False, "replicate", False), (False, "zeros", True)])
@pytest.mark.parametrize("cin,cout,with_add", [(64, 128, False), (128, 256, True), (128, 48, False), (64, 200, True),
                                               (192, 128, True)])      # 1, 2 and 3 chunks of 64 input channels (odd / even tap streams)
@pytest.mark.parametrize("algo", [4, 3])
def test_conv3d_direct_path(causal, mode, tzero, cin, cout, with_add, algo):
    """Shapes the direct (LDS-halo) convolution takes, in both of its forms (algo 4: eight waves per workgroup, 64-channel
    chunks; algo 3: four waves, two workgroups per CU, 32-channel chunks -- where Cout is a multiple of 128, the eight-wave
    form otherwise), with partial tiles on every axis (T = 5, H = 36, W = 100 against 2 x 8 x 16 tiles)."""
    import torch.nn.functional as F
    from ltxmi import ops
    B, T, H, W = 2, 5, 36, 100
    x = rnd(B, cin, T, H, W, seed=110)
    w = rnd(cout, cin, 3, 3, 3, seed=111, scale=(27 * cin) ** -0.5)
    b = rnd(cout, seed=112)
    xf = x.float()
    if tzero:
        truth = F.conv3d(xf, w.float(), b.float(), padding=1)
    else:
        from oracle import vae as ov
        truth = ov.causal_conv3d(xf, {"conv.weight": w.float(), "conv.bias": b.float()}, "", causal, mode)
    add = rnd(B, cout, T, H, W, seed=113) if with_add else None
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()
    out = ops.conv3d(ndhwc(x).to(DEV), wp.to(DEV), b.to(DEV), causal, mode == "replicate",
                     add=ndhwc(add).to(DEV) if with_add else None, time_pad_zeros=tzero, algo=algo)
    check(ncdhw(out.cpu()), truth + (add.float() if with_add else 0), what=f"direct conv {cin}->{cout} algo {algo}")


@pytest.mark.parametrize("cin,ada,causal", [(128, True, False), (64, False, True), (192, True, True)])
def test_conv3d_post_norm_epilogue(cin, ada, causal):
    """ltxmi_conv3d_args.post_norm: PixelNorm -> (1 + scale) x + shift -> SiLU of the result in the epilogue of the four-wave
    direct convolution (Cout 128: one wave holds all channels of a position), from the fp32 accumulators -- against the oracle's
    fp32 convolution followed by the same arithmetic in fp32, and against the two-launch form; partial tiles on every axis;
    where the kernel cannot fuse (other forms / widths) the entry refuses and ops.conv3d runs the second launch."""
    import ctypes
    from ltxmi import ops, _lib
    from oracle import vae as ov
    B, T, H, W, cout = 2, 5, 36, 100, 128
    x = rnd(B, cin, T, H, W, seed=114)
    w = rnd(cout, cin, 3, 3, 3, seed=115, scale=(27 * cin) ** -0.5)
    b = rnd(cout, seed=116)
    scale, shift = (rnd(B, cout, seed=117, scale=0.3).float(), rnd(B, cout, seed=118, scale=0.3).float()) if ada else (None, None)
    y = ov.causal_conv3d(x.float(), {"conv.weight": w.float(), "conv.bias": b.float()}, "", causal, "replicate")
    n = y * torch.rsqrt(y.pow(2).mean(dim=1, keepdim=True) + 1e-8)
    if ada:
        n = n * (1 + scale[:, :, None, None, None]) + shift[:, :, None, None, None]
    truth = torch.nn.functional.silu(n)
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous().to(DEV)
    xd, bd = ndhwc(x).to(DEV), b.to(DEV)
    pn = (scale.to(DEV) if ada else None, shift.to(DEV) if ada else None, 1e-8)
    a = _lib.Conv3dArgs()
    a.bias, a.B, a.T, a.H, a.W, a.Cin, a.Cout, a.causal, a.pad_replicate, a.algo = bd.data_ptr(), B, T, H, W, cin, cout, int(causal), 1, 3
    assert _lib.lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)) == 1
    fused = ops.conv3d(xd, wp, bd, causal, True, algo=3, post_norm=pn)
    check(ncdhw(fused.cpu()), truth, what=f"conv {cin}->128 + post_norm (fused epilogue)")
    two = ops.conv3d(xd, wp, bd, causal, True, algo=3)
    two = ops.pixelnorm_ada_silu(two, pn[0], pn[1], True, 1e-8)
    check(fused, two.float(), rel_l2=4e-3, what="post_norm fused vs two launches")
    # the forms that cannot: the eight-wave form / the implicit GEMM (ops.conv3d then launches the norm itself) ...
    for algo in (4, 1):
        a.algo = algo
        assert _lib.lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)) == 0
        other = ops.conv3d(xd, wp, bd, causal, True, algo=algo, post_norm=pn)
        check(other, two.float(), rel_l2=4e-3, what=f"post_norm as a second launch (algo {algo})")
    # ... and the entry itself refuses post_norm = 1 there
    a.algo, a.x, a.w, a.y = 4, xd.data_ptr(), wp.data_ptr(), two.data_ptr()
    a.post_norm, a.post_eps = 1, 1e-8
    assert _lib.lib.ltxmi_conv3d_ndhwc_bf16(ctypes.byref(a), None) == -2        # LTXMI_ERR_UNSUPPORTED, nothing launched
    assert b"post_norm" in _lib.lib.ltxmi_last_error()


@pytest.mark.parametrize("kind", ["add", "d2s_res", "d2s"])
def test_conv3d_second_activated_output(kind):
    """ltxmi_conv3d_args.y_norm (0.5): the NEXT block's norm1 -> AdaLN -> SiLU as a second output of conv2 + skip (Cout 128) and
    of the depth-to-space store to 128 channels (causal_video_autoencoder.py:1197-1224, 771-795).  The raw output must be
    bit-identical to the same call without post_norm; the activated one must equal ltxmi_pixelnorm_ada_silu_bf16 of it (same
    fp32 arithmetic from the same bf16 values: at most a bf16 ulp apart).  Partial tiles on every axis, batch 2 with per-sample
    scale / shift.  A width the kernel cannot fuse returns the same pair through the second launch."""
    import ctypes
    from ltxmi import ops, _lib
    B, T, H, W = 2, 5, 20, 52
    d2s = kind != "add"
    cin, cout, c_out = (256, 1024, 128) if d2s else (128, 128, 128)
    x = ndhwc(rnd(B, cin, T, H, W, seed=130)).to(DEV)
    wp = rnd(cout, 27 * cin, seed=131, scale=(27 * cin) ** -0.5).to(DEV)
    b = rnd(cout, seed=132).to(DEV)
    add = None if d2s else ndhwc(rnd(B, cout, T, H, W, seed=133)).to(DEV)
    res = x if kind == "d2s_res" else None
    pn = (rnd(B, c_out, seed=134, scale=0.3).float().to(DEV), rnd(B, c_out, seed=135, scale=0.3).float().to(DEV), 1e-8)
    a = _lib.Conv3dArgs()
    a.bias, a.B, a.T, a.H, a.W, a.Cin, a.Cout, a.causal, a.pad_replicate, a.algo, a.d2s = b.data_ptr(), B, T, H, W, cin, cout, 1, 1, 3, int(d2s)
    a.add = add.data_ptr() if add is not None else None
    a.y_norm = x.data_ptr()                                  # (any non-NULL pointer: the query launches nothing)
    assert _lib.lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)) == 1
    plain = ops.conv3d(x, wp, b, True, True, d2s=d2s, residual=res, add=add, algo=3)
    raw, act = ops.conv3d(x, wp, b, True, True, d2s=d2s, residual=res, add=add, algo=3, post_norm=pn, keep_raw=True)
    torch.cuda.synchronize()
    assert raw.shape == plain.shape == act.shape
    assert torch.equal(raw, plain), f"{kind}: the raw output changed with the second output switched on"
    want = ops.pixelnorm_ada_silu(plain, pn[0], pn[1], True, 1e-8)
    d = (act.float() - want.float()).abs()
    tol = want.float().abs() * 2.0 ** -7 + 1e-6             # one bf16 ulp (fast-math reciprocal / exp in both)
    assert bool((d <= tol).all()), f"{kind}: activated output off by up to {float((d - tol).max()):.3e} beyond a bf16 ulp"
    assert float(d.max()) < 0.05 and float((act.float() - want.float()).norm() / want.float().norm()) < 2e-3
    # no scale / shift (a ResnetBlock3D without timestep conditioning)
    raw0, act0 = ops.conv3d(x, wp, b, True, True, d2s=d2s, residual=res, add=add, algo=3, post_norm=(None, None, 1e-8), keep_raw=True)
    want0 = ops.pixelnorm_ada_silu(plain, None, None, True, 1e-8)
    assert torch.equal(raw0, plain)
    assert float((act0.float() - want0.float()).norm() / want0.float().norm()) < 2e-3
    # the forms that cannot fuse: same pair, the norm as a launch of its own
    a.algo = 4
    assert _lib.lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)) == 0
    plain4 = ops.conv3d(x, wp, b, True, True, d2s=d2s, residual=res, add=add, algo=4)
    raw4, act4 = ops.conv3d(x, wp, b, True, True, d2s=d2s, residual=res, add=add, algo=4, post_norm=pn, keep_raw=True)
    assert torch.equal(raw4, plain4) and torch.equal(act4, ops.pixelnorm_ada_silu(plain4, pn[0], pn[1], True, 1e-8))
    # the entry refuses y_norm without post_norm, and y_norm == y
    a.algo, a.x, a.w, a.y, a.post_norm, a.y_norm = 3, x.data_ptr(), wp.data_ptr(), raw.data_ptr(), 0, act.data_ptr()
    assert _lib.lib.ltxmi_conv3d_ndhwc_bf16(ctypes.byref(a), None) == -1        # LTXMI_ERR_INVALID_ARG
    a.post_norm, a.post_eps, a.y_norm = 1, 1e-8, raw.data_ptr()
    assert _lib.lib.ltxmi_conv3d_ndhwc_bf16(ctypes.byref(a), None) == -1


@pytest.mark.parametrize("kind,grid", [("plain", (5, 16, 24)), ("add", (4, 20, 28)), ("post_norm", (5, 16, 24)),
                                       ("add_second", (3, 16, 24)), ("d2s_res_second", (3, 16, 24)), ("d2s", (5, 10, 24)),
                                       ("post_norm_512", (9, 32, 48)), ("add_second_512", (9, 30, 44))])
def test_conv3d_channel_split(kind, grid, monkeypatch):
    """ltxmi_conv3d_args.workspace (0.5): the wide, short layers of the decoder's 1024-channel stage split over their input
    channels (fp32 partial sums of 2 .. 4 ranges + a finalising pass that applies the epilogue, the norm at full width included),
    on tiles whose 16-position rows run along H.  Against the same call without a workspace (the unsplit kernels: equal up to the
    fp32 summation order, i.e. a bf16 ulp here and there) and against the fp32 oracle convolution; partial tiles on both axes."""
    import ctypes
    from ltxmi import ops, _lib
    from oracle import vae as ov
    # (..._512: the decoder's 512-channel stage, split in two only because the norm rides on the finalising pass)
    narrow = kind.endswith("_512")
    kind = kind.replace("_512", "")
    B, (T, H, W), cin = 2 if kind == "post_norm" else 1, grid, 512 if narrow else 1024
    d2s = kind.startswith("d2s")
    cout = 2048 if d2s else cin
    c_norm = cout // 8 if d2s else cout
    x = rnd(B, cin, T, H, W, seed=140)
    w = rnd(cout, cin, 3, 3, 3, seed=141, scale=(27 * cin) ** -0.5)
    b = rnd(cout, seed=142)
    xd, bd = ndhwc(x).to(DEV), b.to(DEV)
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1)
    if d2s:                                        # rows re-ordered (p1 p2 p3, c'): CausalConv3d.packed(d2s=True)
        wp, bdd = wp.view(cout // 8, 8, -1).transpose(0, 1).reshape(cout, -1), b.view(cout // 8, 8).t().reshape(cout).to(DEV)
    else:
        bdd = bd
    wp = wp.contiguous().to(DEV)
    add = ndhwc(rnd(B, cout, T, H, W, seed=143)).to(DEV) if kind.startswith("add") else None
    res = xd if kind.startswith("d2s_res") else None
    pn = None
    if "second" in kind or kind == "post_norm":
        pn = (rnd(B, c_norm, seed=144, scale=0.3).float().to(DEV), rnd(B, c_norm, seed=145, scale=0.3).float().to(DEV), 1e-8)
    keep = "second" in kind
    a = _lib.Conv3dArgs()
    a.bias, a.B, a.T, a.H, a.W, a.Cin, a.Cout, a.causal, a.pad_replicate, a.d2s = bdd.data_ptr(), B, T, H, W, cin, cout, 1, 1, int(d2s)
    if narrow:
        assert _lib.lib.ltxmi_conv3d_workspace_bytes(ctypes.byref(a)) == 0        # not without a norm to take along
        a.post_norm = 1
    want = _lib.lib.ltxmi_conv3d_workspace_bytes(ctypes.byref(a))
    assert want >= 2 * B * T * H * W * cout * 4 and want % (B * T * H * W * cout * 4) == 0, want
    a.post_norm = 0

    def run(fn=ops.conv3d):
        return fn(xd, wp, bdd, True, True, d2s=d2s, residual=res, add=add, post_norm=pn, keep_raw=keep)

    r = run(ops.conv3d_route)
    assert (r["route"], r["epilogue"], r["swap_hw"], r["finalize_blocks"], r["second_launch"]) == \
        (ops.CONV_DIRECT4, 6, int(not narrow and kind != "add"), cout // 256, False) and r["ksplit"] == want // (B * T * H * W * cout * 4), r
    split = run()
    monkeypatch.setattr(ops, "CONV_SPLIT", False)
    r = run(ops.conv3d_route)
    assert r["ksplit"] == 1 and r["epilogue"] < 6 and r["second_launch"] == (pn is not None), r
    plain = run()
    torch.cuda.synchronize()
    outs = list(zip(split, plain)) if keep else [(split, plain)]
    for sp_, pl_ in outs:
        assert sp_.shape == pl_.shape
        d = (sp_.float() - pl_.float()).abs()
        tol = pl_.float().abs() * 2.0 ** -6 + 2e-2           # two bf16 ulps of the value (summation order, then the norm's factor)
        assert bool((d <= tol).all()), f"{kind}: split vs unsplit off by {float((d - tol).max()):.3e} beyond two bf16 ulps"
        # (two bf16 renderings of the same tensor: the unsplit call of these small grids is the implicit GEMM, which adds `add`
        # before its one rounding, and at this width its norm is a second launch on the rounded result)
        assert float((sp_.float() - pl_.float()).norm() / pl_.float().norm()) < 6e-3
    # the raw result against the fp32 oracle (post_norm-only: the activated one)
    y = ov.causal_conv3d(x.float(), {"conv.weight": w.float(), "conv.bias": b.float()}, "", True, "replicate")
    if d2s:
        yt = ov.depth_to_space_upsample(x.float(), {"conv.conv.weight": w.float(), "conv.conv.bias": b.float()}, "",
                                        dict(stride=(2, 2, 2), residual=res is not None, reduction=4), True, "replicate")
        check(ncdhw((split[0] if keep else split).cpu()), yt, what=f"split {kind} vs oracle")
    elif kind == "post_norm":
        n = y * torch.rsqrt(y.pow(2).mean(dim=1, keepdim=True) + 1e-8)
        n = n * (1 + pn[0].cpu()[:, :, None, None, None]) + pn[1].cpu()[:, :, None, None, None]
        check(ncdhw(split.cpu()), torch.nn.functional.silu(n), what="split post_norm vs oracle")
    else:
        yt = y + (ncdhw(add.cpu()).float() if add is not None else 0)
        check(ncdhw((split[0] if keep else split).cpu()), yt, what=f"split {kind} vs oracle")
    # without a workspace the entry runs the unsplit kernels and refuses the norm at this width
    a.x, a.w, a.y, a.post_norm, a.post_eps = xd.data_ptr(), wp.data_ptr(), (plain[0] if keep else plain).data_ptr(), 1, 1e-8
    if d2s:
        a.y_norm = plain[1].data_ptr() if keep else xd.data_ptr()      # (the queries launch nothing)
    assert _lib.lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)) == 0
    ws = torch.empty(want, dtype=torch.uint8, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr(), want
    assert _lib.lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)) == 1
    a.workspace_bytes = want - 16                            # too small: not used
    assert _lib.lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)) == 0
    # the activated result as the ONLY output is for the plain store: with `add` / depth-to-space it needs y_norm
    a.workspace_bytes = want
    if add is not None or d2s:
        a.add = add.data_ptr() if add is not None else None
        a.y_norm = None
        assert _lib.lib.ltxmi_conv3d_fuses_post_norm(ctypes.byref(a)) == 0
        assert _lib.lib.ltxmi_conv3d_ndhwc_bf16(ctypes.byref(a), None) == -2 and b"post_norm" in _lib.lib.ltxmi_last_error()


def test_conv3d_tiles_with_their_rows_along_h():
    """The four-wave direct convolution lays its 2 x 8 x 16 tiles with the 16-position rows along H where that takes fewer rounds of
    the chip (W = 24: 1.5 tiles of 16; H = 16: exactly one).  Against the oracle, and against the same problem transposed in
    (H, W) with transposed taps, which runs the ordinary layout (equal up to the order in which the taps are summed)."""
    from ltxmi import ops
    from oracle import vae as ov
    B, T, H, W, cin, cout = 3, 100, 16, 24, 64, 128              # 600 tiles (2 rounds) the ordinary way, 450 (1 round) with rows along H
    x = rnd(B, cin, T, H, W, seed=150)
    w = rnd(cout, cin, 3, 3, 3, seed=151, scale=(27 * cin) ** -0.5)
    b = rnd(cout, seed=152)
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous().to(DEV)
    r = ops.conv3d_route(ndhwc(x).to(DEV), wp, b.to(DEV), True, False, algo=3)
    assert (r["route"], r["epilogue"], r["ksplit"], r["swap_hw"]) == (ops.CONV_DIRECT4, 0, 1, 1), r
    out = ops.conv3d(ndhwc(x).to(DEV), wp, b.to(DEV), True, False, algo=3)
    truth = ov.causal_conv3d(x.float(), {"conv.weight": w.float(), "conv.bias": b.float()}, "", True, "zeros")
    check(ncdhw(out.cpu()), truth, what="tiles with rows along H vs oracle")
    xt, wt = x.transpose(3, 4).contiguous(), w.transpose(3, 4).contiguous()      # H <-> W: 24 x 16, ordinary layout (3 x 1 tiles)
    wpt = wt.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous().to(DEV)
    assert ops.conv3d_route(ndhwc(xt).to(DEV), wpt, b.to(DEV), True, False, algo=3)["swap_hw"] == 0
    out_t = ops.conv3d(ndhwc(xt).to(DEV), wpt, b.to(DEV), True, False, algo=3).transpose(2, 3)
    d = (out_t.float() - out.float()).abs()
    assert bool((d <= out.float().abs() * 2.0 ** -7 + 1e-2).all()), float(d.max())
    assert float((out_t.float() - out.float()).norm() / out.float().norm()) < 1e-3


@pytest.mark.parametrize("cin,residual,red", [(256, True, 2), (128, False, 1)])
@pytest.mark.parametrize("algo", [4, 3])
def test_conv3d_direct_path_depth_to_space(cin, residual, red, algo, monkeypatch):
    """DepthToSpaceUpsample on the direct-convolution path (Cout/8 a multiple of 128), both forms."""
    from ltxmi import autoencoder as ae, ops
    from oracle import vae as ov
    monkeypatch.setattr(ops, "CONV_ALGO", algo)
    blk = ae.DepthToSpaceUpsample(3, cin, (2, 2, 2), residual=residual, out_channels_reduction_factor=red,
                                  spatial_padding_mode="replicate").to(BF)
    sd = {k: v.detach().float() for k, v in blk.state_dict().items()}
    x = rnd(1, cin, 5, 36, 100, seed=120)
    truth = ov.depth_to_space_upsample(x.float(), sd, "", dict(stride=(2, 2, 2), residual=residual, reduction=red),
                                       False, "replicate")
    out = blk.to(DEV)(ndhwc(x).to(DEV), causal=False)
    assert ncdhw(out.cpu()).shape == truth.shape
    check(ncdhw(out.cpu()), truth, what=f"direct d2s {cin} res={residual} red={red}")


# ------------------------------------------------ the widths and sizes the bench times (real 0.9.5+ decoder)
def _crop_bands(T, H, W):
    """Two corner crops of a [T,H,W] grid, (4, 10, 18) positions each, and for each the slice of crop outputs
    whose 3x3x3 receptive field lies inside the crop (the volume's own borders are inside the crop, so the
    reference's padding acts on the crop exactly as on the full tensor)."""
    near = ((slice(0, 4), slice(0, 10), slice(0, 18)), (slice(0, 3), slice(0, 9), slice(0, 17)))
    far = ((slice(T - 4, T), slice(H - 10, H), slice(W - 18, W)), (slice(1, 4), slice(1, 10), slice(1, 18)))
    return near, far


@pytest.mark.parametrize("cin,cout,grid,with_add", [(512, 512, (25, 32, 48), True), (1024, 1024, (13, 16, 24), False),
                                                    (1024, 1024, (4, 16, 64), True)])
@pytest.mark.parametrize("algo", [4, 3])
def test_conv3d_direct_full_width_bands(cin, cout, grid, with_add, algo):
    """The direct convolution at the channel counts of the timed decoder (Cin 512 / 1024: 8 / 16 chunks of 64 input
    channels per tile) on the bench's own stage grids.  The CPU oracle cannot do 10^11..10^12 FLOP in seconds, but a
    convolution is local: two corner crops of the full-size result are compared with the oracle run on the crops."""
    from ltxmi import ops
    from oracle import vae as ov
    T, H, W = grid
    g = torch.Generator(device=DEV).manual_seed(130 + cin)
    x = torch.randn(1, T, H, W, cin, generator=g, device=DEV).to(BF)                    # NDHWC
    w = rnd(cout, cin, 3, 3, 3, seed=131, scale=(27 * cin) ** -0.5)
    b = rnd(cout, seed=132)
    add = torch.randn(1, T, H, W, cout, generator=g, device=DEV).to(BF) if with_add else None
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()
    out = ops.conv3d(x, wp.to(DEV), b.to(DEV), False, True, add=add, algo=algo)          # the direct kernel in that form, or an error
    assert torch.isfinite(out.float()).all()
    for (ct, cy, cx), (vt, vy, vx) in _crop_bands(T, H, W):
        xc = x[:, ct, cy, cx].permute(0, 4, 1, 2, 3).float().cpu()                       # NCDHW crop
        truth = ov.causal_conv3d(xc, {"conv.weight": w.float(), "conv.bias": b.float()}, "", False, "replicate")
        got = out[:, ct, cy, cx].permute(0, 4, 1, 2, 3).float().cpu()
        if with_add:
            truth = truth + add[:, ct, cy, cx].permute(0, 4, 1, 2, 3).float().cpu()
        check(got[:, :, vt, vy, vx], truth[:, :, vt, vy, vx], what=f"direct conv {cin}->{cout} full-size crop")
    # and the two implementations against each other over the WHOLE tensor
    ref = ops.conv3d(x, wp.to(DEV), b.to(DEV), False, True, add=add, algo=1)             # implicit GEMM
    check(out, ref, rel_l2=4e-3, what=f"direct vs implicit GEMM {cin}->{cout}")


def test_conv3d_direct_full_width_depth_to_space_band():
    """DepthToSpaceUpsample 1024 -> 4096 (+ residual) on the bench's first-stage grid 13 x 16 x 24: crop check of the
    direct kernel's scatter epilogue at full width, and the whole tensor against the implicit GEMM."""
    from ltxmi import autoencoder as ae, ops
    from oracle import vae as ov
    cin, (T, H, W) = 1024, (13, 16, 24)
    blk = ae.DepthToSpaceUpsample(3, cin, (2, 2, 2), residual=True, out_channels_reduction_factor=2,
                                  spatial_padding_mode="replicate").to(BF)
    sd = {k: v.detach().float() for k, v in blk.state_dict().items()}
    g = torch.Generator(device=DEV).manual_seed(140)
    x = torch.randn(1, T, H, W, cin, generator=g, device=DEV).to(BF)
    blk = blk.to(DEV)
    out = blk(x, causal=False)                                                           # [1, 2T-1, 2H, 2W, 512]
    assert out.shape == (1, 2 * T - 1, 2 * H, 2 * W, cin // 2) and torch.isfinite(out.float()).all()
    xc = x[:, 0:4, 0:10, 0:18].permute(0, 4, 1, 2, 3).float().cpu()
    truth = ov.depth_to_space_upsample(xc, sd, "", dict(stride=(2, 2, 2), residual=True, reduction=2), False, "replicate")
    got = out[:, 0:5, 0:18, 0:34].permute(0, 4, 1, 2, 3).float().cpu()                   # from input positions [0:3, 0:9, 0:17]
    check(got, truth[:, :, 0:5, 0:18, 0:34], what="direct d2s 1024->4096 full-size crop")
    old = ops.CONV_ALGO
    try:
        ops.CONV_ALGO = 1
        ref = blk(x, causal=False)
    finally:
        ops.CONV_ALGO = old
    check(out, ref, rel_l2=4e-3, what="direct vs implicit GEMM d2s 1024->4096")


@pytest.mark.parametrize("B,H,N,dh", [(1, 32, 13376, 64), (1, 12, 32760, 128)])
def test_attention_config_shapes_properties(B, H, N, dh):
    """Config 3 (N = 13 376, 32 heads of 64) and config 4 (Wan 1.3B: [1, 32760, 12, 128], a ragged last key tile) at
    full size: softmax rows sum to one, the output is linear in V, and a band of query rows matches the oracle."""
    from ltxmi import ops
    g = torch.Generator(device=DEV).manual_seed(150 + dh)
    q = torch.randn(B, N, H, dh, generator=g, device=DEV).to(BF)
    k = torch.randn(B, N, H, dh, generator=g, device=DEV).to(BF)
    v1 = torch.randn(B, N, H, dh, generator=g, device=DEV).to(BF)
    v2 = torch.randn(B, N, H, dh, generator=g, device=DEV).to(BF)
    o = ops.attention(q, k, torch.ones_like(v1)).float()
    assert (o - 1.0).abs().max() < 8e-3
    o1, o2 = ops.attention(q, k, v1).float(), ops.attention(q, k, v2).float()
    o3 = ops.attention(q, k, (0.5 * v1.float() + 0.25 * v2.float()).to(BF)).float()
    lin = 0.5 * o1 + 0.25 * o2
    e_lin = float((o3 - lin).norm() / lin.norm())
    assert e_lin < 4e-3, e_lin                                       # (derivation: test_attention_full_size_properties_98k)
    for rows in (slice(0, 64), slice(N - 70, N)):                    # first tile and the ragged end
        truth = attn_truth(q[:, rows].cpu(), k.cpu(), v1.cpu())
        e = check(o1[:, rows], truth, what=f"attention N{N} dh{dh} rows {rows}")   # the file's REL_L2 / MAXREL
        print(f"attention N{N} dh{dh} rows {rows}: rel L2 {e:.3e}, linearity {e_lin:.3e}")
    # cross-attention of config 4: 512 text keys, no bias
    kc, vc = k[:, :512].contiguous(), v1[:, :512].contiguous()
    oc = ops.attention(q, kc, vc)
    rows = slice(1000, 1256)
    check(oc[:, rows], attn_truth(q[:, rows].cpu(), kc.cpu(), vc.cpu()), what=f"cross Lk 512 at N{N} dh{dh}")


# ------------------------------------------------------------- fused K1: QKV projection -> q_norm + RoPE on load
@pytest.mark.parametrize("M,N,K,cols", [(300, 384, 128, 128), (6144, 4096, 256, 2048), (14976, 6144, 256, 2048)])
def test_gemm_row_sums_of_squares(M, N, K, cols):
    """gemm(..., rowsumsq=): per-(row, 64-column block) sums of squares of the STORED bf16 outputs for the columns
    < cols (tile kernels and the persistent kernel), the output itself unchanged."""
    from ltxmi import ops
    a, w, b = rnd(M, K, seed=160), rnd(N, K, seed=161, scale=K ** -0.5), rnd(N, seed=162)
    ss = torch.full((M, cols // 64 + 1), -7.0, dtype=torch.float32, device=DEV)      # one guard column
    out = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), rowsumsq=ss, rowsumsq_cols=cols)
    plain = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV))
    assert torch.equal(out, plain)
    want = out[:, :cols].float().reshape(M, cols // 64, 64).pow(2).sum(-1)
    torch.testing.assert_close(ss[:, : cols // 64], want, rtol=1e-5, atol=1e-6)
    assert (ss[:, cols // 64] == -7.0).all()                                          # nothing written past the q columns


@pytest.mark.parametrize("B,H,N,per_sample_tables", [(3, 32, 1400, False), (2, 32, 2100, True)])
def test_attention_q_norm_and_rope_on_load(B, H, N, per_sample_tables):
    """The attention kernel finishing q while it loads it (RMSNorm over all heads from the GEMM's partial sums, weight,
    interleaved RoPE) against the two-pass form (rmsnorm_rope_ on q, then attention) and against the oracle."""
    from ltxmi import ops
    from oracle import dit
    dh, D = 64, H * 64
    assert ops.attention_fuses_qnorm(B, H, N, N, dh)
    g = torch.Generator(device=DEV).manual_seed(170)
    qkv = (torch.randn(B * N, 3 * D, generator=g, device=DEV) * 1.7).to(BF)
    wq = (1.0 + 0.1 * torch.randn(D, generator=g, device=DEV)).to(BF)
    wk = (1.0 + 0.1 * torch.randn(D, generator=g, device=DEV)).to(BF)
    rows = B * N if per_sample_tables else N
    ang = torch.rand(rows, D // 2, generator=g, device=DEV) * 6.28
    cos = ang.cos().repeat_interleave(2, dim=-1).to(BF)
    sin = ang.sin().repeat_interleave(2, dim=-1).to(BF)
    ss = qkv[:, :D].float().reshape(B * N, D // 64, 64).pow(2).sum(-1).contiguous()
    ref = qkv.clone()
    ops.rmsnorm_rope_(ref[:, :D], wq, 1e-5, cos, sin, rows)
    ops.rmsnorm_rope_(ref[:, D:2 * D], wk, 1e-5, cos, sin, rows)
    v5 = ref.view(B, N, 3, H, dh)
    two_pass = ops.attention(v5[:, :, 0], v5[:, :, 1], v5[:, :, 2])
    fused_in = qkv.clone()
    fused_in[:, D:2 * D] = ref[:, D:2 * D]                            # k finished by its own pass, q left raw
    f5 = fused_in.view(B, N, 3, H, dh)
    fused = ops.attention(f5[:, :, 0], f5[:, :, 1], f5[:, :, 2], q_norm=(ss, wq, 1e-5), rope=(cos, sin, rows))
    # (two renderings with INDEPENDENT roundings of q since the pipelined kernel scales q by softmax_scale * log2(e) before its
    # one rounding to bf16 -- the two-pass form rounds q, then scales the scores: 4e-3 apart, each within 3e-3 of the oracle,
    # which the band below checks for the fused one)
    check(fused, two_pass.float(), rel_l2=5e-3, maxrel=1.6e-2, what="q finished on load vs two passes")
    # round 3: the row factor finalised by k's pass (one float per row, ltxmi_rmsnorm_rope_rstd_bf16) instead of the partial
    # sums: k comes out bit-identical to its plain pass, the factor matches fp32, and attention matches the partial-sums form
    k_in = qkv.clone()
    rstd = torch.full((B * N,), float("nan"), dtype=torch.float32, device=DEV)
    ops.rmsnorm_rope_(k_in[:, D:2 * D], wk, 1e-5, cos, sin, rows, rstd_of=(ss, D, 1e-5, rstd))
    assert torch.equal(k_in[:, D:2 * D], ref[:, D:2 * D]) and torch.equal(k_in[:, :D], qkv[:, :D])
    want = torch.rsqrt(qkv[:, :D].float().pow(2).mean(-1) + 1e-5)
    assert float(((rstd - want) / want).abs().max()) < 1e-5
    k5 = k_in.view(B, N, 3, H, dh)
    fused_r = ops.attention(k5[:, :, 0], k5[:, :, 1], k5[:, :, 2], q_norm=(rstd, wq, 1e-5), rope=(cos, sin, rows))
    check(fused_r, fused.float(), rel_l2=5e-4, maxrel=8e-3, what="q factor finalised per row vs partial sums")
    check(fused_r, two_pass.float(), rel_l2=5e-3, maxrel=1.6e-2, what="q finished on load (row factor) vs two passes")
    # a band of rows against the oracle (fp32 norm + RoPE + attention on the same bf16 inputs)
    sel = slice(N - 200, N)
    q32 = qkv[:, :D].float().cpu().view(B, N, D)
    qn = q32 * torch.rsqrt(q32.pow(2).mean(-1, keepdim=True) + 1e-5) * wq.float().cpu()
    tab = (cos.float().cpu().view(-1, N, D), sin.float().cpu().view(-1, N, D))
    qr = dit.apply_rotary_emb(qn, tab)
    truth = attn_truth(qr.view(B, N, H, dh)[:, sel], v5[:, :, 1].cpu(), v5[:, :, 2].cpu())
    check(fused[:, sel], truth, what="q finished on load vs oracle")


# (the parameter tuples of test_attention_q_norm_on_load_generic_kernel that must run one particular kernel id)
Q_ON_LOAD_KERNEL_ID = {(1, 128, 128, 256, 1024, False, True): 6}


@pytest.mark.parametrize("B,H,dh,Lq,Lk,bias,rope", [(3, 32, 64, 4992, 256, True, False),     # the DiT's cross-attention
                                                    (2, 4, 64, 300, 77, True, False), (1, 2, 64, 100, 100, False, True),
                                                    (1, 12, 128, 520, 520, False, True), (2, 3, 128, 130, 64, True, False),
                                                    (1, 128, 128, 256, 1024, False, True)])         # the pipelined head_dim-128 kernel
def test_attention_q_norm_on_load_generic_kernel(B, H, dh, Lq, Lk, bias, rope):
    """The same fusion in the kernel that takes everything else (key bias, small shapes, head_dim 128 incl. its
    scale-folded form), and in the pipelined head_dim-128 kernel (id 6): against the two-pass form."""
    from ltxmi import ops
    D = H * dh
    assert ops.attention_fuses_qnorm(B, H, Lq, Lk, dh, bias)
    want_id = Q_ON_LOAD_KERNEL_ID.get((B, H, dh, Lq, Lk, bias, rope))
    if want_id is not None:
        assert ops.attention_kernel_id(B, H, Lq, Lk, dh, bias, D, D) == want_id
    g = torch.Generator(device=DEV).manual_seed(171)
    q = (torch.randn(B * Lq, D, generator=g, device=DEV) * 1.7).to(BF)
    k = torch.randn(B, Lk, H, dh, generator=g, device=DEV).to(BF)
    v = torch.randn(B, Lk, H, dh, generator=g, device=DEV).to(BF)
    wq = (1.0 + 0.1 * torch.randn(D, generator=g, device=DEV)).to(BF)
    kb = None
    if bias:
        kb = torch.zeros(B, Lk, device=DEV)
        kb[:, Lk - Lk // 3:] = -10000.0
    cos = sin = None
    if rope:
        ang = torch.rand(Lq, D // 2, generator=g, device=DEV) * 6.28
        cos = ang.cos().repeat_interleave(2, dim=-1).to(BF)
        sin = ang.sin().repeat_interleave(2, dim=-1).to(BF)
    ss = q.float().reshape(B * Lq, D // 64, 64).pow(2).sum(-1).contiguous()
    if D <= 8192:
        ref = q.clone()
        ops.rmsnorm_rope_(ref, wq, 1e-6, cos, sin, Lq if rope else 0)
    else:
        # rows wider than the row kernel takes (only the D = 16384 case, 128 heads of 128, comes here): the first pass in
        # torch, with that kernel's arithmetic -- fp32 x * rstd * weight, interleaved-pair rotation, ONE rounding to bf16
        x = q.float()
        o = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * wq.float()
        if rope:
            c, s_ = cos.float().repeat(B, 1), sin.float().repeat(B, 1)
            ev, od = o[:, 0::2], o[:, 1::2]
            o = torch.stack((ev * c[:, 0::2] - od * s_[:, 0::2], od * c[:, 1::2] + ev * s_[:, 1::2]), dim=-1).reshape(B * Lq, D)
        ref = o.to(BF)
    two_pass = ops.attention(ref.view(B, Lq, H, dh), k, v, key_bias=kb)
    fused = ops.attention(q.view(B, Lq, H, dh), k, v, key_bias=kb, q_norm=(ss, wq, 1e-6),
                          rope=(cos, sin, Lq) if rope else None)
    check(fused, two_pass.float(), rel_l2=2e-3, maxrel=1.6e-2, what="q finished on load (generic kernel) vs two passes")
    # the row factor as ONE float per row from its own launch (ltxmi_rowsumsq_rstd_f32; cross-attention's q): the factor
    # against fp32, attention against the partial-sums form
    rstd = ops.rowsumsq_rstd(ss, D, 1e-6)
    want = torch.rsqrt(q.float().pow(2).mean(-1) + 1e-6)
    assert float(((rstd - want) / want).abs().max()) < 1e-5
    fused_r = ops.attention(q.view(B, Lq, H, dh), k, v, key_bias=kb, q_norm=(rstd, wq, 1e-6),
                            rope=(cos, sin, Lq) if rope else None)
    check(fused_r, fused.float(), rel_l2=5e-4, maxrel=8e-3, what="row factor vs partial sums (generic kernel)")


# ------------------------------------------------ kernels of the zero-copy Ulysses exchange, on ONE device
# (the collectives themselves run in tests/test_distributed.py; here the layouts they carry are emulated locally)
@pytest.mark.parametrize("B,Nl,H,P,per_sample", [(3, 624, 32, 8, False), (2, 100, 4, 2, True), (1, 33, 2, 1, False)])
def test_qkv_norm_rope_pack(B, Nl, H, P, per_sample):
    """q/k RMSNorm + RoPE + v, written destination-major [P][Nl][B][3][D/P]: against the two in-place passes
    (rmsnorm_rope_, oracle-checked above) followed by the permutation the kernel fuses."""
    from ltxmi import ops
    D = H * 64
    g = torch.Generator(device=DEV).manual_seed(180)
    qkv = (torch.randn(B * Nl, 3 * D, generator=g, device=DEV) * 1.3).to(BF)
    wq = (1.0 + 0.1 * torch.randn(D, generator=g, device=DEV)).to(BF)
    wk = (1.0 + 0.1 * torch.randn(D, generator=g, device=DEV)).to(BF)
    rows = B * Nl if per_sample else Nl
    ang = torch.rand(rows, D // 2, generator=g, device=DEV) * 6.28
    cos, sin = ang.cos().repeat_interleave(2, -1).to(BF), ang.sin().repeat_interleave(2, -1).to(BF)
    out = ops.qkv_norm_rope_pack(qkv, B, Nl, D, P, wq, wk, 1e-5, cos, sin, rows)
    ref = qkv.clone()
    ops.rmsnorm_rope_(ref[:, :D], wq, 1e-5, cos, sin, rows)
    ops.rmsnorm_rope_(ref[:, D:2 * D], wk, 1e-5, cos, sin, rows)
    want = ref.view(B, Nl, 3, P, D // P).permute(3, 1, 0, 2, 4).contiguous()
    assert out.shape == want.shape == (P, Nl, B, 3, D // P)
    assert torch.equal(out[:, :, :, 2], want[:, :, :, 2])                       # v: a copy
    # q, k: the same arithmetic in another kernel (the compiler may contract the multiply-adds differently): equal up
    # to a last-bit rounding flip on a few elements
    check(out, want.float(), rel_l2=1e-3, maxrel=8e-3, what="qkv_norm_rope_pack vs two passes + permute")
    assert (out != want).float().mean() < 0.02


@pytest.mark.parametrize("B,H,N,P", [(3, 4, 4992, 8), (2, 32, 2048, 2), (2, 2, 200, 4)])
def test_attention_reads_token_major_and_writes_segmented(B, H, N, P):
    """The attention kernel on the layouts of the zero-copy Ulysses exchange: q/k/v as token-major views of
    [N][B][3][H][dh] (the all-to-all's receive buffer) and the output written into [P][B][N/P][H dh] (the return
    exchange's send buffer, a segmented token axis) -- against the plain layouts."""
    from ltxmi import ops
    dh, Nl = 64, N // P
    g = torch.Generator(device=DEV).manual_seed(190)
    full = torch.randn(N, B, 3, H, dh, generator=g, device=DEV).to(BF)
    q, k, v = (full[:, :, i].permute(1, 0, 2, 3) for i in range(3))             # [B, N, H, dh] views
    want = ops.attention(q.contiguous(), k.contiguous(), v.contiguous())
    osend = torch.full((P, B, Nl, H, dh), float("nan"), device=DEV, dtype=BF)
    ops.attention(q, k, v, out=osend[0], out_segments=(Nl, B * Nl * H * dh))
    got = osend.permute(1, 0, 2, 3, 4).reshape(B, N, H, dh)
    assert torch.equal(got, want)


@pytest.mark.parametrize("M,N,K,P,epi", [(1872, 2048, 2048, 8, "gate"), (5000, 384, 512, 2, "none"), (300, 256, 256, 4, "none"),
                                         (5000, 2048, 2048, 8, "gate")])
def test_gemm_k_blocked_operand(M, N, K, P, epi):
    """A = the return all-to-all's receive buffer [P][M][K/P], consumed in place (K-blocked), with the gate + residual
    epilogue of to_out.  The first three shapes have 64, 40 and 2 tiles of 256x256 and run the 128x128 kernel; the last
    (20 x 8 tiles) runs the persistent kernel, as to_out does in the product."""
    from ltxmi import ops
    want_id = 2 if M == 5000 and N == 2048 else 0
    g = torch.Generator(device=DEV).manual_seed(200)
    a = (torch.randn(M, K, generator=g, device=DEV) * 0.5).to(BF)
    w = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(BF)
    b = torch.randn(N, generator=g, device=DEV).to(BF)
    blocked = a.view(M, P, K // P).permute(1, 0, 2).contiguous()                 # [P, M, K/P]
    kw = {}
    if epi == "gate":
        res = torch.randn(M, N, generator=g, device=DEV).to(BF)
        # (three groups exactly: the kernels do not clamp the group index, so rows_per_group rounds UP -- 624 and 1667)
        kw = dict(epilogue=ops.EPI_GATE_RESIDUAL, gate_table=torch.randn(N, generator=g, device=DEV).to(BF),
                  gate_temb=torch.randn(3, N, generator=g, device=DEV).to(BF), rows_per_group=(M + 2) // 3)
        assert ops.gemm_kernel_id(a, w, b, residual=res, out=torch.empty_like(res), **kw) == want_id
        assert ops.gemm_kernel_id(blocked[0], w, b, residual=res, out=torch.empty_like(res), a_kblock=K // P,
                                  a_kblock_stride=M * (K // P), **kw) == want_id
        want = ops.gemm(a, w, b, residual=res.clone(), out=torch.empty_like(res), **kw)
        got = ops.gemm(blocked[0], w, b, residual=res.clone(), out=torch.empty_like(res), a_kblock=K // P,
                       a_kblock_stride=M * (K // P), **kw)
    else:
        assert ops.gemm_kernel_id(a, w, b) == want_id
        assert ops.gemm_kernel_id(blocked[0], w, b, a_kblock=K // P, a_kblock_stride=M * (K // P)) == want_id
        want = ops.gemm(a, w, b)
        got = ops.gemm(blocked[0], w, b, a_kblock=K // P, a_kblock_stride=M * (K // P))
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("dim,extent", [(2, 16), (3, 128), (4, 96), (2, 500)])
def test_tile_blend(dtype, dim, extent):
    """blend_z / blend_v / blend_h (vae.py:193-221) in one kernel, in place in b: against the reference's formula slice by
    slice (fp32 arithmetic, one rounding), for the three dtypes tiles have on the tiled paths; an extent larger than a
    tensor is clipped as in the reference."""
    from ltxmi import ops
    g = torch.Generator().manual_seed(210)
    shape_a = [1, 3, 40, 160, 192]
    shape_b = list(shape_a)
    shape_b[dim] -= 7                                   # the two tiles may differ along the blended axis only
    a = torch.randn(*shape_a, generator=g).to(dtype)
    b = torch.randn(*shape_b, generator=g).to(dtype)
    e = min(a.shape[dim], b.shape[dim], extent)
    want = b.clone().float()
    for z in range(e):
        ia = [slice(None)] * 5
        ib = [slice(None)] * 5
        ia[dim] = a.shape[dim] - e + z
        ib[dim] = z
        want[tuple(ib)] = a[tuple(ia)].float() * (1 - z / e) + b[tuple(ib)].float() * (z / e)
    bd = b.to(DEV)
    out = ops.tile_blend_(a.to(DEV), bd, extent, dim)
    assert out.data_ptr() == bd.data_ptr()
    tol = dict(rtol=0, atol=0) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(out.float().cpu(), want.to(dtype).float(), **(dict(rtol=1e-6, atol=1e-6) if dtype == torch.float32 else tol))
    untouched = [slice(None)] * 5
    untouched[dim] = slice(e, None)
    assert torch.equal(out.cpu()[tuple(untouched)], b[tuple(untouched)])


def test_gemm_ignores_rowsumsq_fields_without_a_pointer():
    """a C caller that leaves rowsumsq_cols / rowsumsq_ld unset (garbage) next to a NULL rowsumsq pointer must
    get the plain GEMM -- the plain epilogue runs on the row-sums kernel instance, whose extra stores used to take their
    geometry from those fields."""
    import ctypes
    from ltxmi import _lib, ops
    # the 128x128 tile kernel (8 x 2 tiles of 256x256) and the persistent 256x256 one (32 x 16 tiles, floor 128)
    for (M, N, K, kernel) in ((2048, 512, 256, 0), (8192, 4096, 128, 2)):
        a, w = rnd(M, K, seed=41).to(DEV), rnd(N, K, seed=42, scale=K ** -0.5).to(DEV)
        guard = torch.full((M * N + 4096,), 7.0, dtype=BF, device=DEV)
        out = guard[:M * N].view(M, N)
        args = _lib.GemmArgs()
        args.A, args.lda, args.W, args.ldw = a.data_ptr(), K, w.data_ptr(), K
        args.C, args.ldc, args.M, args.N, args.K = out.data_ptr(), N, M, N, K
        args.rows_per_group = 1
        args.rowsumsq, args.rowsumsq_cols, args.rowsumsq_ld = None, 0x7fffff00, -12345
        assert _lib.lib.ltxmi_gemm_kernel_id(ctypes.byref(args)) == kernel
        _lib.check(_lib.lib.ltxmi_gemm_bf16(ctypes.byref(args), ops._stream()), "ltxmi_gemm_bf16")
        torch.cuda.synchronize()
        check(out, a.float().cpu() @ w.float().cpu().T, what=f"gemm {M}x{N}x{K} with garbage rowsumsq fields")
        assert (guard[M * N:] == 7.0).all()


def test_stg_blend_grouped_matches_per_group_blends():
    """The one-launch STG blend over the K-blocked layout [P][B, Nl][D/P] of the Ulysses return exchange against P
    launches of the plain blend (attention.py:1127-1141 arithmetic)."""
    from ltxmi import ops
    P, B, Nl, Dp = 4, 3, 37, 128
    D = P * Dp
    a = rnd(P, B, Nl, Dp, seed=51).to(DEV)
    qkv = rnd(B, Nl, 3 * D, seed=52).to(DEV)
    m = torch.tensor([1.0, 1.0, 0.0], device=DEV)
    want = a.clone()
    for p in range(P):
        ops.stg_blend_(want[p], qkv[:, :, 2 * D + p * Dp: 2 * D + (p + 1) * Dp], m)
    got = ops.stg_blend_grouped_(a.clone(), qkv[:, :, 2 * D:], m)
    assert torch.equal(got, want)
    assert torch.equal(got[:, :2], a[:, :2]) and not torch.equal(got[:, 2], a[:, 2])
