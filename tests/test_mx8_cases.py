"""tests/mx8_cases.py pinned on the CPU: the exponent rule and the element rounding of the restated MX-FP8 quantiser against
values written out by hand, the two readings of the rule (bf16 bits / frexp) against each other, the measured GEMM slack, and
the condition on the cases -- the fp32 restatement alone meets every metric the GPU file applies -- and the exact witnesses:
the probe's variants (the default one unchanged, the flat outputs, the wide byte ranges, the strided views and their sentinels),
the tile counts of the probe shapes and the tile walk as a bijection, the exactness condition of every exact epilogue case, the
threshold witness against the literals of its table, and the output guards."""
import pytest
import torch

import gemm_cases as gc
import mx8_cases as mc

BF, F64 = torch.bfloat16, torch.float64


def _block(amax, fill=0.0):
    x = torch.full((1, 32), fill, dtype=F64)
    x[0, 3] = amax
    return x.to(BF)


@pytest.mark.parametrize("amax,e,elem", mc.WITNESSES, ids=lambda v: f"{v:g}")
def test_exponent_rule_witnesses(amax, e, elem):
    x = _block(amax)
    q, s = mc.quantize(x)
    assert int(s[0, 0]) == (0 if amax == 0 else e + 127)
    assert float(q[0, 3].float()) == elem
    # the smallest e with amax * 2^-e <= 448, unless the clamp holds it
    a = float(x[0, 3].to(F64))
    if a > 0 and -127 < e < 127:
        assert a * 2.0 ** -e <= 448 < a * 2.0 ** -(e - 1)
    # -amax gives the same byte and the negated element
    q2, s2 = mc.quantize(-x)
    assert int(s2[0, 0]) == int(s[0, 0]) and float(q2[0, 3].float()) == -elem


def test_rule_names_the_issue_spells_out():
    w = {a: (e, q) for a, e, q in mc.WITNESSES}
    assert w[448.0] == (0, 448.0) and w[450.0] == (1, 224.0) and w[1.0] == (-8, 256.0) and w[0.0][1] == 0.0
    assert w[3e38][0] == 120 and w[2.0 ** -130][0] == -127            # 3e38 and a bf16 subnormal


def test_no_block_saturates_and_the_two_readings_agree():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(64, 256, generator=g) * 10.0 ** (torch.rand(64, 1, generator=g) * 70 - 35)).to(BF)
    x[5] = 0
    x[6, :32] = torch.tensor(2.0 ** -131).to(BF)
    q, s = mc.quantize(x)
    assert torch.equal(s, mc.scale_bytes_real(x))
    qa = q.float().abs().reshape(64, 8, 32).amax(dim=-1)
    assert float(qa.max()) <= 448 and bool(((qa >= 224) | (s == 0)).all())       # the block's amax lands in [224, 448] (byte 0: clamped)
    assert bool((s[5] == 0).all()) and bool((q[5].view(torch.uint8) == 0).all())
    # de-quantised, a block is within half an e4m3 ulp of its amax of the input
    err = (mc.dequantize(q, s) - x.to(F64)).abs().reshape(64, 8, 32)
    amax = x.to(F64).abs().reshape(64, 8, 32).amax(dim=-1, keepdim=True)
    assert bool((err <= amax * 2.0 ** -4 + 2.0 ** -136).all())


def test_element_rounding_ties_and_subnormals():
    """amax 256 -> e = 0, the elements are RNE(x): e4m3 spacing 2^-9 below 2^-6 (subnormals), 2 in [16, 32), 16 in [128, 256)."""
    vals = [2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -9, 2.0 ** -10 * 0.99, 2.0 ** -10 * 1.01, 17.0, 19.0, 21.0, 1.0625, 1.1875,
            240.0, 232.0, 248.0, 0.4375, 2.0 ** -6 - 2.0 ** -10]
    want = [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 0.0, 2.0 ** -9, 16.0, 20.0, 20.0, 1.0, 1.25,
            240.0, 224.0, 256.0, 0.4375, 2.0 ** -6]
    x = torch.zeros(1, 32, dtype=F64)
    x[0, :len(vals)] = torch.tensor(vals, dtype=F64)
    x[0, 31] = 256.0
    for sign in (1.0, -1.0):
        xb = (sign * x).to(BF)
        q, s = mc.quantize(xb)
        assert int(s[0, 0]) == 127
        assert q[0, :len(vals)].float().tolist() == [sign * w for w in want]
    q, _ = mc.quantize((-x).to(BF))
    assert int(q.view(torch.uint8)[0, 0]) == 0x80                     # -2^-10 rounds to -0


def test_witness_rows_carry_their_amax():
    x = mc.witness_rows(64)
    _, s = mc.quantize(x)
    for i, (amax, e, _) in enumerate(mc.WITNESSES):
        assert s[i].tolist() == [0 if amax == 0 else e + 127] * 2, (i, amax)
    assert s[-1].tolist() == [127, 127] and s[-2].tolist() == [127, 127]


def test_probe_is_exact_and_asymmetric():
    for one_hot in ("a", "w"):
        aq, a_s, wq, w_s, want = mc.probe(70, 96, 128, one_hot)
        assert not torch.equal(want[:64, :64], want[:64, :64].T)
        assert len(set(a_s[3].tolist())) == 4 and len(set(w_s[:, 1].tolist())) == 11       # a scale of its own per block and row
        assert float((want.float() != 0).float().mean()) > 0.9


def test_slack_is_measured():
    got = mc.measure_excess()
    print("measured excess:", {k: f"{v:.3e}" for k, v in got.items()})
    for epi, v in got.items():
        assert v <= mc.MEASURED_EXCESS_BY_EPI[epi] * 1.001, (epi, v)
        assert v >= mc.MEASURED_EXCESS_BY_EPI[epi] * 0.5, (epi, v)                          # the pin is the measurement, not a roomy bound
    assert mc.SLACK == 4.0 * max(mc.MEASURED_EXCESS_BY_EPI.values())


@pytest.mark.parametrize("case", mc.SLACK_CASES, ids=lambda c: f"{c[0]}-{c[1]}-K{c[2]}")
def test_restatement_alone_meets_every_metric(case):
    family, epi, K = case
    M, N = mc.SLACK_MN
    d = mc.make(family, M, N, K, epi)
    acc, mag = mc.product(d)
    t, m = mc.epilogue_op(d, epi, acc, mag)
    gc.compare(mc.restate(d, epi), t, m, what=f"restate {family} {epi} K={K}", slack=mc.SLACK)
    if epi in mc.MX_EPIS:
        # the MX-output form: the restated quantiser on the fp32 restatement's values
        v = mc.epilogue_op(d, epi, *mc.product(d, torch.float32))[0]
        s = mc.scale_bytes_real(v)
        f = mc.mx_out_figures(mc.quantize_elements(v, s), s, t, m)
        assert f["scale_bad"] == 0 and f["elem"] <= 1.0, f


def test_case_tables():
    edges = {mc.EDGE_1, mc.EDGE_NARROW}
    assert {c["shape"] for c in mc.GEMM_CASES} == {mc.SMALL, mc.BIG, (1, 288, 256), (1, 4096, 8192), (300, 288, 128)} | edges
    assert {(c["family"], c["epi"]) for c in mc.GEMM_CASES if c["shape"] in (mc.SMALL, mc.BIG)} == \
        {(f, e) for f in mc.FAMILIES for e in mc.EPIS}
    for c in mc.GEMM_CASES + mc.MXOUT_CASES:
        assert c["shape"][1] % 32 == 0 and c["shape"][2] % 128 == 0
    # the new edges: plain under every epilogue of both output forms, and cancel + gate at one K-tile
    assert edges == {(257, 32, 128), (300, 2336, 128)}
    for s in edges:
        assert {(c["family"], c["epi"]) for c in mc.GEMM_CASES if c["shape"] == s} == {("plain", e) for e in mc.EPIS}
        assert {(c["family"], c["epi"]) for c in mc.MXOUT_CASES if c["shape"] == s} == {("plain", e) for e in mc.MX_EPIS}
    assert [(c["family"], c["epi"]) for c in mc.GEMM_CASES if c["shape"] == (300, 288, 128)] == [("cancel", "gate")]
    assert {k for _, _, k in mc.SLACK_CASES} == {128, 256, 8192}


# ------------------------------------------------------------------------------------------------- the exact witnesses
def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == mc.E4M3 else t.contiguous()


def _digest(tensors):
    import hashlib
    return hashlib.sha256(b"".join(_bits(t).view(torch.uint8).numpy().tobytes() for t in tensors)).hexdigest()[:16]


@pytest.mark.parametrize("shape,one_hot,digest", [((70, 96, 128), "a", "2bd137d660f0e3a6"), ((70, 96, 128), "w", "e5b763f61dd5fc1e"),
                                                  ((300, 288, 256), "a", "2b9b6382ab715fbb"), ((300, 288, 256), "w", "1c24333de845fc73"),
                                                  ((520, 544, 384), "a", "045ca8d1337a571c"), ((520, 544, 384), "w", "18be288a83ca54cd")])
def test_default_probe_is_what_it_was(shape, one_hot, digest):
    """The digests are those of probe() before it took ``scales`` and ``geometry``."""
    got = mc.probe(*shape, one_hot)
    assert _digest(got) == digest
    assert [t.dtype for t in got] == [mc.E4M3, torch.uint8, mc.E4M3, torch.uint8, BF] and all(t.is_contiguous() for t in got)
    assert _digest(mc.probe(*shape, one_hot, scales="varied", geometry="contiguous")) == digest


def _tiles(shape):
    M, N, K = shape
    return -(-M // 256), -(-N // 256), K // 128


def test_probe_shapes_reach_what_their_comments_say():
    assert [_tiles(s) for s in mc.WALK_SHAPES] == [(1, 1, 1), (2, 1, 1), (2, 10, 1), (3, 12, 1)]
    assert mc.WALK_SHAPES == [(256, 256, 128), (257, 32, 128), (300, 2336, 128), (520, 2848, 128)]
    assert 10 - 8 == 2 and 2336 - 9 * 256 == 32 and 12 - 8 == 4 and 257 - 256 == 1 and 256 - 32 == 224
    assert [_tiles(s) for s in mc.KTILE_SHAPES] == [(2, 2, t) for t in (1, 4, 5, 7)]
    assert mc.TRUTH_KTILES == [1, 2, 3, 4, 5, 7] and set(mc.WALK_SHAPES + mc.KTILE_SHAPES) <= set(mc.PROBE_SHAPES)
    assert mc.PROBE_SHAPES[:2] == [mc.SMALL, (520, 544, 384)]
    assert [(v["shape"], v["scales"], v["geometry"]) for v in mc.PROBE_VARIANTS] == [
        ((300, 288, 512), "wide", "contiguous"), ((257, 32, 512), "wide", "contiguous"),
        ((300, 288, 384), "varied", "strided"), ((300, 2336, 128), "varied", "strided")]
    for s in mc.PROBE_SHAPES + [v["shape"] for v in mc.PROBE_VARIANTS]:
        assert s[1] % 32 == 0 and s[2] % 128 == 0 and s[2] <= 896


def _tile_walk(tiles_m, tiles_n):
    """The kernel's walk restated: workgroup id -> xcd_work_id -> (tm, tn) in bands of 8 N-tiles."""
    nwg = tiles_m * tiles_n
    q, r = nwg >> 3, nwg & 7
    out = []
    for orig in range(nwg):
        xcd = orig & 7
        tile = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (orig >> 3)
        band, rem = divmod(tile, tiles_m * 8)
        gn = min(8, tiles_n - band * 8)
        out.append((rem // gn, band * 8 + rem % gn))
    return out


def test_tile_walk_is_a_bijection():
    for tm in range(1, 12):
        for tn in range(1, 40):
            assert sorted(_tile_walk(tm, tn)) == [(i, j) for i in range(tm) for j in range(tn)], (tm, tn)
    # and with gn = 8 unconditionally the narrow band of the 2 x 10 grid is not covered: the shape can tell the two apart
    band1 = [(rem // 8, 8 + rem % 8) for rem in range(2 * 2)]
    assert sorted(band1) != [(i, j) for i in range(2) for j in (8, 9)]


@pytest.mark.parametrize("one_hot", ["a", "w"])
def test_flat_probe(one_hot):
    aq, a_s, wq, w_s, want = mc.probe(300, 288, 128, one_hot, scales="flat")
    assert bool((a_s == 127).all()) and bool((w_s == 127).all())
    v = want.to(F64)
    assert bool((v == v.round()).all()) and float(v.min()) == -7 and float(v.max()) == 7
    # the operands are those of the default probe: only the scales differ
    ref = mc.probe(300, 288, 128, one_hot)
    assert torch.equal(_bits(aq), _bits(ref[0])) and torch.equal(_bits(wq), _bits(ref[2]))


@pytest.mark.parametrize("v", [v for v in mc.PROBE_VARIANTS if v["scales"] == "wide"], ids=lambda v: "x".join(map(str, v["shape"])))
@pytest.mark.parametrize("one_hot", ["a", "w"])
def test_wide_probe(v, one_hot):
    M, N, K = v["shape"]
    assert K // 128 >= 4
    aq, a_s, wq, w_s, want = mc.probe(M, N, K, one_hot, scales="wide")
    for s in (a_s, w_s):
        assert int(s.min()) == 1 and int(s.max()) == 253 and not bool((s == 255).any())
        assert all(len(set(row.tolist())) == K // 32 for row in s[:7])                       # a byte of its own in every block
        assert int((s[0].to(torch.int32).max() - s[0].to(torch.int32).min())) >= 240         # one row alone spans the range
    e = (a_s.to(torch.int32)[:, None, :] - 127) + (w_s.to(torch.int32)[None, :, :] - 127)    # [M, N, blocks]
    assert int(e.abs().max()) <= 12 and int(e.min()) < 0 < int(e.max())
    t = want.to(F64)
    assert torch.equal(t, mc.dequantize(aq, a_s) @ mc.dequantize(wq, w_s).T)                  # representable in bf16, exactly
    nz = t[t != 0].abs()
    assert float(nz.min()) >= 2.0 ** -126 and float(nz.max()) <= 7 * 2.0 ** 12 and nz.numel() > 0.9 * t.numel()


@pytest.mark.parametrize("v", [v for v in mc.PROBE_VARIANTS if v["geometry"] == "strided"], ids=lambda v: "x".join(map(str, v["shape"])))
def test_strided_probe(v):
    M, N, K = v["shape"]
    ref = mc.probe(M, N, K, "a")
    got = mc.probe(M, N, K, "a", geometry="strided")
    assert all(torch.equal(_bits(g), _bits(r)) and g.dtype == r.dtype for g, r in zip(got, ref))
    aq, a_s, wq, w_s, _ = got
    assert aq.stride() == (K + 16, 1) and a_s.stride() == (K // 32 + 4, 1) and a_s.storage_offset() == 4
    assert wq.stride() == (K, 1) and wq.storage_offset() == 5 * K and w_s.stride() == (K // 32, 1) and w_s.storage_offset() == 5 * K // 32
    views, bufs = mc.strided_operands(*ref[:4])
    assert bufs[2].shape == (N + 9, K) and bufs[3].shape == (N + 9, K // 32)
    for view, buf, fill in zip(views, bufs, (0x7f, 0xff, 0x7f, 0xff)):
        inside = torch.zeros(buf.numel(), dtype=torch.bool)
        torch.as_strided(inside, view.shape, view.stride(), view.storage_offset()).fill_(True)
        flat = buf.reshape(-1)
        assert bool((flat[~inside] == fill).all()) and int((~inside).sum()) > 0
        assert torch.equal(flat[inside].reshape(view.shape), _bits(view).view(torch.uint8))
        # the pattern is no value of the operand: a NaN in either format
        assert not bool((_bits(view).view(torch.uint8) & (0x7f if fill == 0x7f else 0xff) == fill).any())


@pytest.mark.parametrize("c", mc.EXACT_CASES, ids=mc.exact_id)
def test_exact_cases_are_exact(c):
    d = mc.exact(c)
    assert mc.exact_ok(d, c["out"])
    M, N, K = c["shape"]
    assert (d["bias"] is not None) == c["bias"] and d["truth"].shape == (M, N)
    if c["bias"]:
        assert int(d["bias"].min()) == -8 and int(d["bias"].max()) == 8
    if c["epi"] in ("gate", "residual"):
        assert int(d["residual"].min()) == -32 and int(d["residual"].max()) == 32
    if c["epi"] == "gate":
        gate = gc.gate_rows(d, M, F64)
        assert set(gate.unique().tolist()) == set(mc.GATE_SUMS) == {0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0}
        assert d["temb_full"].shape == ((M + c["rpg"] - 1) // c["rpg"], 6 * N) and d["gate_temb"].stride() == (6 * N, 1)
        assert d["gate_temb"].data_ptr() == d["temb_full"].data_ptr() + 2 * N * 2
    if c["out"] == "mx":
        assert float(d["truth"].abs().max()) == (15 if c["bias"] else 7)
    # the arithmetic by hand for one element, in Python floats
    r, n = M - 1, N - 3
    v = float(d["partials"][0][r, n]) + (float(d["bias"][n]) if c["bias"] else 0.0)
    if c["epi"] == "gate":
        v *= float(d["gate_table"][n]) + float(d["gate_temb"][r // c["rpg"], n])
    if c["epi"] in ("gate", "residual"):
        v += float(d["residual"][r, n])
    assert v == float(d["truth"][r, n])


def test_exact_case_table():
    for s in (mc.EDGE_NARROW, mc.EDGE_1):
        cs = [c for c in mc.EXACT_CASES if c["shape"] == s]
        key = lambda c: (c["epi"], c["bias"], c["out"])
        assert {key(c) for c in cs} == {("none", True, "bf16"), ("none", False, "bf16"), ("residual", True, "bf16"),
                                        ("residual", False, "bf16"), ("gate", True, "bf16"), ("gate", False, "bf16"),
                                        ("none", True, "mx"), ("none", False, "mx")}
        assert {c["in_place"] for c in cs if c["epi"] == "residual"} == {True, False}
        assert {c["rpg"] for c in cs if c["epi"] == "gate"} == {1, 7, s[0] + 3} and s[0] % 7
    k640 = [c for c in mc.EXACT_CASES if c["shape"][2] == 640]
    assert sorted((c["epi"], c["out"]) for c in k640) == [("gate", "bf16"), ("none", "bf16"), ("none", "mx"), ("residual", "bf16")]
    assert len({mc.exact_id(c) for c in mc.EXACT_CASES}) == len(mc.EXACT_CASES)


# value, scale byte, element: the fp32 rule at its threshold, as the issue of these tests tabulates it
THRESHOLD_TABLE = [(448.0, 127, 448.0), (448.5, 128, 224.0), (447.5, 127, 448.0), (1.75, 119, 448.0), (1.75 + 2.0 ** -7, 120, 224.0),
                   (0.0, 0, 0.0)]


def test_threshold_witness_literals():
    w = mc.witness_mx_out_threshold()
    assert w["values"].tolist() == [v for v, _, _ in THRESHOLD_TABLE]
    assert w["scales"].tolist() == [[b] for _, b, _ in THRESHOLD_TABLE]
    assert bool((w["q"].to(F64) == torch.tensor([e for _, _, e in THRESHOLD_TABLE], dtype=F64)[:, None]).all())
    assert int(w["q"].view(torch.uint8)[5, 0]) == 0x00 and bool((w["q"].view(torch.uint8)[5] == 0).all())
    # K = 128, N = 32, every input scale 2^0; the big product at k = 0, the addend at k = 8 (another group of 8)
    assert w["aq"].shape == (6, 128) and w["wq"].shape == (32, 128) and bool((w["a_scales"] == 127).all()) and bool((w["w_scales"] == 127).all())
    a, wt = w["aq"].to(F64), w["wq"].to(F64)
    assert sorted(set(a.nonzero()[:, 1].tolist())) == [0, 8] and sorted(set(wt.nonzero()[:, 1].tolist())) == [0, 8]
    assert torch.equal((a @ wt.T), w["values"][:, None].expand(6, 32))
    # the residual cancels the large term exactly and leaves a bf16 value
    assert w["after"].tolist() == [0.0, 0.5, -0.5, 0.0, 2.0 ** -7, 0.0]
    assert torch.equal(w["residual"].to(F64), -(a[:, :1] * wt[:1, 0]).expand(6, 32))
    # every value is an fp32 number, and its mantissa sits where the table says relative to 0x600000
    bits = w["values"].to(torch.float32).view(torch.int32) & 0x7fffff
    assert w["values"].to(torch.float32).to(F64).tolist() == w["values"].tolist()
    assert [int(b) - 0x600000 for b in bits[:5]] == [0, 0x4000, -0x4000, 0, 0x10000]            # 0.5 / 256 = 2^-9, 2^-7
    # a rule switching on >= would give other bytes for the rows that sit exactly on the threshold
    assert [b + 1 for v, b, _ in THRESHOLD_TABLE if v in (448.0, 1.75)] == [128, 120]


def test_guards_hold_no_legal_value():
    for kind, (bits, pattern, dtype) in mc.GUARDS.items():
        buf, view = mc.guarded(5, 8, 4, kind, "cpu")
        assert view.dtype == dtype and view.shape == (5, 8) and view.stride() == (12, 1) and buf.numel() == 7 * 12
        assert mc.guard_figures(buf, view, kind) == (40, 0)
        if dtype.is_floating_point:
            assert bool(torch.isnan(view).all())
        view[:] = 1
        assert mc.guard_figures(buf, view, kind) == (0, 0)
        buf[3] = 0
        assert mc.guard_figures(buf, view, kind) == (0, 1)
    assert bool(torch.isnan(torch.tensor([0x7f], dtype=torch.uint8).view(mc.E4M3).float()).all())      # e4m3fn: S.1111.111
    assert mc.GUARDS["scale"][1] == 0xff                                                               # E8M0: 0xff is NaN
