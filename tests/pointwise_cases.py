"""Inputs, float64 truths and metrics for the pointwise, layout and step-math kernels -- TEST INFRASTRUCTURE ONLY (plain
module, no GPU).  Shared by tests/test_pointwise_cases.py (CPU) and tests/test_gpu_pointwise_kernels.py (MI355X).

Kernels: csrc/pointwise.hip (silu, add, stg_blend, the four layout passes, space_to_depth_skip, the guidance + Euler step,
image_cond_noise) and the tail of csrc/upsampler.hip (pixel_shuffle2d, tile_blend, adain_filter).

INPUT FAMILIES (``make``): seeded, rounded to bf16 before anything is computed from them (fp32 kernels get those values).
  plain       randn * 2
  offset      randn * 0.5 + 4
  tiny        randn * 1e-4
  large       randn * 1e4   (for silu: values below -90, where exp of the negated input overflows; the result is -0)
  row_scales  row r multiplied by 10 ** u_r, u_r uniform in [-3, 3]
No NaN and no infinity.

OPERATIONS.  Every ``*_op`` is the reference's formula in plain torch (taken from oracle/ where it has one: the module
named at each function), generic over the dtype it is run in: in float64 it is the truth, in float32 followed by ONE
rounding to the output dtype (``restate``) it is what a correct fp32 kernel gives.  Each returns (value, mag); ``mag`` is,
per element, the sum of the magnitudes of the terms that can cancel in front of the rounding:
  silu            |silu(x)|                              add        |a| + |b|
  stg_blend       |a| |m| + |v| |1 - m|                  tile_blend |a| (1 - w) + |b| w
  un-normalise    |v| std + |mean|                       normalise  (|v| + |mean|) / std
  space_to_depth  |conv| + mean_j |x_j|
  guidance step   |lat| + dt factor (|u| (1 + |gs|) |alpha| + |t| (|gs| + |stg| + 1) + |ptb| |stg|)
  cond_noise      |init| + |noise_scale noise t^2|
  adain           |x| + |f| ((|x| + |mean_x|) sd_r / sd_x + |mean_r| + |x|)
The guidance inputs are what one model gives for three prompts of one sample: uncond and perturbed are text plus 0.3 of
its spread of independent noise, so alpha (the projection of text on uncond) is of order 1, as in the product.

METRICS.  Pure copies (layout kernels without std / mean, pixel_shuffle2d, padded channels, everything an in-place kernel
must leave alone) are compared with ``torch.equal`` by the callers.  Arithmetic kernels must meet two checks (``compare``):
  1. ``check`` of tests/test_gpu_kernels.py on the whole tensor (REL_L2 3e-3, MAXREL 1.6e-2; imported, not copied), for
     tensors of at least 64 values as for the rows of tests/norm_cases.py: one bf16 rounding is up to 2^-8 = 3.9e-3
     relative and REL_L2 counts on the average over many (the fp32 restatement of the guidance step at n = 2 is at
     3.04e-3), so the sizes 2 and 8 are held by the per-element bound alone, which is the tighter one per element;
  2. per element |out - truth| <= 2^-7 |truth| + SLACK mag for bf16 outputs, SLACK mag alone for fp32 outputs.  Elements
     whose mag is below 1e-30 (silu's flushed tail) must be below 1e-30 in magnitude themselves.
SLACK = 4 x MEASURED_EXCESS, and MEASURED_EXCESS is the largest (|restate - truth| - r |truth|) / mag over every case of
``ARITH_CASES`` (``measure_excess``; r = 2^-8 for bf16 outputs, 0 for fp32): per operation, in units of 2^-24 = 5.96e-8,
  guidance step 2.55 (fp32 latents, plain, n = 4992 x 128), cond_noise 2.43, adain 1.75, tile_blend 0.97,
  and nothing above the rounding allowance (0.00) for silu, add, stg_blend, the two normalising passes and s2d_skip, whose
  outputs are all bf16
so the largest is 1.518e-7 (recorded as MEASURED_EXCESS = 1.55e-7; tests/test_pointwise_cases.py re-measures it) and SLACK
is 6.2e-7.  4 times, the project's factor (tests/norm_cases.py), for the GPU's exp2 / rcp / division ulps and its
summation order.  Nothing in it comes from a kernel.  ``DROPPED``: the (operation, family) pairs the fp32 restatement
itself cannot pass -- none.  (Measuring it is what found tile_blend's weight: written as the kernel had it, 1 - fp32(z /
extent), the restatement was at 8.57 units on the 33-slice band; ``tile_weight_inputs`` keeps that case.)

THE GUIDANCE SCALARS.  alpha = sum(text uncond) / (sum(uncond^2) + 1e-8) and the rescale factor
rs std(text) / std(out) + (1 - rs) are sums over the whole tensor; each is held to its float64 value within 2^-9
relative (one bf16 rounding: the reference computes ``.std()`` on bf16 tensors).  The kernel does not output them;
``recover_scalars`` recovers them from an fp32-latent call with latents = 0 and dt = -1, which returns
o_i = factor (alpha a_i + c_i) exactly, with a_i = u_i (1 - gs) and c_i = gs t_i + stg (t_i - p_i) known in float64: the
least-squares solution of o = (factor alpha) a + factor c over all elements (float64) gives both, good to the fp32
rounding of o (1e-7), far inside 2^-9.

THRESHOLDS (``cond_noise_threshold_masks``, ``guidance_threshold_case``).  Masks built with ``torch.nextafter`` in fp32
around the value at which the reference's decision flips; the expected decision is the one the oracle makes when run in
float32 (``oracle_resets`` / ``oracle_moves``).
  guidance step: a token moves iff t - 1e-6 < 1 - mask.  A mask in [0.5, 1) is a multiple of 2^-24 and 1 - mask is exact,
  so 1 - mask moves on the grid 2^-24; the masks are 1 - A with A = fp32(t - 1e-6), its two fp32 neighbours (1 - mask =
  A -+ 2^-24) and fp32(1 - t).  fp32 decides (frozen, frozen, moves, moves); float64 sees t - 1e-6 unrounded and moves the
  token at A whenever fp32 rounded A up and A is on the grid.  fp32 rounds A DOWN for every t in [0.25, 1) (1e-6 is
  16.78 x 2^-24 and 33.55 x 2^-25), so no such t exists there, strength 0.5 at t = 0.5 included; it rounds up in
  [0.125, 0.25) (67.1 x 2^-26 -> 67), where A is on the grid for one t in four -- but never for a t of the default
  schedule: its terminal stretch ends in ``1 - x``, so every one of its timesteps is itself on the grid 2^-24 and
  A = t - 67 x 2^-26 is not (the CPU test pins this: on the product's schedule the two runs cannot differ).  The case
  therefore searches oracle.sched.set_timesteps without the terminal stretch, then without shifting
  (``THRESHOLD_SCHEDULES``), step counts 8, 9, ..., for the first t on which the two runs disagree: 19 steps, index 17,
  t = 0.24470679 (deterministic; the CPU test pins the disagreement).
  cond_noise: a token is reset iff mask > 1 - 1e-6.  fp32(1 - 1e-6) = 16777199 x 2^-24 = 0.99999898672, the next fp32
  value is 0.99999904633 and the unrounded 0.999999 lies between them, so for masks that are fp32 values (the only ones
  the kernel can be given) the float32 and the float64 runs of the oracle decide alike on every mask: here the case
  cannot show a disagreement, and the CPU test pins that instead.  It still separates ``>`` from ``>=`` (the mask equal
  to the threshold), which is what a wrong kernel would get wrong.
The truth of a moved token is lat - dt v with the one dt = t - t_next the kernel is given (scheduler_step with the scalar
timestep).  The reference steps a token whose 1 - mask lies within 1e-6 below t from min(t, 1 - mask), i.e. with a dt
smaller by less than 1e-6; the kernel does not, which is a difference of 1e-6 |v| on such tokens only."""
import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

FAMILIES = ["plain", "offset", "tiny", "large", "row_scales"]

# largest excess of the fp32 restatement over the float64 truth across ARITH_CASES (measure_excess); SLACK = 4 x that
MEASURED_EXCESS = 1.55e-7
SLACK_TIMES = 4.0
SLACK = SLACK_TIMES * MEASURED_EXCESS
SCALAR_TOL = 2.0 ** -9
MIN_CHECK_VALUES = 64           # ``check`` is a figure over many roundings: as for the rows of tests/norm_cases.py

# (operation, family) pairs the fp32 restatement itself cannot pass, with the figure it misses (at most 3, never plain)
DROPPED = {}

# Grid caps the geometries below are meant to pass: name -> (blocks, threads, file, text that states the cap there); at the
# time of writing pointwise.hip:11 (pw_grid) and :463 (the guidance launches), upsampler.hip:296 and :328
CAPS = {
    "pw_grid": (256 * 8, 256, "pointwise.hip", "const int64_t cap = 256 * 8;"),
    "guidance": (256, 256, "pointwise.hip", "if (g > 256) g = 256;"),
    "pixel_shuffle2d": (2048, 256, "upsampler.hip", "if (g > 2048) g = 2048;"),
    "tile_blend": (65535, 256, "upsampler.hip", ": 65535);"),
}


def cap_items(name):
    return CAPS[name][0] * CAPS[name][1]


# ----------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make(family, rows, D, seed=0, dtype=BF):
    """[rows, D] of a family, rounded to bf16 (returned as ``dtype`` holding those values)."""
    g = _gen(8000 + 131 * FAMILIES.index(family) + seed)
    x = torch.randn(rows, D, generator=g)
    if family == "plain":
        x = x * 2
    elif family == "offset":
        x = x * 0.5 + 4
    elif family == "tiny":
        x = x * 1e-4
    elif family == "large":
        x = x * 1e4
    elif family == "row_scales":
        x = x * 10.0 ** (torch.rand(rows, 1, generator=g) * 6 - 3)
    else:
        raise KeyError(family)
    return x.to(BF).to(dtype)


def make_like(family, shape, seed=0, dtype=BF):
    """A tensor of ``shape`` whose rows (for row_scales) are its last axis."""
    D = shape[-1]
    n = 1
    for s in shape[:-1]:
        n *= s
    return make(family, n, D, seed, dtype).reshape(shape)


def spread(family):
    return {"plain": 2.0, "offset": 0.5, "tiny": 1e-4, "large": 1e4, "row_scales": 1.0}[family]


# ------------------------------------------------------------------------------------- operations (dtype-generic)
def silu_op(x, dt=F64):
    """oracle.leaves.timestep_embedding_mlp's F.silu (transformer3d.py:428)."""
    y = torch.nn.functional.silu(x.to(dt))
    return y, y.abs()


def add_op(a, b, dt=F64):
    a, b = a.to(dt), b.to(dt)
    return a + b, a.abs() + b.abs()


def stg_blend_op(a, v, m, dt=F64):
    """attention.py:1134-1141: a * m + v * (1 - m), m [B] per sample of a [B, L, D]."""
    a, v, m = a.to(dt), v.to(dt), m.to(dt).view(-1, 1, 1)
    return a * m + v * (1 - m), a.abs() * m.abs() + v.abs() * (1 - m).abs()


def to_ndhwc(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def to_ncdhw(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def unnormalise_op(z, std, mean, dt=F64):
    """oracle.vae.un_normalize_latents on NCDHW z, returned NDHWC."""
    z, s, m = z.to(dt), std.to(dt).view(1, -1, 1, 1, 1), mean.to(dt).view(1, -1, 1, 1, 1)
    return to_ndhwc(z * s + m), to_ndhwc(z.abs() * s.abs() + m.abs().expand_as(z))


def normalise_op(x, c0, C, std, mean, dt=F64):
    """oracle.vae_encoder.normalize_latents on channels c0 .. c0 + C of NDHWC x, returned NCDHW."""
    z = to_ncdhw(x[..., c0:c0 + C].to(dt))
    s, m = std.to(dt).view(1, -1, 1, 1, 1), mean.to(dt).view(1, -1, 1, 1, 1)
    return (z - m) / s, (z.abs() + m.abs()) / s.abs()


def s2d_skip_op(conv, x, stride, group, dt=F64):
    """The tail of oracle.vae_encoder.space_to_depth_downsample: conv NDHWC [B, T', H, W, Cc] (T' = T + 1 when the time
    stride is 2), x NDHWC [B, T, H, W, Cin] -> NDHWC."""
    from oracle import vae_encoder as oe
    st = (stride[0], stride[1], stride[1])
    c, xx = to_ncdhw(conv.to(dt)), to_ncdhw(x.to(dt))
    if st[0] == 2:
        xx = torch.cat([xx[:, :, :1], xx], dim=2)
    xin = oe.space_to_depth(xx, st)
    B, C, D, H, W = xin.shape
    skip = xin.view(B, C // group, group, D, H, W).mean(dim=2)
    skip_mag = xin.abs().view(B, C // group, group, D, H, W).mean(dim=2)
    cs = oe.space_to_depth(c, st)
    return to_ndhwc(cs + skip), to_ndhwc(cs.abs() + skip_mag)


def guidance_parts(npred, gs, stg, rs, do_cfg, do_stg, do_rescale, dt=F64):
    """oracle.sched.guidance in ``dt`` plus what the metrics need: (v, alpha, factor, vmag) with vmag the bracket of the
    guidance step's mag (module docstring) times factor.  npred [num_conds, ...]."""
    from oracle import sched
    nc = npred.shape[0]
    x = npred.to(dt).reshape(nc, -1, 1)                                 # one sample: [num_conds * B, N, C] with B = 1
    v = sched.guidance(x, nc, gs, stg, rs, do_cfg, do_stg, do_rescale).reshape(npred.shape[1:])
    chunks = list(npred.to(dt))
    text = chunks[1] if do_cfg else chunks[0]
    zero = torch.zeros_like(text)
    unc = chunks[0] if do_cfg else zero
    ptb = chunks[-1] if do_stg else zero
    use_cfg = do_cfg and gs != 0 and gs != 1
    alpha = (text * unc).sum() / ((unc * unc).sum() + 1e-8) if use_cfg else torch.ones((), dtype=dt)
    out = alpha * unc + gs * (text - alpha * unc) if use_cfg else text
    factor = torch.ones((), dtype=dt)
    if do_stg:
        out = out + stg * (text - ptb)
        if do_rescale and stg > 0:
            factor = rs * (text.std() / out.std()) + (1 - rs)
    g, s = (abs(gs) if use_cfg else 0.0), (abs(stg) if do_stg else 0.0)
    vmag = factor.abs() * (unc.abs() * (1 + g) * alpha.abs() * (1.0 if use_cfg else 0.0) + text.abs() * (g + s + 1) + ptb.abs() * s)
    return v, alpha, factor, vmag


def guidance_step_op(npred, lat, dt_step, gs, stg, rs, do_cfg, do_stg, do_rescale, dt=F64):
    """oracle.sched.guidance then oracle.sched.scheduler_step's ``sample - dt * model_output``."""
    v, _, _, vmag = guidance_parts(npred, gs, stg, rs, do_cfg, do_stg, do_rescale, dt)
    lat = lat.to(dt).reshape(v.shape)
    return lat - dt_step * v, lat.abs() + abs(dt_step) * vmag


def cond_noise_op(lat, init, noise, mask, noise_scale, t, dt=F64, need=None):
    """oracle.conditioning.add_noise_to_image_conditioning_latents; ``need`` overrides the decision (the float64 truth takes
    the float32 oracle's, see THRESHOLDS)."""
    lat, init, noise = lat.to(dt), init.to(dt), noise.to(dt)
    if need is None:
        need = mask.to(dt) > 1.0 - 1e-6
    noisy = noise_scale * noise * (t ** 2)
    need = need.unsqueeze(-1)
    return torch.where(need, init + noisy, lat), torch.where(need, init.abs() + noisy.abs(), lat.abs())


def adain_op(x, ref, factor, dt=F64):
    """oracle.upsampler.adain_filter_latent, vectorised over the (b, c) planes."""
    x, ref = x.to(dt), ref.to(dt)
    B, C = x.shape[:2]
    xp, rp = x.reshape(B, C, -1), ref.reshape(B, C, -1)
    r_sd, r_mean = torch.std_mean(rp, dim=-1, keepdim=True)
    i_sd, i_mean = torch.std_mean(xp, dim=-1, keepdim=True)
    res = ((xp - i_mean) / i_sd) * r_sd + r_mean
    out = torch.lerp(xp, res, factor)
    mag = xp.abs() + abs(factor) * ((xp.abs() + i_mean.abs()) / i_sd * r_sd + r_mean.abs() + xp.abs())
    return out.reshape(x.shape), mag.reshape(x.shape)


def tile_blend_op(a, b, extent, dim, dt=F64):
    """oracle.vae._blend (blend_z / blend_v / blend_h), vectorised over the band; returns the whole of b."""
    a, b = a.to(dt), b.clone().to(dt)
    e = min(a.shape[dim], b.shape[dim], extent)
    shape = [1] * a.dim()
    shape[dim] = e
    z = torch.arange(e, dtype=F64)
    w, w1 = (z / e).to(dt).view(shape), (1 - z / e).to(dt).view(shape)       # Python doubles there, rounded to the tensor's dtype
    ta, tb = a.narrow(dim, a.shape[dim] - e, e), b.narrow(dim, 0, e)
    mag = b.abs().clone()
    mag.narrow(dim, 0, e).copy_(ta.abs() * w1 + tb.abs() * w)
    b.narrow(dim, 0, e).copy_(ta * w1 + tb * w)
    return b, mag


def unpatchify_ref(x_ndhwc, patch):
    """oracle.vae.unpatchify of an NDHWC tensor -> NCDHW (a pure copy)."""
    from oracle import vae as ov
    return ov.unpatchify(to_ncdhw(x_ndhwc), patch, 1).contiguous()


def patchify_ref(x, patch, c_pad):
    """oracle.vae.patchify of NCDHW pixels -> NDHWC with channels padded with zeros to c_pad."""
    from oracle import vae as ov
    y = to_ndhwc(ov.patchify(x, patch, 1))
    out = torch.zeros(*y.shape[:-1], c_pad, dtype=y.dtype)
    out[..., :y.shape[-1]] = y
    return out


def pixel_shuffle2d_ref(x):
    """oracle.upsampler.pixel_shuffle(dims=2) per frame of packed NDHWC x [B, T, H, W, 4 C] (channel (p1 p2 c)) -> NDHWC."""
    from oracle import upsampler as up
    B, T, H, W, C4 = x.shape
    C = C4 // 4
    ref_order = x.reshape(B * T, H, W, 4, C).permute(0, 4, 3, 1, 2).reshape(B * T, 4 * C, H, W)     # (c p1 p2)
    y = up.pixel_shuffle(ref_order, 2)
    return y.permute(0, 2, 3, 1).reshape(B, T, 2 * H, 2 * W, C).contiguous()


def restate(op, *args, out_dtype=BF, **kw):
    """The operation in fp32 with ONE rounding to the output dtype."""
    out, _ = op(*args, dt=F32, **kw)
    return out.to(out_dtype)


# ----------------------------------------------------------------------------------------------------- metrics
def element_figure(out, truth, mag, slack=SLACK):
    """Worst |out - truth| / bound over live elements, and whether the dead ones are (near) zero."""
    r = 2.0 ** -7 if out.dtype != F32 else 0.0
    o, t, m = out.detach().cpu().to(F64), truth.detach().cpu().to(F64), mag.detach().cpu().to(F64)
    assert o.shape == t.shape == m.shape, (o.shape, t.shape, m.shape)
    live = m >= 1e-30
    dead_ok = bool((o[~live].abs() <= 1e-30).all())
    bound = r * t.abs() + slack * m
    fig = float(((o - t).abs()[live] / bound[live]).max()) if bool(live.any()) else 0.0
    return fig, dead_ok


def compare(out, truth, mag, what="", slack=SLACK):
    """Assert the two metrics; returns the per-element figure as a fraction of its limit."""
    from test_gpu_kernels import check
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite output"
    if float(truth.abs().max()) > 0 and truth.numel() >= MIN_CHECK_VALUES:
        check(out.reshape(truth.shape), truth, what=what)
    fig, dead_ok = element_figure(out.reshape(truth.shape), truth, mag, slack)
    assert dead_ok, f"{what}: an element whose truth is below 1e-30 is not"
    assert fig <= 1, f"{what}: worst element at {fig:.3f} of its bound"
    return fig


def excess(out, truth, mag):
    """max (|out - truth| - r |truth|) / mag, r = 2^-8 for a bf16 output and 0 for fp32: what SLACK is measured from."""
    r = 2.0 ** -8 if out.dtype != F32 else 0.0
    o, t, m = out.to(F64), truth.to(F64), mag.to(F64)
    live = m >= 1e-30
    if not bool(live.any()):
        return 0.0
    return float((((o - t).abs() - r * t.abs()) / m)[live].max())


def recover_scalars(o, npred, gs, stg, do_cfg, do_stg):
    """(alpha, factor) from o = the fp32 latents after a call with latents 0 and dt -1 (module docstring)."""
    x = list(npred.to(F64))
    text = x[1] if do_cfg else x[0]
    use_cfg = do_cfg and gs != 0 and gs != 1
    c = (gs * text if use_cfg else text) + (stg * (text - x[-1]) if do_stg else 0)
    o, c = o.detach().cpu().to(F64).reshape(-1), c.reshape(-1)
    if not use_cfg:
        return None, float((o * c).sum() / (c * c).sum())
    a = (x[0] * (1 - gs)).reshape(-1)
    sol = torch.linalg.lstsq(torch.stack([a, c], 1), o.unsqueeze(1)).solution.reshape(-1)
    return float(sol[0] / sol[1]), float(sol[1])


# ------------------------------------------------------------------------------------------------ thresholds
def cond_noise_threshold_masks():
    """fp32 [4]: 1 - 1e-6 as fp32 evaluates it, its two neighbours, and exactly 1.0 (order: below, at, above, one)."""
    thr = torch.tensor(1.0, dtype=F32) - torch.tensor(1e-6, dtype=F32)
    return torch.stack([torch.nextafter(thr, torch.tensor(0.0)), thr, torch.nextafter(thr, torch.tensor(2.0)),
                        torch.tensor(1.0)])


def oracle_resets(mask, dt=F32):
    """Which tokens add_noise_to_image_conditioning_latents resets, by running the oracle in ``dt``.  mask [1, N]."""
    from oracle import conditioning as oc
    z = torch.zeros(1, mask.shape[1], 1, dtype=dt)
    return oc.add_noise_to_image_conditioning_latents(0.5, z + 1, z, 0.0, mask.to(dt), z)[..., 0] != 0


def oracle_moves(tsch, t, mask, dt=F32):
    """Which tokens denoising_step advances at timestep t, by running the oracle in ``dt``.  mask [1, N]."""
    from oracle import sched
    z = torch.zeros(1, mask.shape[1], 1, dtype=dt)
    return sched.denoising_step(tsch.to(dt), z, z + 1, None, mask.to(dt), t.to(dt))[..., 0] != 0


# set_timesteps arguments searched in this order (module docstring: the default's timesteps cannot show a disagreement)
THRESHOLD_SCHEDULES = [dict(target_shift_terminal=None), dict(shifting=None)]
_threshold_case = []


def guidance_threshold_case(shape=(1, 128, 3, 20, 20)):
    """(timesteps, index, masks fp32 [4]): 1 - masks = A - 2^-24, A, A + 2^-24 with A = fp32(t - 1e-6), and t (to the
    grid of 1 - mask); the first step count from 8 up and the first t in it on which the float64 oracle disagrees with
    the float32 one (module docstring)."""
    from oracle import sched
    if _threshold_case:
        return _threshold_case[0]
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    for steps, kw in [(n, kw) for kw in THRESHOLD_SCHEDULES for n in range(8, 200)]:
        tsch = sched.set_timesteps(steps, shape, **kw)
        for i in range(1, steps - 1):
            t = tsch[i]
            A = t - torch.tensor(1e-6, dtype=F32)
            mA = 1.0 - A
            if not bool(1.0 - mA == A):
                continue
            masks = torch.stack([torch.nextafter(mA, one), mA, torch.nextafter(mA, zero), 1.0 - t])
            m = masks.view(1, -1)
            m32 = oracle_moves(tsch, t, m, F32)
            if m32.tolist() == [[False, False, True, True]] and not torch.equal(m32, oracle_moves(tsch, t, m, F64)):
                _threshold_case.append((tsch, i, masks))
                return tsch, i, masks
    raise AssertionError("no timestep with a float32 / float64 disagreement found")


def threshold_mask(masks4, tokens, seed=5):
    """fp32 [1, tokens]: the four threshold values in every order at the head, then seeded picks of them, 0.0 and 0.3."""
    pool = torch.cat([masks4, torch.tensor([0.0, 0.3])])
    idx = torch.randint(0, pool.numel(), (tokens,), generator=_gen(9900 + seed))
    idx[:4] = torch.arange(4)
    idx[-4:] = torch.arange(3, -1, -1)
    return pool[idx].view(1, tokens).contiguous()


# ----------------------------------------------------------- the arithmetic cases: (operation, family, geometry)
SILU_SIZES = [8, 8 * (2048 * 256 + 5)]                      # one chunk; a second trip of pw_grid with a ragged end
STG_M = [1.0, 0.0, 0.25]
# (B, L, D, lda, ldv): ldv == 3 D means v is the middle column block of a packed [rows, 3 D] buffer
STG_GEOMS = [(3, 20, 8, 24, 40), (3, 5, 2048, 2048 + 8, 2048 + 16), (3, 1400, 1024, 1024, 3 * 1024)]
# (B, C, T, H, W)
LAYOUT_SHAPES = [(2, 16, 3, 5, 7), (1, 1, 3, 5, 7), (2, 128, 3, 33, 23)]
NORMALISE_PAD = (3, 5)                                      # c0, extra channels after c0 + C: ldx = c0 + C + 5
# (stride_t, stride_hw, group, B, T, H, W, Cin)
S2D_GEOMS = [(2, 1, 1, 2, 1, 3, 5, 16), (1, 2, 2, 1, 4, 6, 10, 16), (2, 2, 4, 2, 5, 6, 10, 32), (2, 2, 4, 1, 3, 128, 132, 32)]
GUIDANCE_N = [2, 255, 256, 257, 65536 + 3, 4992 * 128]
# (guidance_scale, stg_scale, rescaling_scale, do_cfg, do_stg, do_rescale): the four of test_guidance_step, then guidance
# scale exactly 1.0 and 0.0 with do_cfg set (the branch that must return text)
GUIDANCE_SETTINGS = [(3.0, 1.0, 0.7, True, True, True), (0.0, 1.0, 0.7, False, True, True), (3.0, 0.0, 1.0, True, False, False),
                     (3.0, 1.0, 1.0, True, True, False), (1.0, 1.0, 0.7, True, True, True), (0.0, 1.0, 0.7, True, True, True)]
GUIDANCE_DT = 0.0371
MASKED_GEOMS = [(37, 1), (4100, 128)]                       # (tokens, channels)
COND_NOISE = (0.15, 0.63)                                   # noise_scale, t
# (B, C, latent plane, reference plane)
ADAIN_GEOMS = [(2, 5, (3, 8, 10), (3, 4, 5)), (1, 3, (1, 1, 2), (1, 2, 2)), (1, 4, (1, 2, 3), (1, 1, 2))]
ADAIN_FACTORS = [0.0, 1.0, 0.25]
ADAIN_OFFSET = 100.0
# (shape of a, length of b along dim, dim, extent)
TILE_GEOMS = [((1, 3, 9, 16, 24), 7, 2, 1), ((1, 3, 9, 16, 24), 12, 3, 5), ((1, 2, 33, 256, 1000), 33, 2, 33)]
PIXEL_SHUFFLE_SHAPE = (1, 3, 210, 209, 32)                  # C = 8: 3 * 4 * 210 * 209 chunks
# (B, T, H, W, C_out, patch, input offset in elements)
UNPATCHIFY_GEOMS = [(1, 3, 420, 417, 3, 4, 0), (2, 3, 5, 7, 3, 4, 0), (1, 3, 210, 209, 3, 2, 0), (1, 1, 106, 104, 4, 4, 0),
                    (1, 3, 421, 417, 3, 1, 0), (1, 3, 420, 417, 3, 4, 4)]
# (B, C, T, H, W, patch, C_pad)
PATCHIFY_GEOMS = [(1, 3, 3, 212, 208, 4, 64), (2, 5, 3, 411, 43, 1, 5), (2, 3, 3, 8, 12, 4, 64)]


def guidance_inputs(family, n, num_conds, lat_dtype):
    """npred bf16 [num_conds, n, 1] in the kernel's chunk order (uncond, text, perturbed; text is always there) and the
    latents [1, n, 1]."""
    text = make(family, 1, n, seed=31).float()
    g = _gen(9800 + FAMILIES.index(family))
    others = [(text + 0.3 * spread(family) * torch.randn(1, n, generator=g)).to(BF) for _ in range(2)]
    rows = {1: [text], 2: [others[0], text], 3: [others[0], text, others[1]]}
    lat = make("plain", 1, n, seed=32).float() * 0.5
    return torch.cat([r.to(BF) for r in rows[num_conds]]).reshape(num_conds, n, 1), lat.to(BF).to(lat_dtype).reshape(1, n, 1)


def guidance_npred(family, n, do_cfg, do_stg):
    """npred for a setting: rows (uncond if do_cfg, text, perturbed if do_stg)."""
    full, _ = guidance_inputs(family, n, 3, F32)
    keep = ([0] if do_cfg else []) + [1] + ([2] if do_stg else [])
    return full[keep].contiguous()


def stg_inputs(family, geom):
    """(a buffer [B, L, lda], v buffer [B, L, ldv], column offset of v, m): a = abuf[..., :D], v = vbuf[..., off:off + D]."""
    B, L, D, lda, ldv = geom
    abuf = make_like(family, (B, L, lda), seed=41)
    vbuf = make_like(family, (B, L, ldv), seed=42)
    off = D if ldv == 3 * D else 0
    return abuf, vbuf, off, torch.tensor(STG_M[:B])


def layout_inputs(family, shape):
    """(z NCDHW, x NDHWC with padded channels, std, mean fp32 [C]) of a layout case."""
    B, C, T, H, W = shape
    c0, extra = NORMALISE_PAD
    z = to_ncdhw(make_like(family, (B, T, H, W, C), seed=51))
    x = make_like(family, (B, T, H, W, c0 + C + extra), seed=52)
    g = _gen(9700)
    return z, x, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * spread(family)


def s2d_inputs(family, geom):
    st, s, group, B, T, H, W, Cin = geom
    Tc = T + 1 if st == 2 else T
    return make_like(family, (B, Tc, H, W, Cin // group), seed=61), make_like(family, (B, T, H, W, Cin), seed=62)


def masked_inputs(family, tokens, channels, dtype):
    """(lat, init, noise) [1, tokens, channels] of ``dtype`` holding bf16 values."""
    return tuple(make_like(family, (1, tokens, channels), seed=70 + k, dtype=dtype) for k in range(3))


def adain_inputs(family, geom, dtype):
    B, C, pl, pr = geom
    x = make_like(family, (B, C) + pl, seed=81).float()
    r = make_like(family, (B, C) + pr, seed=82).float() * 0.5
    if family == "offset":
        x, r = x + ADAIN_OFFSET, r - ADAIN_OFFSET / 2
    return x.to(BF).to(dtype), r.to(BF).to(dtype)


def tile_inputs(geom, dtype=BF):
    sa, lb, dim, _ = geom
    sb = list(sa)
    sb[dim] = lb
    return make_like("plain", tuple(sa), seed=91, dtype=dtype), make_like("plain", tuple(sb), seed=92, dtype=dtype)


def tile_weight_inputs():
    """fp32 a and an all-zero b over a 33-slice band: out = a (1 - z / 33), so the weight of ``a`` alone is on test.  The
    weight written 1.0f - fp32(z / 33) carries the rounding of z / 33, up to 1e-6 of 1 / 33 at z = 32."""
    a = make_like("plain", (1, 2, 33, 8, 24), seed=93, dtype=F32)
    return a, torch.zeros_like(a)


def tile_blend_one_minus_w(a, b, extent, dim):
    """tile_blend in fp32 with the weight of ``a`` formed as 1 - fp32(z / extent): the kernel's former arithmetic, for the
    teeth test only."""
    e = min(a.shape[dim], b.shape[dim], extent)
    shape = [1] * a.dim()
    shape[dim] = e
    w = (torch.arange(e, dtype=F32) / e).view(shape)
    out = b.clone().float()
    out.narrow(dim, 0, e).copy_(a.float().narrow(dim, a.shape[dim] - e, e) * (1.0 - w) + out.narrow(dim, 0, e) * w)
    return out


def _fams(small):
    return FAMILIES if small else ["plain"]


def arith_cases():
    """[(operation, family, geometry key)]: every arithmetic case the GPU module runs."""
    cases = []
    for op in ("silu", "add"):
        cases += [(op, f, n) for n in SILU_SIZES for f in FAMILIES]
    cases += [("stg_blend", f, g) for g in STG_GEOMS for f in _fams(g[1] < 1000)]
    for op in ("unnormalise", "normalise"):
        cases += [(op, f, s) for s in LAYOUT_SHAPES for f in _fams(s[1] <= 16)]
    cases += [("s2d_skip", f, g) for g in S2D_GEOMS for f in _fams(g[5] < 100)]
    for lt in ("f32", "bf16"):
        cases += [("guidance_" + lt, f, (n, k)) for n in GUIDANCE_N for k in range(len(GUIDANCE_SETTINGS))
                  for f in ("plain", "offset")]
        cases += [("cond_noise_" + lt, f, g) for g in MASKED_GEOMS for f in _fams(g[0] < 100)]
        cases += [("adain_" + lt, f, (g, fac)) for g in ADAIN_GEOMS for fac in ADAIN_FACTORS for f in _fams(g is ADAIN_GEOMS[0])]
    cases += [("tile_blend", "plain", g) for g in TILE_GEOMS]
    return [c for c in cases if (c[0], c[1]) not in DROPPED]


ARITH_CASES = arith_cases()


def arith_truth(op, family, geom):
    """(operation function, its arguments, keyword arguments, output dtype) of a case; truth = fn(*args, **kw)."""
    lt = F32 if op.endswith("_f32") else BF
    if op == "silu":
        return silu_op, (make(family, 1, geom, seed=11),), {}, BF
    if op == "add":
        return add_op, (make(family, 1, geom, seed=12), make(family, 1, geom, seed=13)), {}, BF
    if op == "stg_blend":
        abuf, vbuf, off, m = stg_inputs(family, geom)
        D = geom[2]
        return stg_blend_op, (abuf[..., :D], vbuf[..., off:off + D], m), {}, BF
    if op == "unnormalise":
        z, _, std, mean = layout_inputs(family, geom)
        return unnormalise_op, (z, std, mean), {}, BF
    if op == "normalise":
        _, x, std, mean = layout_inputs(family, geom)
        return normalise_op, (x, NORMALISE_PAD[0], geom[1], std, mean), {}, BF
    if op == "s2d_skip":
        conv, x = s2d_inputs(family, geom)
        return s2d_skip_op, (conv, x, (geom[0], geom[1]), geom[2]), {}, BF
    if op.startswith("guidance_"):
        n, k = geom
        gs, stg, rs, do_cfg, do_stg, do_res = GUIDANCE_SETTINGS[k]
        _, lat = guidance_inputs(family, n, 3, lt)
        return guidance_step_op, (guidance_npred(family, n, do_cfg, do_stg), lat, GUIDANCE_DT, gs, stg, rs, do_cfg, do_stg,
                                  do_res), {}, lt
    if op.startswith("cond_noise_"):
        tokens, channels = geom
        lat, init, noise = masked_inputs(family, tokens, channels, lt)
        mask = threshold_mask(cond_noise_threshold_masks(), tokens)
        return cond_noise_op, (lat, init, noise, mask, *COND_NOISE), {"need": oracle_resets(mask)}, lt
    if op.startswith("adain_"):
        g, fac = geom
        x, r = adain_inputs(family, g, lt)
        return adain_op, (x, r, fac), {}, lt
    if op == "tile_blend":
        a, b = tile_inputs(geom)
        return tile_blend_op, (a, b, geom[3], geom[2]), {}, BF
    raise KeyError(op)


def cpu_case(op, family, geom):
    """(fp32 restatement in the output dtype, truth, mag) of one case."""
    fn, args, kw, od = arith_truth(op, family, geom)
    truth, mag = fn(*args, **kw)
    return restate(fn, *args, out_dtype=od, **kw), truth, mag


def op_group(op):
    return op.rsplit("_", 1)[0] if op.endswith(("_f32", "_bf16")) else op


def measure_excess(cases=None):
    """{operation: largest excess} over every case; what MEASURED_EXCESS records."""
    worst = {}
    for op, fam, geom in (ARITH_CASES if cases is None else cases):
        out, truth, mag = cpu_case(op, fam, geom)
        worst[op_group(op)] = max(worst.get(op_group(op), 0.0), excess(out, truth, mag))
    return worst


if __name__ == "__main__":
    for k, v in measure_excess().items():
        print(f"{k}: {v:.3e} = {v / 2.0 ** -24:.2f} x 2^-24")
