// conv_plan.hip -- the convolution's host side: which of the four forms a call runs as (the implicit GEMM of gemm.hip with
// 128- or 256-wide tiles, the eight- or four-wave direct convolution of conv_direct.hip), how it is laid out on the chip, the one
// validation of a call, and the entry points.  Pure host arithmetic: no kernel lives here.
#include "conv.h"

namespace ltxmi {

// the shapes the direct convolution takes at all (either form)
static bool conv3d_direct_takes(const ltxmi_conv3d_args* a) {
    const int st = a->stride_t > 0 ? a->stride_t : 1, sh = a->stride_hw > 0 ? a->stride_hw : 1;
    const int kt = a->kernel_t > 0 ? a->kernel_t : 3;
    if (st != 1 || sh != 1 || kt != 3 || a->out_T > 0 || a->tpad > 0) return false;
    if (a->Cin % 64 != 0 || a->Cout % 8 != 0 || !a->bias) return false;
    if ((int64_t)a->B * a->T * a->H * a->W * a->Cin * 2 >= 0x7ffffff0ll) return false;   // halo rows are addressed with 32-bit byte offsets
    if (a->d2s && (a->Cout % 1024 != 0 || a->add)) return false;       // a 128-column block must be one (p1 p2 p3)
    // the residual's channel wrap (c' mod Cres/8) is a mask in the four-wave form
    if (a->d2s && a->residual && (a->res_channels < 8 || ((a->res_channels >> 3) & ((a->res_channels >> 3) - 1)) != 0)) return false;
    return true;
}
// whole 128-channel blocks: the four-wave form, two workgroups per CU (algo 3 asks for it, algo 4 for the eight-wave form)
// (from 768 workgroups = 1.5 rounds of the chip's 512 slots; measured: 896 workgroups +5.8 %, 600 -0.6 %, 224 -21 %)
static bool conv3d_direct_four_wave_form(const ltxmi_conv3d_args* a, int64_t grid) {
    return a->Cout % 128 == 0 && grid < (1ll << 31) && ((a->algo != 4 && grid >= 768) || a->algo == 3);
}

// How a call is laid out on the chip.  Tiles are 2 (t) x 8 x 16 positions; the 16-position direction is W, or H (swap: the
// four-wave form only).  ksplit > 1: the input channels in ksplit ranges with fp32 partial sums and a finalising pass -- for the
// wide, short layers (Cin >= 1024: the partial sums are Cin / (4 ksplit) times smaller than the halo traffic they replace) whose
// tiles do not fill the chip: 1024 -> 1024 at 13 x 16 x 24 positions is 224 tiles of which 70 % of the positions exist (W = 24
// is 1.5 tiles); swapped it is 168 tiles at 93 %, and three channel ranges make 504 workgroups for the 512 slots.
static ConvPlan conv3d_plan(const ltxmi_conv3d_args* a) {      // a != NULL, sizes positive; algo honoured as given
    ConvPlan pl = {};
    // output grid: nn.Conv3d arithmetic on the padded input (time padded by tpad frames in front, and by one replicated frame
    // behind when not causal; space padded by 1): floor((L + pad - 3) / s) + 1
    pl.sT = a->stride_t > 0 ? a->stride_t : 1; pl.sHW = a->stride_hw > 0 ? a->stride_hw : 1;
    pl.kt = a->kernel_t > 0 ? a->kernel_t : 3;       // 1: a 3x3 nn.Conv2d applied to every frame
    pl.tpad = pl.kt == 1 ? 0 : (a->tpad > 0 ? a->tpad : (a->causal ? 2 : 1));
    const int tpad_back = (pl.kt == 1 || a->tpad > 0 || a->causal) ? 0 : 1;
    pl.oT = a->out_T > 0 ? a->out_T : (a->T + pl.tpad + tpad_back - pl.kt) / pl.sT + 1;
    pl.oH = (a->H + 2 - 3) / pl.sHW + 1; pl.oW = (a->W + 2 - 3) / pl.sHW + 1;
    pl.M = (int64_t)a->B * pl.oT * pl.oH * pl.oW;
    pl.epi = a->d2s ? 2 : (a->add ? 1 : 0);
    pl.ksplit = 1;
    const ConvRoute gemm = conv3d_gemm_tile(pl.M, a->Cout) == 256 ? CONV_GEMM256 : CONV_GEMM128;
    if (a->algo == 1 || !conv3d_direct_takes(a)) {
        pl.route = a->algo >= 2 ? CONV_REFUSED : gemm;
        return pl;
    }
    pl.tiles_t = (a->T + CONV_TT - 1) / CONV_TT; pl.tiles_n = (a->Cout + 127) / 128;
    const int64_t per = (int64_t)a->B * pl.tiles_t * pl.tiles_n;
    const int64_t g_n = per * ((a->H + 7) / 8) * ((a->W + 15) / 16), g_s = per * ((a->W + 7) / 8) * ((a->H + 15) / 16);
    bool four_wave = conv3d_direct_four_wave_form(a, g_n);
    const double positions = (double)a->B * pl.tiles_t * CONV_TT * a->H * a->W * pl.tiles_n;       // (x 128 channels each, t rounded up)
    auto eff4 = [&](int64_t g, int S) {           // useful share of the tiles x fill of the last round of 512 slots - the split's price
        const double rounds = (double)g * S / 512.0;
        return positions / ((double)g * 256.0) * rounds / (double)(int64_t)(rounds + 0.999999) - 0.03 * (S - 1);
    };
    const double eff_now = four_wave ? eff4(g_n, 1)
                                     : positions / ((double)g_n * 256.0) * ((double)g_n / 256.0) / (double)((g_n + 255) / 256) * 0.93;
    // The channel split: the product's own choice (algo 0 / 2 / 3), output rows the finalising pass takes (512 or n x 1024
    // channels).  Cin >= 1024: wherever it buys more than 5 % of the launch at 3 % per extra range.  512 <= Cin < 1024 (the partial
    // sums cost twice as much per FLOP): two ranges only, and only for a call that asks for a norm the unsplit form could not
    // fuse -- the finalising pass replaces that launch (0.084 ms beside a 0.55-ms convolution at the decoder's 512-channel stage,
    // whose 624 workgroups are 2.44 rounds of the eight-wave form), which the efficiency figure does not see.
    const int nch = a->Cin / 32;
    const bool rows_ok = (a->Cout == 512 || a->Cout % 1024 == 0) && a->Cout <= 4096;
    const bool wants_unfusable_norm = a->post_norm && !(a->Cout == 128 || (a->d2s && a->Cout == 1024));
    if (rows_ok && a->Cin % 32 == 0 && a->algo != 1 && a->algo != 4 && (a->Cin >= 1024 || (a->Cin >= 512 && wants_unfusable_norm))) {
        const int64_t g = g_s < g_n ? g_s : g_n;
        const bool wide = a->Cin >= 1024;
        const double price = wide ? 0.03 : 0.06;
        int best = 1;
        double best_eff = wide ? eff_now + 0.05 : eff_now - 0.05;
        for (int S = 2; S <= (wide ? 4 : 2) && S * 4 <= nch; ++S) {
            const double e = eff4(g, S) + 0.03 * (S - 1) - price * (S - 1);
            if (g * S < (1ll << 31) && e > best_eff) { best = S; best_eff = e; }
        }
        if (best > 1) {
            pl.split_bytes = (int64_t)best * a->B * a->T * a->H * a->W * a->Cout * 4;
            if (a->workspace && a->workspace_bytes >= pl.split_bytes && (((uintptr_t)a->workspace) & 15) == 0) {
                pl.ksplit = best; four_wave = true; pl.swap = g_s < g_n;
            }
        }
    }
    if (pl.ksplit == 1 && four_wave && (g_s + 511) / 512 < (g_n + 511) / 512) pl.swap = 1;    // fewer rounds of the chip
    pl.tiles_8 = pl.swap ? (a->W + 7) / 8 : (a->H + 7) / 8;
    pl.tiles_16 = pl.swap ? (a->H + 15) / 16 : (a->W + 15) / 16;
    pl.grid = per * pl.tiles_8 * pl.tiles_16;
    // post_norm rides along where a wave holds every channel of its output positions: ONE 128-channel block of the four-wave
    // form (plain store; with `add` only as the second output y_norm beside the raw y), or its depth-to-space store to 128
    // channels (second output only: a 128-column block is one (p1 p2 p3)) -- and on every call split over its input channels
    // (the finalising pass holds whole rows).  Without y_norm the activated result is the only output: the plain store only.
    if (a->y_norm || !(a->add || a->d2s)) {
        pl.fuses_post_norm = pl.ksplit > 1 ||
                             (four_wave && (a->y_norm ? (a->d2s && a->Cout == 1024) || (!a->d2s && a->add && a->Cout == 128)
                                                      : a->Cout == 128));
    }
    if (four_wave) {
        pl.route = CONV_DIRECT4;
        pl.epi = pl.ksplit > 1 ? 6 : pl.epi + (a->post_norm && pl.fuses_post_norm ? 3 : 0);
    } else if (pl.grid >= (1ll << 31) || (pl.grid < 128 && a->algo < 2)) {
        // one eight-wave workgroup per CU is resident: below ~half the CUs the implicit GEMM's smaller tiles fill the chip
        // better (algo >= 2 asks for the direct convolution whatever the grid)
        pl.route = a->algo >= 2 ? CONV_REFUSED : gemm;
    } else {
        pl.route = CONV_DIRECT8;
    }
    return pl;
}

// the two queries: fields of the plan of the arguments as given (0 without a bias -- the direct convolution needs one)
static bool conv3d_plannable(const ltxmi_conv3d_args* a) {
    return a != nullptr && a->bias != nullptr && a->B > 0 && a->T > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0;
}
extern "C" int ltxmi_conv3d_fuses_post_norm(const ltxmi_conv3d_args* a) { return conv3d_plannable(a) && conv3d_plan(a).fuses_post_norm; }
extern "C" int64_t ltxmi_conv3d_workspace_bytes(const ltxmi_conv3d_args* a) { return conv3d_plannable(a) ? conv3d_plan(a).split_bytes : 0; }

// The ONE place that validates a convolution call and plans it: ltxmi_conv3d_ndhwc_bf16 launches what this leaves in *pl and
// ltxmi_conv3d_route reports it.  Pure host arithmetic on the struct: no device call, no device memory read.  Returns LTXMI_OK
// with the plan in *pl, or the negative ltxmi_status (error text set).
static int conv3d_check(const ltxmi_conv3d_args* a, ConvPlan* plan) {
    LTXMI_REQUIRE(a && a->x && a->w && a->y, LTXMI_ERR_INVALID_ARG, "ltxmi_conv3d_ndhwc_bf16: NULL argument");
    LTXMI_REQUIRE(a->B > 0 && a->T > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_conv3d_ndhwc_bf16: non-positive shape");
    // the spatial padding mode: it chooses nothing in the plan (a reflect call runs on the route of its replicate twin)
    LTXMI_REQUIRE(a->pad_replicate >= CONV_PAD_ZEROS && a->pad_replicate <= CONV_PAD_REFLECT, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_conv3d_ndhwc_bf16: pad_replicate = %d is no spatial padding mode (0 zeros, 1 replicate, 2 reflect)",
                  a->pad_replicate);
    LTXMI_REQUIRE(a->pad_replicate != CONV_PAD_REFLECT || (a->H >= 2 && a->W >= 2), LTXMI_ERR_INVALID_ARG,
                  "ltxmi_conv3d_ndhwc_bf16: reflect padding needs H >= 2 and W >= 2 (got %d x %d): the mirror of a "
                  "single row or column does not exist", a->H, a->W);
    const ConvPlan pl = *plan = conv3d_plan(a);
    LTXMI_REQUIRE(a->Cin % 64 == 0, LTXMI_ERR_UNSUPPORTED, "ltxmi_conv3d_ndhwc_bf16: Cin=%d must be a multiple of 64", a->Cin);
    LTXMI_REQUIRE(a->Cout % 8 == 0, LTXMI_ERR_UNSUPPORTED, "ltxmi_conv3d_ndhwc_bf16: Cout=%d must be a multiple of 8", a->Cout);
    LTXMI_REQUIRE((pl.sT == 1 || pl.sT == 2) && (pl.sHW == 1 || pl.sHW == 2), LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_conv3d_ndhwc_bf16: strides must be 1 or 2");
    LTXMI_REQUIRE(pl.kt == 3 || (pl.kt == 1 && pl.sT == 1 && a->tpad == 0 && a->out_T == 0), LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_conv3d_ndhwc_bf16: kernel_t must be 3, or 1 without time stride/padding");
    LTXMI_REQUIRE(!(a->d2s && (pl.sT != 1 || pl.sHW != 1 || pl.oT != a->T)), LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_conv3d_ndhwc_bf16: depth-to-space store needs a stride-1, same-size convolution");
    LTXMI_REQUIRE(pl.M < (1ll << 31) && (int64_t)a->B * (2 * a->T) * (2 * a->H) * (2 * a->W) < (1ll << 31),
                  LTXMI_ERR_UNSUPPORTED, "ltxmi_conv3d_ndhwc_bf16: too many positions");
    if (a->d2s) {
        LTXMI_REQUIRE(a->Cout % 32 == 0, LTXMI_ERR_UNSUPPORTED,
                      "ltxmi_conv3d_ndhwc_bf16: depth-to-space needs Cout %% 32 == 0 (got %d)", a->Cout);
        if (a->residual)
            LTXMI_REQUIRE(a->res_channels > 0 && a->res_channels % 8 == 0, LTXMI_ERR_INVALID_ARG,
                          "ltxmi_conv3d_ndhwc_bf16: bad residual channel count %d", a->res_channels);
    }
    LTXMI_REQUIRE((((uintptr_t)a->x | (uintptr_t)a->w) & 15) == 0 && (((uintptr_t)a->y | (uintptr_t)a->bias) & 7) == 0,
                  LTXMI_ERR_UNSUPPORTED, "ltxmi_conv3d_ndhwc_bf16: misaligned pointer");
    LTXMI_REQUIRE(a->algo >= 0 && a->algo <= 4, LTXMI_ERR_INVALID_ARG, "ltxmi_conv3d_ndhwc_bf16: algo %d not in {0 .. 4}", a->algo);
    LTXMI_REQUIRE(a->workspace_bytes >= 0 && (a->workspace != nullptr || a->workspace_bytes == 0), LTXMI_ERR_INVALID_ARG,
                  "ltxmi_conv3d_ndhwc_bf16: workspace_bytes without a workspace");
    if (a->post_norm) {
        LTXMI_REQUIRE(a->post_norm == 1 && (a->post_scale != nullptr) == (a->post_shift != nullptr) && a->post_eps >= 0.f,
                      LTXMI_ERR_INVALID_ARG, "ltxmi_conv3d_ndhwc_bf16: post_norm must be 0 or 1, post_scale / post_shift both given or both NULL");
        LTXMI_REQUIRE((((uintptr_t)a->post_scale | (uintptr_t)a->post_shift) & 15) == 0, LTXMI_ERR_UNSUPPORTED,
                      "ltxmi_conv3d_ndhwc_bf16: misaligned post_scale / post_shift");
        LTXMI_REQUIRE(((uintptr_t)a->y_norm & 15) == 0 && a->y_norm != a->y, LTXMI_ERR_INVALID_ARG,
                      "ltxmi_conv3d_ndhwc_bf16: y_norm must be 16-byte aligned and distinct from y");
        LTXMI_REQUIRE(pl.fuses_post_norm, LTXMI_ERR_UNSUPPORTED,
                      "ltxmi_conv3d_ndhwc_bf16: post_norm is applied by the four-wave direct convolution where a wave holds all "
                      "channels of a position (ask ltxmi_conv3d_fuses_post_norm first)");
    } else {
        LTXMI_REQUIRE(a->y_norm == nullptr, LTXMI_ERR_INVALID_ARG, "ltxmi_conv3d_ndhwc_bf16: y_norm without post_norm");
    }
    LTXMI_REQUIRE(pl.route != CONV_REFUSED, LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_conv3d_ndhwc_bf16: algo = %d (direct convolution) does not take this shape", a->algo);
    // (`d2s` with `add` never reaches the direct forms: conv3d_direct_takes)
    LTXMI_REQUIRE(!(a->d2s && a->add), LTXMI_ERR_INVALID_ARG, "ltxmi_conv3d_ndhwc_bf16: `add` is for the plain store only");
    return LTXMI_OK;
}

extern "C" int ltxmi_conv3d_route(const ltxmi_conv3d_args* a, ltxmi_conv3d_route_info* out) {
    LTXMI_REQUIRE(out != nullptr, LTXMI_ERR_INVALID_ARG, "ltxmi_conv3d_route: NULL out");
    *out = ltxmi_conv3d_route_info{-1, 0, 0, 0, 0};
    ConvPlan pl;
    if (const int rc = conv3d_check(a, &pl)) return rc;
    out->route = (int32_t)pl.route;               // CONV_GEMM128 .. CONV_DIRECT4 are 0 .. 3, the header's numbering
    out->epilogue = pl.epi;
    out->ksplit = pl.ksplit;
    out->swap_hw = pl.swap;
    out->finalize_blocks = pl.ksplit > 1 ? a->Cout / 256 : 0;
    return LTXMI_OK;
}

extern "C" int ltxmi_conv3d_ndhwc_bf16(const ltxmi_conv3d_args* a, void* stream) {
    ConvPlan pl;
    if (const int rc = conv3d_check(a, &pl)) return rc;
    if (pl.route == CONV_DIRECT4 || pl.route == CONV_DIRECT8) return launch_conv3d_direct(a, pl, (hipStream_t)stream);
    return launch_conv3d_gemm(a, pl, (hipStream_t)stream);
}

}  // namespace ltxmi
