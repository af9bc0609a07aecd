// stream32.hip -- row kernels of the mixed-precision DiT path: the residual stream is fp32, everything that feeds a
// linear is bf16 (the reference's `mixed=True`, transformer3d.py:439-442, attention.py:231-364).
//
// Same shape as rowops.hip: HBM-bound passes, 16-byte accesses, a lane owns 8 consecutive channels (32 bytes of the fp32
// stream = two 16-byte accesses, 16 bytes of every bf16 operand), fixed order, no LDS, no atomics.
//   norm_modulate_f32in : one wave per row, the row held in registers between the reduction and the modulation
//   gate_residual_f32   : no reduction -> one lane per 8-channel chunk over the flat [rows, D / 8] index, so narrow rows
//                         share a wave
#include "rows.h"

// What is rounded where is the specification of this path (include/ltxmi.h): every sum and product below is the single
// correctly rounded fp32 operation it is written as, whatever -ffast-math allows elsewhere.
#pragma clang fp reassociate(off) contract(off)

namespace ltxmi {

// ------------------------------------------------- norm + AdaLN modulate, fp32 rows in, bf16 rows out
// norm_modulate_kernel of rowops.hip with the row read as fp32: the statistics and the modulation are fp32 from the
// unrounded stream, the only rounding is the bf16 store (autocast's cast at the linear that consumes the row).
template <int NCH, bool LAYER>
__global__ __launch_bounds__(256) void norm_modulate_f32in_kernel(
    const float* __restrict__ x, int64_t ldx, uint16_t* __restrict__ y, int64_t ldy, int rows, int D, float eps,
    const uint16_t* __restrict__ sc_tab, const uint16_t* __restrict__ sc_temb, const uint16_t* __restrict__ sh_tab,
    const uint16_t* __restrict__ sh_temb, int64_t temb_ld, int rows_per_group) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nchunk = D >> 3;
    const float* xr = x + (int64_t)row * ldx;
    Chunk c[NCH];
    float s1 = 0.f, s2 = 0.f;
    LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
        c[j] = load_f32x8(xr + ch * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (LAYER) s1 += c[j].v[e];
            else s2 += c[j].v[e] * c[j].v[e];
        }
    }
    float mean = 0.f;
    if (LAYER) {
        // variance about the mean from the registers, as norm_modulate_kernel<LAYER>
        mean = wave_sum(s1) / D;
        s2 = 0.f;
        LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = c[j].v[e] - mean;
                s2 += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(s2) / D + eps);
    const int64_t g = (int64_t)(row / rows_per_group) * temb_ld;
    uint16_t* yr = y + (int64_t)row * ldy;
    LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
        const Chunk a = load_bf16x8(sc_tab + ch * 8), a2 = load_bf16x8(sc_temb + g + ch * 8);
        const Chunk b = load_bf16x8(sh_tab + ch * 8), b2 = load_bf16x8(sh_temb + g + ch * 8);
        Chunk o;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            o.v[e] = (c[j].v[e] - mean) * rstd * (1.0f + (a.v[e] + a2.v[e])) + (b.v[e] + b2.v[e]);
        store_bf16x8(yr + ch * 8, o);
    }
}

// ------------------------------------------------- h += gate * y on the fp32 stream (+ the bf16 copy of the new row)
// GATED: gate = table + temb row of the group; else gate = 1 (attn2).  ROUND: the product goes through bf16 first
// (attention.py:285 multiplies the bf16 attention output in place); else it stays fp32 (:348, the FF output lives in an
// fp32 buffer by then).
template <bool GATED, bool ROUND, bool COPY>
__global__ __launch_bounds__(256) void gate_residual_f32_kernel(float* __restrict__ h, int64_t ldh,
                                                                const uint16_t* __restrict__ y, int64_t ldy, int nchunk,
                                                                uint32_t total, const uint16_t* __restrict__ g_tab,
                                                                const uint16_t* __restrict__ g_temb, int64_t gate_ld,
                                                                int rows_per_group, uint16_t* __restrict__ hb, int64_t ldhb) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / (uint32_t)nchunk;
    const int c0 = (int)(idx - row * (uint32_t)nchunk) * 8;
    float* hp = h + (int64_t)row * ldh + c0;
    Chunk acc = load_f32x8(hp);
    const Chunk yv = load_bf16x8(y + (int64_t)row * ldy + c0);
    if (GATED) {
        const Chunk gt = load_bf16x8(g_tab + c0);
        const Chunk ge = load_bf16x8(g_temb + (int64_t)(row / (uint32_t)rows_per_group) * gate_ld + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float gate = gt.v[e] + ge.v[e];
            // ROUND: three single roundings (product, bf16, sum).  Else one fused multiply-add: the unrounded product, and an
            // error of half an ulp of the sum where a separate product and sum could be a whole ulp and a half off
            if (ROUND) acc.v[e] = acc.v[e] + bf2f(f2bf(gate * yv.v[e]));
            else acc.v[e] = __builtin_fmaf(gate, yv.v[e], acc.v[e]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc.v[e] = acc.v[e] + yv.v[e];
    }
    store_f32x8(hp, acc);
    if (COPY) store_bf16x8(hb + (int64_t)row * ldhb + c0, acc);
}

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_norm_modulate_f32in_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t D,
                                              float eps, int32_t kind, const void* scale_table, const void* scale_temb,
                                              const void* shift_table, const void* shift_temb, int64_t temb_ld,
                                              int32_t rows_per_group, void* stream) {
    LTXMI_REQUIRE(x && y && scale_table && scale_temb && shift_table && shift_temb, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_norm_modulate_f32in_bf16: NULL argument");
    LTXMI_REQUIRE(rows > 0 && D > 0 && rows_per_group > 0, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_norm_modulate_f32in_bf16: non-positive size rows=%d D=%d rows_per_group=%d", rows, D, rows_per_group);
    LTXMI_REQUIRE(kind == LTXMI_NORM_RMS || kind == LTXMI_NORM_LAYER, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_norm_modulate_f32in_bf16: bad kind %d", kind);
    LTXMI_REQUIRE((const void*)x != (const void*)y, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_norm_modulate_f32in_bf16: y cannot alias x (fp32 rows in, bf16 rows out)");
    LTXMI_REQUIRE(row_width_ok(D), LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_norm_modulate_f32in_bf16: D=%d must be a multiple of 8 and <= 8192", D);
    LTXMI_REQUIRE(ldx >= D && ldx % 4 == 0 && row_stride_ok(ldy, D) && temb_ld % 8 == 0 && temb_ld >= 0, LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_norm_modulate_f32in_bf16: strides must cover D=%d and keep rows 16-byte aligned (ldx %lld, ldy %lld, "
                  "temb_ld %lld)", D, (long long)ldx, (long long)ldy, (long long)temb_ld);
    LTXMI_REQUIRE(aligned16(x, y, scale_table, scale_temb, shift_table, shift_temb),
                  LTXMI_ERR_UNSUPPORTED, "ltxmi_norm_modulate_f32in_bf16: every pointer must be 16-byte aligned");
    const int grid = (rows + ROWS_PER_WG - 1) / ROWS_PER_WG;
    hipStream_t s = (hipStream_t)stream;
    dispatch_nch<true>(D, [&](auto nch) {                    // (with the NCH = 8 instance: the 13B width, 4096)
        auto go = [&](auto layer) {
            hipLaunchKernelGGL((norm_modulate_f32in_kernel<decltype(nch)::value, decltype(layer)::value>), dim3(grid), dim3(256), 0, s,
                               x, ldx, (uint16_t*)y, ldy, rows, D, eps, (const uint16_t*)scale_table, (const uint16_t*)scale_temb,
                               (const uint16_t*)shift_table, (const uint16_t*)shift_temb, temb_ld, rows_per_group);
        };
        if (kind == LTXMI_NORM_LAYER) go(std::true_type{});
        else go(std::false_type{});
    });
    return check_launch("ltxmi_norm_modulate_f32in_bf16");
}

extern "C" int ltxmi_gate_residual_f32(float* h, int64_t ldh, const void* y, int64_t ldy, int32_t rows, int32_t D,
                                       const void* gate_table, const void* gate_temb, int64_t gate_ld,
                                       int32_t rows_per_group, int32_t round_product, void* h_bf16, int64_t ld_h_bf16,
                                       void* stream) {
    LTXMI_REQUIRE(h && y, LTXMI_ERR_INVALID_ARG, "ltxmi_gate_residual_f32: NULL argument");
    LTXMI_REQUIRE(rows > 0 && D > 0, LTXMI_ERR_INVALID_ARG, "ltxmi_gate_residual_f32: non-positive size rows=%d D=%d", rows, D);
    LTXMI_REQUIRE(gate_table == nullptr || gate_temb != nullptr, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_gate_residual_f32: a gate_table needs gate_temb");
    LTXMI_REQUIRE(gate_table == nullptr || rows_per_group > 0, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_gate_residual_f32: rows_per_group=%d must be positive", rows_per_group);
    LTXMI_REQUIRE(gate_table == nullptr || round_product == 0 || round_product == 1, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_gate_residual_f32: round_product=%d must be 0 or 1", round_product);
    LTXMI_REQUIRE((const void*)h != y && (const void*)h != (const void*)h_bf16 && y != (const void*)h_bf16, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_gate_residual_f32: h, y and h_bf16 are three different buffers");
    LTXMI_REQUIRE(row_width_ok(D), LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_gate_residual_f32: D=%d must be a multiple of 8 and <= 8192", D);
    LTXMI_REQUIRE(ldh >= D && ldh % 4 == 0 && row_stride_ok(ldy, D) && (!gate_table || (gate_ld % 8 == 0 && gate_ld >= 0)) &&
                      (!h_bf16 || row_stride_ok(ld_h_bf16, D)),
                  LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_gate_residual_f32: strides must cover D=%d and keep rows 16-byte aligned (ldh %lld, ldy %lld, gate_ld "
                  "%lld, ld_h_bf16 %lld)", D, (long long)ldh, (long long)ldy, (long long)gate_ld, (long long)ld_h_bf16);
    LTXMI_REQUIRE(aligned16(h, y, gate_table, gate_table ? gate_temb : nullptr, h_bf16),
                  LTXMI_ERR_UNSUPPORTED, "ltxmi_gate_residual_f32: every pointer must be 16-byte aligned");
    const int nchunk = D >> 3;
    const int64_t total = (int64_t)rows * nchunk;
    LTXMI_REQUIRE(total < (1ll << 31), LTXMI_ERR_UNSUPPORTED, "ltxmi_gate_residual_f32: too many elements (rows %d x D %d)", rows, D);
    const unsigned grid = (unsigned)((total + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
#define CALLG(G, R, C)                                                                                                  \
    hipLaunchKernelGGL((gate_residual_f32_kernel<G, R, C>), dim3(grid), dim3(256), 0, s, h, ldh, (const uint16_t*)y, ldy, \
                       nchunk, (uint32_t)total, (const uint16_t*)gate_table, (const uint16_t*)gate_temb, gate_ld,       \
                       rows_per_group, (uint16_t*)h_bf16, ld_h_bf16)
#define CALLC(G, R)            \
    if (h_bf16) CALLG(G, R, true); \
    else CALLG(G, R, false)
    if (!gate_table) {
        CALLC(false, false);
    } else if (round_product) {
        CALLC(true, true);
    } else {
        CALLC(true, false);
    }
#undef CALLC
#undef CALLG
    return check_launch("ltxmi_gate_residual_f32");
}
