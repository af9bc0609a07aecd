// norm_mx8.hip -- ltxmi_norm_modulate_mx8 (include/ltxmi_mx_attn.h): norm + AdaLN modulate whose output row leaves as MX-FP8.
// norm_modulate_kernel of rowops.hip up to the bf16 rounding of a chunk, then the chunk step of quantize_mx8_kernel
// (quant_mx8.hip) on those bf16 bits in registers: both kernels give lane l the 8-element chunks l, l + 64, ..., so the four
// lanes that own a 32-element block are neighbours here as there.  The normalised bf16 row is never written or read back:
// traffic is one read of the stream and a quarter of its bytes + the scales written.
#include "mx8.h"
#include "rows.h"
#include "../../include/ltxmi_mx_attn.h"

namespace ltxmi {

// load_bf16x8's widening of the 16 bytes it read
__device__ __forceinline__ Chunk widen(u32x4 w) {
    Chunk c;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c.v[2 * i] = bf_lo(w[i]);
        c.v[2 * i + 1] = bf_hi(w[i]);
    }
    return c;
}

// the same, of words the compiler is not to know: it would otherwise widen a row once and keep the fp32 copy beside the words
// across the reductions (the NCH = 16 layer-norm instance: 256 registers and accumulation registers on top).  Only where a row
// is that long: the NCH = 4 layer-norm instance comes out with 84 registers for 70 this way.
template <bool OPAQUE>
__device__ __forceinline__ Chunk widen_again(u32x4& w) {
    if (OPAQUE) asm volatile("" : "+v"(w));
    return widen(w);
}

template <int NCH, bool LAYER>
__global__ __launch_bounds__(256) void norm_modulate_mx8_kernel(
    const uint16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ q, int64_t ldq, uint8_t* __restrict__ sc, int64_t lds,
    int rows, int D, float eps, const uint16_t* __restrict__ sc_tab, const uint16_t* __restrict__ sc_temb,
    const uint16_t* __restrict__ sh_tab, const uint16_t* __restrict__ sh_temb, int64_t temb_ld, int rows_per_group) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nchunk = D >> 3;             // a multiple of 4: the four lanes of a block are in a chunk step together
    const uint16_t* xr = x + (int64_t)row * ldx;
    // the row stays in registers as the bf16 words it was read as, 4 registers a chunk, and is widened (exactly) where it is used:
    // held as fp32 as norm_modulate_kernel holds it, the NCH = 4 instances took 80 registers, 6 waves per SIMD for that kernel's 7
    u32x4 w[NCH];
    float s1 = 0.f, s2 = 0.f;
    LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
        w[j] = *(const u32x4*)(xr + ch * 8);
        const Chunk c = widen(w[j]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (LAYER) s1 += c.v[e];
            else s2 += c.v[e] * c.v[e];
        }
    }
    float mean = 0.f;
    if (LAYER) {                           // variance about the mean, as norm_modulate_kernel<LAYER>
        mean = wave_sum(s1) / D;
        s2 = 0.f;
        LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
            const Chunk c = widen_again<(NCH > 4)>(w[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = c.v[e] - mean;
                s2 += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(s2) / D + eps);
    const int64_t g = (int64_t)(row / rows_per_group) * temb_ld;
    // the bf16 words norm_modulate_kernel stores, for the whole row, in place of the input's
    LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
        const Chunk a = load_bf16x8(sc_tab + ch * 8), a2 = load_bf16x8(sc_temb + g + ch * 8);
        const Chunk b = load_bf16x8(sh_tab + ch * 8), b2 = load_bf16x8(sh_temb + g + ch * 8);
        const Chunk c = widen_again<(NCH > 4)>(w[j]);
        Chunk o;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            o.v[e] = (c.v[e] - mean) * rstd * (1.0f + a.v[e] + a2.v[e]) + (b.v[e] + b2.v[e]);
#pragma unroll
        for (int i = 0; i < 4; ++i) w[j][i] = pack_bf16(o.v[2 * i], o.v[2 * i + 1]);
    }
    // quantize_mx8_kernel's chunk step on them
    uint8_t* qr = q + (int64_t)row * ldq;
    uint8_t* sr = sc + (int64_t)row * lds;
    LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
        uint32_t am = 0;                   // |y| as bf16 bits: their integer order is the values' order
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            am = max(am, w[j][i] & 0x7fffu);
            am = max(am, (w[j][i] >> 16) & 0x7fffu);
        }
        am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
        am = max(am, (uint32_t)__shfl_xor((int)am, 2, 64));
        const int byte = mx8_scale_byte(am << 16);
        const float inv = mx8_inv_scale(byte);
        u32x2 o8;
        o8[0] = mx8_pack4(bf_lo(w[j][0]), bf_hi(w[j][0]), bf_lo(w[j][1]), bf_hi(w[j][1]), inv);
        o8[1] = mx8_pack4(bf_lo(w[j][2]), bf_hi(w[j][2]), bf_lo(w[j][3]), bf_hi(w[j][3]), inv);
        *(u32x2*)(qr + ch * 8) = o8;
        if ((lane & 3) == 0) sr[ch >> 2] = (uint8_t)byte;
    }
}

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_norm_modulate_mx8(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int32_t rows,
                                       int32_t D, float eps, int32_t kind, const void* scale_table, const void* scale_temb,
                                       const void* shift_table, const void* shift_temb, int64_t temb_ld, int32_t rows_per_group,
                                       void* stream) {
    const char* what = "ltxmi_norm_modulate_mx8";
    LTXMI_REQUIRE(x && q && scales && scale_table && scale_temb && shift_table && shift_temb, LTXMI_ERR_INVALID_ARG,
                  "%s: NULL argument", what);
    LTXMI_REQUIRE(rows > 0 && D > 0 && rows_per_group > 0, LTXMI_ERR_INVALID_ARG, "%s: non-positive size rows=%d D=%d rows_per_group=%d",
                  what, rows, D, rows_per_group);
    LTXMI_REQUIRE(kind == LTXMI_NORM_RMS || kind == LTXMI_NORM_LAYER, LTXMI_ERR_INVALID_ARG, "%s: bad kind %d", what, kind);
    LTXMI_REQUIRE(D % LTXMI_MX_BLOCK == 0 && D <= 8192, LTXMI_ERR_UNSUPPORTED, "%s: D=%d must be a multiple of 32 and <= 8192", what, D);
    LTXMI_REQUIRE(row_stride_ok(ldx, D) && temb_ld % 8 == 0 && ldq % 16 == 0 && ldq >= D && lds >= D / LTXMI_MX_BLOCK,
                  LTXMI_ERR_UNSUPPORTED, "%s: ldx, temb_ld %% 8, ldq %% 16 and every stride >= its row (ldx=%lld ldq=%lld lds=%lld temb_ld=%lld D=%d)",
                  what, (long long)ldx, (long long)ldq, (long long)lds, (long long)temb_ld, D);
    LTXMI_REQUIRE(aligned16(x, q), LTXMI_ERR_UNSUPPORTED, "%s: x and q must be 16-byte aligned", what);
    const int64_t grid = ((int64_t)rows + ROWS_PER_WG - 1) / ROWS_PER_WG;
    hipStream_t s = (hipStream_t)stream;
    dispatch_nch<false>(D, [&](auto nch) {
        auto go = [&](auto layer) {
            hipLaunchKernelGGL((norm_modulate_mx8_kernel<decltype(nch)::value, decltype(layer)::value>), dim3((unsigned)grid), dim3(256), 0, s,
                               (const uint16_t*)x, ldx, (uint8_t*)q, ldq, (uint8_t*)scales, lds, rows, D, eps,
                               (const uint16_t*)scale_table, (const uint16_t*)scale_temb, (const uint16_t*)shift_table,
                               (const uint16_t*)shift_temb, temb_ld, rows_per_group);
        };
        if (kind == LTXMI_NORM_LAYER) go(std::true_type{});
        else go(std::false_type{});
    });
    return check_launch(what);
}
