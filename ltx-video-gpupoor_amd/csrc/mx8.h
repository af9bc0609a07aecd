// mx8.h -- the MX-FP8 number format (include/ltxmi_mx.h) as device code: a block's E8M0 byte from its amax, and four fp32
// values to four e4m3 bytes.  Shared by quant_mx8.hip (bf16 rows) and the MX-output epilogue of gemm_mx8.hip (fp32 accumulators).
#pragma once
#include "common.h"
#include "../../include/ltxmi_mx.h"

namespace ltxmi {

// amax >= 0 as fp32 bits -> the scale byte e + 127.  amax = m * 2^k: e = k - 8 if m <= 1.75 else k - 7, clamped at -127 (e never
// reaches +127: k <= 127).  With E = k + 127 the exponent field that is max(E - 8 + (mantissa > 0.75), 0); a zero or subnormal
// amax (E = 0; any bf16 or fp32 subnormal has k <= -127, so its e is far below the clamp) comes out as byte 0 by the same line.
__device__ __forceinline__ int mx8_scale_byte(uint32_t amax_bits) {
    const int e = (int)(amax_bits >> 23) - 8 + ((amax_bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    return e > 0 ? e : 0;
}
// 2^-e for a scale byte: exponent field 254 - byte, in [7, 254] for the bytes mx8_scale_byte returns (<= 248)
__device__ __forceinline__ float mx8_inv_scale(int byte) { return __uint_as_float((uint32_t)(254 - byte) << 23); }

// RNE to OCP e4m3fn, saturating at +-448 (the scale rule keeps every value inside; the clamp is the format's own guard)
__device__ __forceinline__ uint32_t mx8_pack4(float a, float b, float c, float d, float inv) {
    auto sat = [](float v) { return __builtin_fminf(__builtin_fmaxf(v, -448.f), 448.f); };
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(sat(a * inv), sat(b * inv), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(sat(c * inv), sat(d * inv), w, true);
    return (uint32_t)w;
}

}  // namespace ltxmi
