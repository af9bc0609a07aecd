// epilogue.h -- the pieces the epilogues of gemm.hip and conv_direct.hip have in common (force-inlined device helpers).
#pragma once
#include "common.h"

namespace ltxmi {

// ---- four accumulator values (a float[4], an f32x4, a pointer to four floats) and four packed bf16 operands (8 bytes)
template <class V>
__device__ __forceinline__ void add_bf16x4(V&& v, u32x2 w) {
    v[0] += bf_lo(w[0]); v[1] += bf_hi(w[0]);
    v[2] += bf_lo(w[1]); v[3] += bf_hi(w[1]);
}
// v + a + b with the association written down.  Left to -ffast-math, hipcc picks one per kernel instance (two add_bf16x4 in a row
// came out as v + (a + b) in one instance and (v + a) + b in another of the same source): one bf16 ulp in a few values per
// million after the rounding, where the two-pair kernel owes the bits of the plain GEMM on the concatenation.
template <bool OPERANDS_FIRST, class V>
__device__ __forceinline__ void add2_bf16x4(V&& v, u32x2 a, u32x2 b) {
#pragma clang fp reassociate(off)
    if (OPERANDS_FIRST) {
        v[0] = v[0] + (bf_lo(a[0]) + bf_lo(b[0])); v[1] = v[1] + (bf_hi(a[0]) + bf_hi(b[0]));
        v[2] = v[2] + (bf_lo(a[1]) + bf_lo(b[1])); v[3] = v[3] + (bf_hi(a[1]) + bf_hi(b[1]));
    } else {
        v[0] = (v[0] + bf_lo(a[0])) + bf_lo(b[0]); v[1] = (v[1] + bf_hi(a[0])) + bf_hi(b[0]);
        v[2] = (v[2] + bf_lo(a[1])) + bf_lo(b[1]); v[3] = (v[3] + bf_hi(a[1])) + bf_hi(b[1]);
    }
}
template <class V>
__device__ __forceinline__ void mul_sum_bf16x4(V&& v, u32x2 a, u32x2 b) {      // v *= a + b
    v[0] *= bf_lo(a[0]) + bf_lo(b[0]); v[1] *= bf_hi(a[0]) + bf_hi(b[0]);
    v[2] *= bf_lo(a[1]) + bf_lo(b[1]); v[3] *= bf_hi(a[1]) + bf_hi(b[1]);
}
template <class V>
__device__ __forceinline__ u32x2 pack_bf16x4(V&& v) {
    return u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
}
// ---- the GEMMs' internal epilogues, beside the public ltxmi_epilogue values (gemm.hip, gemm_pair2.hip)
constexpr int EPI_D2S = 4;        // internal: conv + pixel-shuffle(2,2,2) scatter (+ residual)
constexpr int EPI_RESIDUAL = 5;   // internal: GATE_RESIDUAL without a gate (C = R + acc + bias)
constexpr int EPI_SUMSQ = 6;      // internal: plain store + per-(row, 64-column block) sum of squares of the stored bf16
                                  // values for the columns < sumsq_cols (the q part of a fused QKV projection: the
                                  // attention kernel turns them into q's RMSNorm factor, attention.py:1040-1041)

// s + the squares of four stored bf16 values, as ONE fixed chain of fused multiply-adds: under -ffast-math hipcc is free to
// associate "s += a*a + b*b + c*c + d*d" differently in every kernel instance, and the row sums of squares (which become
// q's RMSNorm factor) must not depend on which GEMM kernel the dispatcher picked for a given M
__device__ __forceinline__ float sumsq4(float s, u32x2 o) {
    s = __builtin_fmaf(bf_lo(o[0]), bf_lo(o[0]), s);
    s = __builtin_fmaf(bf_hi(o[0]), bf_hi(o[0]), s);
    s = __builtin_fmaf(bf_lo(o[1]), bf_lo(o[1]), s);
    s = __builtin_fmaf(bf_hi(o[1]), bf_hi(o[1]), s);
    return s;
}

// ---- a wave's 4-KB LDS scratch: 32 rows x 128 B (64 bf16 columns), 16-byte chunks XOR-swizzled by row & 7; written in the
// accumulators' layout and read row-major, or the other way round.  Both return the ADDRESS, formed term by term: hipcc folds the
// row term's constant part into the instruction's offset field only then.  The 8-byte piece of fragment column j in row row_l:
__device__ __forceinline__ char* scratch_acc_ptr(char* scr, int row_l, int j, int lane) {
    const int chunk = j * 2 + (lane >> 5);
    return scr + row_l * 128 + ((chunk ^ (row_l & 7)) << 4) + ((lane >> 4) & 1) * 8;
}
__device__ __forceinline__ char* scratch_row_ptr(char* scr, int row_l, int chunk) {      // row-major: 16-byte piece `chunk` of row row_l
    return scr + row_l * 128 + ((chunk ^ (row_l & 7)) << 4);
}

}  // namespace ltxmi
