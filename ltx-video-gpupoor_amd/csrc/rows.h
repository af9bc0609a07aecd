// rows.h -- what the "one wave per row" kernels of rowops.hip, stream32.hip and t5.hip have in common: the 8-channel chunk a lane
// owns with its loads and stores, the walk over a lane's chunks of a row, the D -> chunks-per-lane choice, and the predicates
// their entry points check arguments with.
//
// NO floating-point arithmetic lives here: the three files compile theirs under different rules (rowops.hip plain -ffast-math,
// stream32.hip wholly and t5.hip in two functions under `#pragma clang fp reassociate(off) contract(off)`), so sums, products
// and modulations stay in kernels and lambdas written in the .hip file.  Widening bf16 to fp32 by a shift and pack_bf16 are the
// only conversions below.
#pragma once
#include <type_traits>

#include "common.h"

namespace ltxmi {

constexpr int ROWS_PER_WG = 4;  // 4 waves, one row each

// 8 consecutive channels of a row: 16 bytes of a bf16 operand, 32 bytes (two 16-byte accesses) of an fp32 one
struct Chunk {
    float v[8];
};
__device__ __forceinline__ Chunk load_bf16x8(const uint16_t* p) {
    const u32x4 w = *(const u32x4*)p;
    Chunk c;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c.v[2 * i] = bf_lo(w[i]);
        c.v[2 * i + 1] = bf_hi(w[i]);
    }
    return c;
}
__device__ __forceinline__ void store_bf16x8(uint16_t* p, const Chunk& c) {
    u32x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = pack_bf16(c.v[2 * i], c.v[2 * i + 1]);
    *(u32x4*)p = w;
}
__device__ __forceinline__ Chunk load_f32x8(const float* p) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
    Chunk c;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c.v[i] = a[i];
        c.v[4 + i] = b[i];
    }
    return c;
}
__device__ __forceinline__ void store_f32x8(float* p, const Chunk& c) {
    *(f32x4*)p = f32x4{c.v[0], c.v[1], c.v[2], c.v[3]};
    *(f32x4*)(p + 4) = f32x4{c.v[4], c.v[5], c.v[6], c.v[7]};
}

// A lane's chunks of a row of nchunk chunks: lane l takes chunks l, l + 64, ... (1 KiB coalesced per wave-instruction), NCH of
// them at the most.  A loop header: the block that follows runs with the register slot J and the chunk index CH, and not for
// a chunk past the row's end.
// (A header and not a function taking a lambda: for_row_chunks<NCH>(lane, nchunk, [&](int j, int ch) {...}), force-inlined or
// not, keeps every captured local in memory through the early passes, and 27 of the 47 row instances then came out with other
// address arithmetic, other vectorisation of the sums and up to 8 % more instructions -- tools/codegen_diff.py.  Spelled
// this way the kernels compile to what they compiled to with the loop written out.)
// The header ends in an `if`: follow it with a braced block and no `else` (an else would bind to that hidden if).
#define LTXMI_FOR_ROW_CHUNKS(NCH, LANE, NCHUNK, J, CH) \
    _Pragma("unroll") for (int J = 0; J < (NCH); ++J)  \
        if (const int CH = (LANE) + 64 * J; CH < (NCHUNK))

// D -> chunks per lane, as a tag: f(std::integral_constant<int, NCH>).  1 / 4 / 16 cover D <= 512 / 2048 / 8192; WITH8 adds
// 8 for D <= 4096 (the 13B width and T5-XXL's d_model: the row in 64 registers per lane instead of 128).  A per-call choice:
// a kernel gets the NCH = 8 instance only where its entry point asks for it.
template <bool WITH8, class F>
static inline void dispatch_nch(int D, F&& f) {
    if (D <= 512) f(std::integral_constant<int, 1>{});
    else if (D <= 2048) f(std::integral_constant<int, 4>{});
    else if (WITH8 && D <= 4096) {
        if constexpr (WITH8) f(std::integral_constant<int, 8>{});
    } else f(std::integral_constant<int, 16>{});
}

// ---- the entry points' argument checks (each keeps its own error text)
static inline bool row_width_ok(int D) { return D % 8 == 0 && D <= 8192; }                       // whole chunks, NCH <= 16
static inline bool row_stride_ok(int64_t ld, int D) { return ld % 8 == 0 && ld >= D; }            // bf16 rows: covers D, 16-byte rows
template <class... P>
static inline bool aligned16(const P*... p) { return ((((uintptr_t)p) | ... | (uintptr_t)0) & 15) == 0; }

}  // namespace ltxmi
