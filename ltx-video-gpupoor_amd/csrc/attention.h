// attention.h -- what the four attention kernel files (attention.hip, attention_pipe.hip, attention_pipe128.hip,
// attention_cross.hip) have in common: the parameter block, the kernel ids, and the parts outside the key loops that could
// be shared with the generated code unchanged -- the work item, the lane layouts' constants (row-sum operand, transposed-read
// offset, V^T fragment, lane-half maximum), the launchers' tail, and for the two pipelined kernels the Q^T fragment finish on
// load, the LDS-DMA source, the range check and the redo agreement.  Every helper is force-inlined and takes as parameters
// only what differs between the kernels.  What is NOT here, because each kernel's register allocation or rounding moved with it
// ("Attention, shared parts"): the ragged-tile key mask, the epilogues, and the q finish of attention.hip and
// attention_cross.hip.  tests/test_kernel_resources.py pins registers, spills and occupancy of all four files.
#pragma once
#include "common.h"

namespace ltxmi {

struct AttnParams {
    const uint16_t* q; int64_t q_sb, q_sl;
    const uint16_t* k; int64_t k_sb, k_sl;
    const uint16_t* v; int64_t v_sb, v_sl;
    uint16_t* o; int64_t o_sb, o_sl;
    const float* bias; int64_t bias_sb;
    int B, H, Lq, Lk;
    float scale_log2e;   // softmax_scale * log2(e)
    int q_tiles;         // query tiles per (batch, head)
    // optional: q arrives as the raw projection output; RMSNorm over all H * dh channels (row sums of squares
    // given as per-64-column partials by the projection GEMM) x weight, then interleaved RoPE, applied on load
    const float* q_ss; int64_t q_ss_sb, q_ss_sl; int q_ss_n;
    // ... or, finalised (one float per row: rsqrt(mean(x^2) + eps), ltxmi_rmsnorm_rope_rstd_bf16); takes precedence
    const float* q_rstd; int64_t q_rstd_sb, q_rstd_sl;
    const uint16_t* q_w; float q_eps;
    const uint16_t* rope_cos; const uint16_t* rope_sin; int64_t rope_sb, rope_sl;
    // optional: the output's token axis is cut into segments of o_seg tokens, o_sseg elements apart (Ulysses: the
    // return all-to-all's send buffer [P dst][B][N / P][H dh]); 0 = one segment
    int o_seg; int64_t o_sseg;
    // diagnostics of the pipelined kernels' steady (reference-0) form: a device counter that every workgroup whose item had to
    // be redone in the exact form bumps once (nullptr = off), and a switch that sends EVERY item straight to the exact form
    uint32_t* redo_count; int force_exact;
    // optional second output: lse[b * lse_sb + head * lse_sh + row] = ln sum_j exp(scale q.k_j + bias_j), fp32 (nullptr = off)
    float* lse; int64_t lse_sb, lse_sh;

    __host__ __device__ __forceinline__ bool q_on_load() const { return q_ss != nullptr || q_rstd != nullptr; }
    // q's RMSNorm factor of row `row` of batch b (HD = H * head_dim, the normalised width)
    __device__ __forceinline__ float q_row_rstd(int b, int row, int HD) const {
        if (q_rstd) return q_rstd[(int64_t)b * q_rstd_sb + (int64_t)row * q_rstd_sl];
        const float* ss = q_ss + (int64_t)b * q_ss_sb + (int64_t)row * q_ss_sl;
        float s2 = 0.f;
        if ((q_ss_n & 3) == 0 && (((uintptr_t)ss) & 15) == 0) {
            // (one 16-byte load per four partials: the row's partials are contiguous)
            const f32x4* ss4 = (const f32x4*)ss;
            for (int j = 0; j < (q_ss_n >> 2); ++j) {
                const f32x4 v4 = ss4[j];
                s2 += (v4[0] + v4[1]) + (v4[2] + v4[3]);
            }
        } else {
            for (int j = 0; j < q_ss_n; ++j) s2 += ss[j];
        }
        return rsqrtf(s2 / (float)HD + q_eps);
    }

    // The row's log-sum-exp from the kernel's OWN normaliser: l = the row sum O is divided by, taken against the reference
    // m_log2 (the running / tile maximum in bits; 0 in the pipelined kernels' steady form).  removed: the maximum, in the
    // units the bias was clamped in, sits at the clamp -- every key of the row was removed and the row reports -inf.  Called inside
    // a wave-uniform `if (p.lse)` in the epilogue by the lanes that hold a row's l and m.
    __device__ __forceinline__ void store_lse(int b, int head, int row, float m_log2, float l, bool removed) const {
        constexpr float LN2 = 0.6931471805599453f;
        lse[(int64_t)b * lse_sb + (int64_t)head * lse_sh + row] = removed ? -INFINITY : (m_log2 + __log2f(l)) * LN2;
    }

    __device__ __forceinline__ int64_t o_row(int row) const {
        if (o_seg <= 0) return (int64_t)row * o_sl;
        const int sg = row / o_seg;
        return (int64_t)sg * o_sseg + (int64_t)(row - sg * o_seg) * o_sl;
    }
};

// The kernel instances behind ltxmi_attention_fwd_bf16, numbered as ltxmi_attention_kernel_id reports them (ABI: callers compare
// ids, tests pin them); attn_select (attention.hip) alone chooses among them.  attention.hip's kernel at head_dim 64 (+ key bias,
// + 64 query rows per wave) and 128 (+ key bias), the software-pipelined kernels of attention_pipe.hip (head_dim 64) and
// attention_pipe128.hip (128), and attention_cross.hip's for short key sequences (K / V resident in LDS; head_dim 64).
enum AttnKernel : int {
    ATTN_DH64 = 0, ATTN_DH64_BIAS = 1, ATTN_DH64_QB2 = 2, ATTN_PIPE = 3,
    ATTN_DH128 = 4, ATTN_DH128_BIAS = 5, ATTN_PIPE128 = 6, ATTN_CROSS = 7,
};
constexpr int ATTN_CROSS_MAX_KEYS = 256;
// key_bias contract (include/ltxmi.h): any finite value and -inf are accepted.  The bias-taking kernels clamp the bias, in the
// units they stage it in (x log2(e), or / softmax_scale), to this floor: a key at or below it is removed (P = 0 exactly), and
// -inf or an overflowing "most negative" mask never meets +inf or a zero operand as NaN.
constexpr float ATTN_BIAS_FLOOR = -1e30f;
// A row whose maximum score sits at the floor (to the 2^-16 of the short-key kernel's hi + lo bias split) has every key removed
constexpr float ATTN_ROW_REMOVED = 0.99f * ATTN_BIAS_FLOOR;

// ---- the work item ------------------------------------------------------------------------------------------------------------
// Workgroup -> (batch, head, tile) with p.q_tiles tiles per (batch, head), through the XCD-aware work id (common.h): an XCD walks
// whole (batch, head) pairs, so the CUs that share an L2 stream the same K / V at the same time.  q / k / v / o: the (batch,
// head)'s first row.
struct AttnItem {
    int b, head, tile;
    const uint16_t *q, *k, *v;
    uint16_t* o;
};
template <int DH>
__device__ __forceinline__ AttnItem attn_item(const AttnParams& p) {
    const int work = xcd_work_id();
    const int bh = work / p.q_tiles;
    AttnItem w;
    w.tile = work % p.q_tiles;
    w.b = bh / p.H;
    w.head = bh % p.H;
    w.q = p.q + (int64_t)w.b * p.q_sb + w.head * DH;
    w.k = p.k + (int64_t)w.b * p.k_sb + w.head * DH;
    w.v = p.v + (int64_t)w.b * p.v_sb + w.head * DH;
    w.o = p.o + (int64_t)w.b * p.o_sb + w.head * DH;
    return w;
}

// ---- lane layouts (lane = (r, hh): query column r = lane & 31, 4-row group hh = lane >> 5 of every 8 accumulator rows) ----------
// Q^T fragments (B operand of S^T = K Q^T): k-step s holds Q[row][16 s + 8 hh .. + 7].  q arrives as the raw projection output and
// is finished here, on load: q_norm (RMSNorm over all H * dh channels: x * rstd * weight) and the interleaved-pair RoPE on the
// flat channel axis, with the arithmetic of rmsnorm_rope_kernel (rowops.hip) -- fp32, then `post` (softmax_scale * log2(e) where
// the scores are to leave the matrix pipe in bits, 1 elsewhere), then ONE rounding to bf16.  row: the (clamped) query row the
// fragments were loaded from.  Used by the two pipelined kernels; attention.hip and attention_cross.hip keep their own copies
// (see there).
template <int DH>
__device__ __forceinline__ void attn_finish_q(const AttnParams& p, const AttnItem& w, int row, int hh, float rstd, float post,
                                              bf16x8 (&q)[DH / 16]) {
    const int64_t trow = (int64_t)w.b * p.rope_sb + (int64_t)row * p.rope_sl;
#pragma unroll
    for (int s = 0; s < DH / 16; ++s) {
        const int col = w.head * DH + 16 * s + 8 * hh;
        const bf16x8 wv = *(const bf16x8*)(p.q_w + col);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (float)q[s][e] * rstd * (float)wv[e];
        if (p.rope_cos) {
            const bf16x8 cv = *(const bf16x8*)(p.rope_cos + trow + col), sv = *(const bf16x8*)(p.rope_sin + trow + col);
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const float r0 = o[e] * (float)cv[e] - o[e + 1] * (float)sv[e];
                const float r1 = o[e + 1] * (float)cv[e + 1] + o[e] * (float)sv[e + 1];
                o[e] = r0;
                o[e + 1] = r1;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) q[s][e] = (__bf16)(o[e] * post);
    }
}

// Row sums on the matrix pipe: the P^T fragment of the 32x32x16 PV product, re-read as the B operand of a 16x16x32 MFMA, puts
// query (lane & 15) [+16 for odd 16-lane groups] on the column and the lane's 8 keys in k-group (lane >> 4).  With A = 1 on
// (row 0, even k-groups) and (row 1, odd k-groups), D[0][n] = the sum over the keys of P[query n] and D[1][n] = the same for
// query n + 16: lanes 0..15 hold them in registers 0 and 1.  This is that A operand.
__device__ __forceinline__ bf16x8 attn_ones_operand(int lane) {
    const bool on = ((lane & 15) == 0 && ((lane >> 4) & 1) == 0) || ((lane & 15) == 1 && ((lane >> 4) & 1) == 1);
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = on ? (__bf16)1.0f : (__bf16)0.0f;
    return ones;
}

// V image: [8 key][32 col] sub-tiles of 512 B, sub-tile (key >> 3) * (DH / 32) + (col >> 5).  V^T (A operand of O^T += V^T P^T)
// comes from it by transposed reads; the lane's byte offset inside a sub-tile ...
__device__ __forceinline__ int attn_vt_offset(int lane) {
    const int g16 = lane >> 4, i16 = lane & 15;
    return (4 * (g16 >> 1) + (i16 >> 2)) * 64 + (16 * (g16 & 1) + 4 * (i16 & 3)) * 2;
}
// ... and one fragment (16 keys x 32 columns): at = the lane's address in the sub-tile of the fragment's first 8 keys
template <int DH>
__device__ __forceinline__ bf16x8 attn_vt_fragment(const char* at) {
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(at));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(at + (DH / 32) * 512));
    const s16x8 both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, both);
}

// A query's keys are split over the lane halves (lane, lane ^ 32): the maximum over both
__device__ __forceinline__ float attn_lane_half_max(float m) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}

// ---- the pipelined kernels' K / V stream and redo ---------------------------------------------------------------------------
// LDS-DMA source: one buffer descriptor per operand, base = the (batch, head)'s first row, num_records = up to the end of its
// last row (stride `sl` elements): key rows past Lk are out of range and arrive as zeros.
template <int DH>
__device__ __forceinline__ u32x4 attn_kv_desc(const void* base, int Lk, int64_t sl) {
    const uint64_t a = (uint64_t)base;
    const int64_t bytes = ((int64_t)(Lk - 1) * sl + DH) * 2;
    return u32x4{(uint32_t)a, (uint32_t)(a >> 32) & 0xffffu, (uint32_t)bytes, 0x00020000u};
}
// One LDS-DMA piece (1 KiB per wave: 16 bytes per lane from byte offset voff, to the LDS byte address lds_addr through M0).
// Issued from inline asm: for a builtin LDS-DMA hipcc puts s_waitcnt vmcnt(0) in front of the next transposed LDS read (it
// cannot tell the slots apart), which would drain the ring every segment.  Completion is counted by hand instead (a counted
// vmcnt at the end of an iteration, then the barrier).
__device__ __forceinline__ void attn_lds_dma(const u32x4& desc, uint32_t lds_addr, uint32_t voff) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %1, %3, 0 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(lds_addr), "s"(desc)
        : "memory");
}
// The steady form's range check (P against a fixed reference): a row sum or an accumulator of magnitude >= 2^100 (or inf / NaN:
// the test is on the exponent bits, the files are built with -fno-honor-nans) = a score too large for the reference (not only
// overflow: 1 / l for l > 2^126 is a denormal and flushes to zero; a legitimate l is at most (keys) x 2^(a few bits));
// VANISH: also a row sum below 2^-100 (or 0) = a row whose scores all underflowed.  Returns worst | (non-zero = out of range).
template <bool VANISH, int ND>
__device__ __forceinline__ uint32_t attn_out_of_range(uint32_t worst, const f32x4& l, const f32x16 (&o)[ND], int lane) {
    constexpr uint32_t OUTGROWN_EXP = (127u + 100u) << 23, VANISHED_EXP = (127u - 100u) << 23;
    worst |= (uint32_t)((__float_as_uint(l[0]) & 0x7f800000u) >= OUTGROWN_EXP);
    worst |= (uint32_t)((__float_as_uint(l[1]) & 0x7f800000u) >= OUTGROWN_EXP);
    // (the row sums live in lanes 0..15, registers 0 / 1; a sum of 0 has exponent bits 0)
    if (VANISH && lane < 16) {
        worst |= (uint32_t)((__float_as_uint(l[0]) & 0x7f800000u) < VANISHED_EXP);
        worst |= (uint32_t)((__float_as_uint(l[1]) & 0x7f800000u) < VANISHED_EXP);
    }
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) worst |= (uint32_t)((__float_as_uint(o[d][e]) & 0x7f800000u) >= OUTGROWN_EXP);
    return worst;
}
// The workgroup agrees on the redo through one LDS word (zeroed before the item): non-zero if any wave asked for it
__device__ __forceinline__ int attn_agree_redo(volatile int* redo_flag, bool outgrown, int lane) {
    if (outgrown && lane == 0) *redo_flag = 1;
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    const int redo = *redo_flag;
    __builtin_amdgcn_s_barrier();
    return redo;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// The launchers' tail: `tiles` workgroups of 256 threads per (batch, head) (the kernels find it in p.q_tiles), lds bytes of
// dynamic LDS (reserved once per device: lds_done is the kernel's own mask), extra = further kernel arguments.
template <typename Kern, typename... Extra>
static inline int attn_launch(Kern kern, int lds, unsigned long long* lds_done, AttnParams p, int tiles, hipStream_t stream,
                              Extra... extra) {
    if (const int rc = reserve_lds((const void*)kern, lds, lds_done, "ltxmi_attention_fwd_bf16")) return rc;
    p.q_tiles = tiles;
    const int64_t grid = (int64_t)p.B * p.H * tiles;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, stream, p, extra...);
    return check_launch("ltxmi_attention_fwd_bf16");
}

// Launchers of the kernels in the other attention files: each runs the shape it is given (attn_select has chosen it)
int launch_attn_pipe(AttnParams p, hipStream_t stream);
int launch_attn_pipe128(AttnParams p, hipStream_t stream);
int launch_attn_cross(AttnParams p, hipStream_t stream);

}  // namespace ltxmi
