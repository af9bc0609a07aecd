// attention.h -- parameter block shared by the attention kernels (attention.hip, attention_pipe.hip).
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

// Launchers of the kernels in the other attention files: each runs the shape it is given (attn_select has chosen it)
int launch_attn_pipe(AttnParams p, hipStream_t stream);
int launch_attn_pipe128(AttnParams p, hipStream_t stream);
int launch_attn_cross(AttnParams p, hipStream_t stream);

}  // namespace ltxmi
