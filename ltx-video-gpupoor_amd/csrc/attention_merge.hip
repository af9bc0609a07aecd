// attention_merge.hip -- n-way merge of partial attention results over disjoint key sets (ltxmi_attention_merge_bf16).
//
// Ring sequence parallelism leaves every rank with P partial results (O_i, lse_i) for its own queries, one per K/V shard that
// came round (xdit_context_parallel.py:179-184 of the reference -> xFuserLongContextAttention, whose ring updates out / lse
// pairwise after every step).  With lse_i the normaliser O_i was divided by,
//     m = max_i lse_i,  w_i = exp(lse_i - m),  O = sum_i w_i O_i / sum_i w_i,  lse = m + ln sum_i w_i
// is the softmax over the union of the key sets.  All n partials in ONE launch: the result is rounded to bf16 once, not once
// per ring step.
//
// A pure streaming kernel: (n + 1) x 2 bytes per output element, 16-byte loads and stores, no reuse.  One workgroup owns
// MERGE_TOK consecutive tokens of a batch row with all their heads (in groups of at most MERGE_HG heads): the lse tensors are
// [B, H, Lq], so the tokens of one (partial, head) are MERGE_TOK contiguous floats, read once into LDS and turned into
// normalised weights there; then the O rows stream through, consecutive lanes on consecutive 16-byte chunks of a token's row.
// A partial whose weight is exactly 0 (lse_i = -inf: every key of its shard removed, its O undefined -- NaN included -- or so
// far below the maximum that exp underflows) is skipped by selection: its O is not even loaded.
#include "common.h"

namespace ltxmi {

namespace merge {

constexpr int MAX_N = 8;
constexpr int MERGE_TOK = 16;       // tokens per workgroup: 64-byte runs of lse per (partial, head)
constexpr int MERGE_HG = 64;        // heads per workgroup: n x 64 x 16 floats of LDS = 32 KiB at n = 8
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

struct MergeParams {
    const uint16_t* o_part[MAX_N]; int64_t op_sb[MAX_N], op_sl[MAX_N];
    const float* lse_part[MAX_N]; int64_t lp_sb[MAX_N], lp_sh[MAX_N];
    uint16_t* o; int64_t o_sb, o_sl;
    float* lse; int64_t lse_sb, lse_sh;
    int n, B, H, Lq, dh;
};

__global__ __launch_bounds__(256) void attn_merge_kernel(MergeParams p) {
    extern __shared__ __attribute__((aligned(16))) float w_lds[];       // [n][hg][MERGE_TOK]
    const int tid = threadIdx.x;
    const int l0 = blockIdx.x * MERGE_TOK, h0 = blockIdx.y * MERGE_HG, b = blockIdx.z;
    const int hg = min(MERGE_HG, p.H - h0);
    const int cells = hg * MERGE_TOK;                                   // (head, token) pairs of this workgroup

    // ---- lse_i -> LDS (token fastest: coalesced 64-byte runs); tokens past Lq read nothing and are never used
    for (int idx = tid; idx < p.n * cells; idx += 256) {
        const int i = idx / cells, cell = idx - i * cells;
        const int h = cell / MERGE_TOK, t = cell % MERGE_TOK;
        float v = -INFINITY;
        // (p.lse_part[i] with a run-time i: picked by a chain of selects over the kernel arguments, no scratch)
        const float* src = nullptr; int64_t sb = 0, sh = 0;
#pragma unroll
        for (int j = 0; j < MAX_N; ++j)
            if (j == i) { src = p.lse_part[j]; sb = p.lp_sb[j]; sh = p.lp_sh[j]; }
        if (l0 + t < p.Lq) v = src[(int64_t)b * sb + (int64_t)(h0 + h) * sh + l0 + t];
        w_lds[idx] = v;
    }
    __syncthreads();
    // ---- per (head, token): weights normalised by their sum, merged lse
    for (int cell = tid; cell < cells; cell += 256) {
        float m = -INFINITY;
        for (int i = 0; i < p.n; ++i) m = fmaxf(m, w_lds[i * cells + cell]);
        float sum = 0.f;
        float w[MAX_N];
#pragma unroll
        for (int i = 0; i < MAX_N; ++i) {
            // (m = -inf: every partial empty; lse_i - m would be NaN)
            w[i] = (i < p.n && m > -INFINITY) ? fast_exp2((w_lds[i * cells + cell] - m) * LOG2E) : 0.f;
            sum += w[i];
        }
        const float inv = sum > 0.f ? 1.0f / sum : 0.f;
#pragma unroll
        for (int i = 0; i < MAX_N; ++i)
            if (i < p.n) w_lds[i * cells + cell] = w[i] * inv;
        const int h = cell / MERGE_TOK, t = cell % MERGE_TOK;
        if (p.lse != nullptr && l0 + t < p.Lq)
            p.lse[(int64_t)b * p.lse_sb + (int64_t)(h0 + h) * p.lse_sh + l0 + t] = sum > 0.f ? m + __log2f(sum) * LN2 : -INFINITY;
    }
    __syncthreads();
    // ---- O rows: chunk = 8 channels = 16 bytes; up to n independent 16-byte loads in flight per lane
    const int cpr = hg * p.dh / 8;                                      // chunks per token row (of this head group)
    const int cph = p.dh / 8;                                           // chunks per head
    const int tok = min(MERGE_TOK, p.Lq - l0);
    for (int idx = tid; idx < tok * cpr; idx += 256) {
        const int t = idx / cpr, ch = idx - t * cpr;
        const int cell = (ch / cph) * MERGE_TOK + t;
        const int64_t col = (int64_t)h0 * p.dh + ch * 8;
        float w[MAX_N];
        u32x4 v[MAX_N];
#pragma unroll
        for (int i = 0; i < MAX_N; ++i) {
            w[i] = i < p.n ? w_lds[i * cells + cell] : 0.f;
            if (w[i] != 0.f) v[i] = *(const u32x4*)(p.o_part[i] + (int64_t)b * p.op_sb[i] + (int64_t)(l0 + t) * p.op_sl[i] + col);
        }
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < MAX_N; ++i)
            if (w[i] != 0.f) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[2 * e] = __builtin_fmaf(w[i], bf_lo(v[i][e]), acc[2 * e]);
                    acc[2 * e + 1] = __builtin_fmaf(w[i], bf_hi(v[i][e]), acc[2 * e + 1]);
                }
            }
        u32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = pack_bf16(acc[2 * e], acc[2 * e + 1]);
        *(u32x4*)(p.o + (int64_t)b * p.o_sb + (int64_t)(l0 + t) * p.o_sl + col) = out;
    }
}

}  // namespace merge

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_attention_merge_bf16(const ltxmi_attn_merge_args* a, void* stream) {
    LTXMI_REQUIRE(a != nullptr, LTXMI_ERR_INVALID_ARG, "ltxmi_attention_merge_bf16: NULL argument");
    LTXMI_REQUIRE(a->n >= 2 && a->n <= LTXMI_ATTN_MERGE_MAX, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_attention_merge_bf16: n = %d partials, not in 2 .. %d", a->n, LTXMI_ATTN_MERGE_MAX);
    LTXMI_REQUIRE(a->B > 0 && a->H > 0 && a->Lq > 0 && a->head_dim > 0, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_attention_merge_bf16: non-positive shape B=%d H=%d Lq=%d head_dim=%d", a->B, a->H, a->Lq, a->head_dim);
    LTXMI_REQUIRE(a->o != nullptr, LTXMI_ERR_INVALID_ARG, "ltxmi_attention_merge_bf16: NULL output");
    LTXMI_REQUIRE(a->head_dim % 8 == 0, LTXMI_ERR_UNSUPPORTED, "ltxmi_attention_merge_bf16: head_dim %d is not a multiple of 8", a->head_dim);
    LTXMI_REQUIRE(a->B <= 65535 && (a->H + merge::MERGE_HG - 1) / merge::MERGE_HG <= 65535, LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_attention_merge_bf16: grid too large");
    merge::MergeParams p = {};
    const int64_t row = (int64_t)a->H * a->head_dim;
    for (int i = 0; i < a->n; ++i) {
        LTXMI_REQUIRE(a->o_part[i] != nullptr && a->lse_part[i] != nullptr, LTXMI_ERR_INVALID_ARG,
                      "ltxmi_attention_merge_bf16: partial %d is NULL", i);
        LTXMI_REQUIRE((((uintptr_t)a->lse_part[i]) & 3) == 0 && a->lse_part_stride_h[i] >= a->Lq &&
                          (a->B == 1 ? a->lse_part_stride_b[i] >= 0 : a->lse_part_stride_b[i] >= (int64_t)a->H * a->lse_part_stride_h[i]),
                      LTXMI_ERR_INVALID_ARG, "ltxmi_attention_merge_bf16: lse of partial %d: must be 4-byte aligned, strides [B, H, Lq]", i);
        LTXMI_REQUIRE((((uintptr_t)a->o_part[i]) & 15) == 0 && a->o_part_stride_b[i] % 8 == 0 && a->o_part_stride_l[i] % 8 == 0 &&
                          a->o_part_stride_l[i] >= row,
                      LTXMI_ERR_UNSUPPORTED, "ltxmi_attention_merge_bf16: o of partial %d: 16-byte aligned rows of H * head_dim", i);
        p.o_part[i] = (const uint16_t*)a->o_part[i]; p.op_sb[i] = a->o_part_stride_b[i]; p.op_sl[i] = a->o_part_stride_l[i];
        p.lse_part[i] = a->lse_part[i]; p.lp_sb[i] = a->lse_part_stride_b[i]; p.lp_sh[i] = a->lse_part_stride_h[i];
    }
    if (a->lse)
        LTXMI_REQUIRE((((uintptr_t)a->lse) & 3) == 0 && a->lse_stride_h >= a->Lq &&
                          (a->B == 1 ? a->lse_stride_b >= 0 : a->lse_stride_b >= (int64_t)a->H * a->lse_stride_h),
                      LTXMI_ERR_INVALID_ARG, "ltxmi_attention_merge_bf16: merged lse must be 4-byte aligned, strides [B, H, Lq]");
    LTXMI_REQUIRE((((uintptr_t)a->o) & 15) == 0 && a->o_stride_b % 8 == 0 && a->o_stride_l % 8 == 0 && a->o_stride_l >= row,
                  LTXMI_ERR_UNSUPPORTED, "ltxmi_attention_merge_bf16: o: 16-byte aligned rows of H * head_dim");
    p.o = (uint16_t*)a->o; p.o_sb = a->o_stride_b; p.o_sl = a->o_stride_l;
    p.lse = a->lse; p.lse_sb = a->lse_stride_b; p.lse_sh = a->lse_stride_h;
    p.n = a->n; p.B = a->B; p.H = a->H; p.Lq = a->Lq; p.dh = a->head_dim;
    const int hg = a->H < merge::MERGE_HG ? a->H : merge::MERGE_HG;
    const size_t lds = (size_t)a->n * hg * merge::MERGE_TOK * sizeof(float);
    const dim3 grid((unsigned)((a->Lq + merge::MERGE_TOK - 1) / merge::MERGE_TOK), (unsigned)((a->H + merge::MERGE_HG - 1) / merge::MERGE_HG),
                    (unsigned)a->B);
    hipLaunchKernelGGL(merge::attn_merge_kernel, grid, dim3(256), lds, (hipStream_t)stream, p);
    return check_launch("ltxmi_attention_merge_bf16");
}
