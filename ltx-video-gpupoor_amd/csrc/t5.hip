// t5.hip -- the four kernels the T5-v1.1 text encoder needs beside the GEMM (ltxmi/t5.py):
//   * attention with an additive bias per (head, key - query) and the textbook max-subtracted softmax,
//   * the out-of-place weighted RMSNorm that rounds where T5LayerNorm rounds,
//   * the gated tanh-GELU of DenseGatedActDense over one stacked [wi_0; wi_1] projection,
//   * the embedding gather.
// The arithmetic restated is the eager bf16 forward of Hugging Face transformers' modeling_t5.py, which the reference pipeline
// calls at pipeline_ltx_video.py:405-417 and :449-461.
//
// Attention.  The problem is small (B x H of about 128 pairs, L <= 512) and the logits are unscaled: they reach hundreds, so the
// fixed-reference-0 form of the pipelined kernels is out and a row's maximum has to be known before its first exponential.  With
// at most 512 keys a query's whole score row fits in registers, so the softmax is the single-pass textbook one -- maximum, exp2,
// sum -- with no running maximum and no rescale.  One workgroup of four waves per (batch, head, 64-query tile), 16 queries per
// wave:
//   * K ([key][64], rows padded to 144 B) and V^T ([64][keys + 8]) of the (batch, head) are staged in LDS once, with the key bias
//     and the Lk + 63 relative-bias values the tile can meet; one barrier, none afterwards;
//   * S^T = K Q^T on mfma_f32_16x16x32_bf16: the query sits on the lane (lane & 15), 4 keys of every 16-key tile in the lane's
//     registers, so P^T goes from the accumulator registers straight into the B operand of O^T += V^T P^T (two 16-key tiles make
//     one 32-deep step; V^T's fragment takes the same key order by two 8-byte LDS reads);
//   * x = scale * s + rel[key - query] + key_bias[key] in fp32; a key at or below -1e30 (or past Lk) is -inf and gets P = 0;
//   * the row sum is taken over the bf16-rounded P, the values the matrix pipe multiplies, and O = O^T / l is rounded once.
// NT = ceil(Lk / 32) rounded up to a power of two is a template parameter (1, 2, 4, 8, 16): every register index is static.
#include "rows.h"

namespace ltxmi {

namespace t5 {

constexpr int DH = 64;
constexpr int Q_TILE = 64;                  // queries per workgroup: 4 waves x 16
constexpr int K_ROW = 144;                  // bytes per key row of the K image: 128 + 16, ds_read_b128 without bank conflicts
constexpr float LOG2E = 1.4426950408889634f;
constexpr float KEY_REMOVED = -1e30f;       // include/ltxmi.h: a key bias at or below this removes the key

struct RelBiasParams {
    const uint16_t* q; int64_t q_sb, q_sl;
    const uint16_t* k; int64_t k_sb, k_sl;
    const uint16_t* v; int64_t v_sb, v_sl;
    uint16_t* o; int64_t o_sb, o_sl;
    const float* key_bias; int64_t bias_sb;
    const float* rel; int64_t rel_sh; int rel_center;
    int B, H, Lq, Lk, q_tiles;
    float scale;
};

__host__ __device__ constexpr int vt_row_bytes(int NT) { return (32 * NT + 8) * 2; }      // V^T row: the keys + 8 of padding
__host__ __device__ constexpr int k_off(int) { return 0; }
__host__ __device__ constexpr int vt_off(int NT) { return 32 * NT * K_ROW; }
__host__ __device__ constexpr int kb_off(int NT) { return vt_off(NT) + DH * vt_row_bytes(NT); }
__host__ __device__ constexpr int rb_off(int NT) { return kb_off(NT) + 32 * NT * 4; }
__host__ __device__ constexpr int smem_bytes(int NT) { return rb_off(NT) + (32 * NT + Q_TILE) * 4; }

template <int NT>
__global__ __launch_bounds__(256) void attn_relbias_kernel(RelBiasParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int LKP = 32 * NT;            // keys the instance walks; those past Lk are masked
    constexpr int VT_ROW = vt_row_bytes(NT);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;

    const int work = xcd_work_id();
    const int bh = work / p.q_tiles, tile = work % p.q_tiles;
    const int b = bh / p.H, head = bh % p.H;
    const int q0 = tile * Q_TILE;
    const uint16_t* qb = p.q + (int64_t)b * p.q_sb + head * DH;
    const uint16_t* kb = p.k + (int64_t)b * p.k_sb + head * DH;
    const uint16_t* vb = p.v + (int64_t)b * p.v_sb + head * DH;
    uint16_t* ob = p.o + (int64_t)b * p.o_sb + head * DH;

    // ---- stage K, V^T and the two bias vectors.  Keys past Lk re-read the last key (finite data) and are removed by their bias.
    for (int c = tid; c < LKP * 8; c += 256) {
        const int key = c >> 3, dc = c & 7;
        const int src = key < p.Lk ? key : p.Lk - 1;
        *(u32x4*)(smem + k_off(NT) + key * K_ROW + dc * 16) = *(const u32x4*)(kb + (int64_t)src * p.k_sl + dc * 8);
    }
    for (int c = tid; c < LKP * 4; c += 256) {
        // two neighbouring keys x 8 channels -> 8 dwords of V^T, one per channel
        const int pair = c >> 3, dc = c & 7;
        const int k0 = 2 * pair < p.Lk ? 2 * pair : p.Lk - 1, k1 = 2 * pair + 1 < p.Lk ? 2 * pair + 1 : p.Lk - 1;
        const u32x4 a = *(const u32x4*)(vb + (int64_t)k0 * p.v_sl + dc * 8);
        const u32x4 c2 = *(const u32x4*)(vb + (int64_t)k1 * p.v_sl + dc * 8);
        char* dst = smem + vt_off(NT) + (8 * dc) * VT_ROW + pair * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *(uint32_t*)(dst + (2 * i) * VT_ROW) = (a[i] & 0xffffu) | (c2[i] << 16);
            *(uint32_t*)(dst + (2 * i + 1) * VT_ROW) = (a[i] >> 16) | (c2[i] & 0xffff0000u);
        }
    }
    for (int key = tid; key < LKP; key += 256) {
        float bv = -INFINITY;
        if (key < p.Lk) {
            bv = p.key_bias ? p.key_bias[(int64_t)b * p.bias_sb + key] : 0.f;
            if (!(bv > KEY_REMOVED)) bv = -INFINITY;
        }
        *(float*)(smem + kb_off(NT) + key * 4) = bv;
    }
    // rel[t] = the bias of offset d = key - query = t - (q0 + 63) for this head; offsets no (query, key) pair of the call has read 0
    for (int t = tid; t < LKP + Q_TILE; t += 256) {
        const int d = t - (q0 + Q_TILE - 1);
        float rv = 0.f;
        if (d >= -(p.Lq - 1) && d <= p.Lk - 1) rv = p.rel[(int64_t)head * p.rel_sh + p.rel_center + d];
        *(float*)(smem + rb_off(NT) + t * 4) = rv;
    }

    // ---- Q^T fragments (B operand): Q[query][32 s + 8 g .. + 7]
    const int qi = 16 * wave + c16;                          // the lane's query within the tile
    const int qrow = q0 + qi < p.Lq ? q0 + qi : p.Lq - 1;
    bf16x8 qf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) qf[s] = *(const bf16x8*)(qb + (int64_t)qrow * p.q_sl + 32 * s + 8 * g);
    __syncthreads();                                         // the only barrier: the images are read-only from here on

    // ---- x = scale * K Q^T + rel + key bias: register r of tile t holds key 16 t + 4 g + r for query c16
    f32x4 x[2 * NT];
    const char* krd = smem + k_off(NT) + c16 * K_ROW + g * 16;
    const float* relp = (const float*)(smem + rb_off(NT)) + (4 * g - qi + Q_TILE - 1);
    const float* kbp = (const float*)(smem + kb_off(NT)) + 4 * g;
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2 * NT; ++t) {
        const bf16x8 k0 = *(const bf16x8*)(krd + t * 16 * K_ROW), k1 = *(const bf16x8*)(krd + t * 16 * K_ROW + 64);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[1], acc, 0, 0, 0);
        const f32x4 kbv = *(const f32x4*)(kbp + 16 * t);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            x[t][r] = (acc[r] * p.scale + relp[16 * t + r]) + kbv[r];
            m = fmaxf(m, x[t][r]);
        }
    }
    // a query's keys are spread over the four 16-lane groups
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    if (m == -INFINITY) m = 0.f;                             // every key removed: outside the contract, kept free of inf - inf
    const float nm = -m * LOG2E;

    // ---- P = 2^((x - m) log2 e) rounded to bf16, l = sum of the rounded P, O^T += V^T P^T in steps of 32 keys
    f32x4 oT[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oT[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    const char* vrd = smem + vt_off(NT) + c16 * VT_ROW + g * 8;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const __bf16 pv = (__bf16)fast_exp2(x[2 * u + (j >> 2)][j & 3] * LOG2E + nm);
            pf[j] = pv;
            l += (float)pv;
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            // V^T[16 dt + c16][32 u + 4 g .. + 3] and [.. + 16 ..]: the keys of P's elements 0..3 and 4..7
            const char* at = vrd + dt * 16 * VT_ROW + u * 64;
            const u32x2 lo = *(const u32x2*)at, hi = *(const u32x2*)(at + 32);
            const u32x4 w = {lo[0], lo[1], hi[0], hi[1]};
            oT[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), pf, oT[dt], 0, 0, 0);
        }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;

    // ---- O[query][16 dt + 4 g + r] = O^T / l: 8 bytes per lane and tile
    if (q0 + qi < p.Lq) {
        uint16_t* orow = ob + (int64_t)(q0 + qi) * p.o_sl + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            u32x2 w;
            w[0] = pack_bf16(oT[dt][0] * inv, oT[dt][1] * inv);
            w[1] = pack_bf16(oT[dt][2] * inv, oT[dt][3] * inv);
            *(u32x2*)(orow + 16 * dt) = w;
        }
    }
}

template <int NT>
static int launch_relbias(const RelBiasParams& p, hipStream_t stream) {
    const int64_t grid = (int64_t)p.B * p.H * p.q_tiles;
    return launch_with_lds<attn_relbias_kernel<NT>>(p, dim3((unsigned)grid), dim3(256), smem_bytes(NT), stream,
                                                    "ltxmi_attention_relbias_bf16");
}

// ------------------------------------------------------------------ T5LayerNorm: out of place, two roundings
// One wave per row as rowops.hip: fp32 sum of squares in a fixed order, then y = bf16(bf16(x * rstd) * w).
// The row statistic, kept apart from the build's fast-math.  The squares are added in the order written here (reassociation
// off): per lane its chunks in turn, eight elements each, then the wave butterfly.  The factor is 1 / sqrt(sum / D + eps) with the
// divide, the square root and the reciprocal taken in double and rounded to fp32 after each step: a double result good to 2^-51
// (what the fast-math expansions of the f64 divide and square root keep) rounds to the correctly rounded fp32 value, because the
// exact quotient, root or reciprocal of fp32 operands is either an fp32 value or at least 2^-50 (relative) away from a 25-bit
// midpoint.  That is mean, + eps and rsqrt as torch computes them in fp32 on the CPU.  bf16(x * rstd) is a second rounding of an
// fp32 product, so a factor one fp32 ulp off moves the elements that sit on a bf16 tie by a whole bf16 ulp.
// tests/test_gpu_t5_kernels.py replays this order and these roundings.
__device__ __forceinline__ float sumsq_chunk(float s, const float (&v)[8]) {
#pragma clang fp reassociate(off)
#pragma unroll
    for (int e = 0; e < 8; ++e) s = s + v[e] * v[e];         // (a bf16 square is exact in fp32: fused or not, one rounding per add)
    return s;
}
__device__ __forceinline__ float rstd_rounded(float sumsq, int D, float eps) {
#pragma clang fp reassociate(off) contract(off)
    const float mean = (float)((double)sumsq / (double)D);
    const float var = mean + eps;
    double root = (double)(float)__builtin_sqrt((double)var);
    asm volatile("" : "+v"(root));                           // (opaque: else 1.0 / (double)(float) narrows to an fp32 v_rcp_f32)
    return (float)(1.0 / root);
}

template <int NCH>
__global__ __launch_bounds__(256) void rmsnorm_weight_kernel(const uint16_t* __restrict__ x, int64_t ldx, uint16_t* __restrict__ y,
                                                             int64_t ldy, int rows, int D, const uint16_t* __restrict__ w,
                                                             float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nchunk = D >> 3;
    const uint16_t* xr = x + (int64_t)row * ldx;
    Chunk c[NCH];
    float s2 = 0.f;
    LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
        c[j] = load_bf16x8(xr + ch * 8);
        s2 = sumsq_chunk(s2, c[j].v);
    }
    const float rstd = rstd_rounded(wave_sum(s2), D, eps);
    uint16_t* yr = y + (int64_t)row * ldy;
    LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
        const Chunk wt = load_bf16x8(w + ch * 8);
        Chunk o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.v[e] = bf2f(f2bf(c[j].v[e] * rstd)) * wt.v[e];
        store_bf16x8(yr + ch * 8, o);
    }
}

// ------------------------------------------------------------------ gated tanh-GELU over [rows, 2F]
constexpr int GG_THREADS = 256;
constexpr int GG_MAX_BLOCKS = 256 * 8;      // grid-stride beyond 8 blocks per CU

// gelu_tanh(x) = 0.5 x (1 + tanh u) = x sigmoid(2u) = x / (1 + 2^-t), t = 2 log2(e) u, u = sqrt(2/pi) (x + 0.044715 x^3): the form
// without the cancellation of 1 + tanh u.  common.h's gelu_tanh_f is this for t > -126; below that (x < -9.3) 2^-t overflows or
// its reciprocal is a denormal that v_rcp_f32 flushes, and the value -- 1e-37 down to the fp32 denormals, which bf16 still
// represents -- came out as 0 or with a few bits.  From t < -32 on, 1 + 2^-t is 2^-t to fp32, so sigmoid = 2^t: taken with 2^64
// of head-room so that neither the exponential nor the product with x passes through a denormal; the last multiply by 2^-64 is
// exact or the one rounding into the denormal range.  x^2 and x^3 of a bf16 x are exact in fp32: t carries two roundings.
__device__ __forceinline__ float gelu_tanh_full_range(float x) {
    const float t = fmaf(0.10294324f, x * x * x, 2.30220820f * x);
    if (t < -32.f) return (x * fast_exp2(t + 64.f)) * 0x1p-64f;
    return gelu_tanh_f(x);
}

__global__ __launch_bounds__(GG_THREADS) void gated_gelu_kernel(const uint16_t* __restrict__ h, int64_t ldh,
                                                                uint16_t* __restrict__ y, int64_t ldy, int64_t rows, int F) {
    const int cpr = F >> 3;                                  // 16-byte chunks per output row
    const int64_t total = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * GG_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * GG_THREADS) {
        const int64_t r = i / cpr;
        const int c = (int)(i - r * cpr) * 8;
        const Chunk a = load_bf16x8(h + r * ldh + c), gt = load_bf16x8(h + r * ldh + F + c);
        Chunk o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.v[e] = bf2f(f2bf(gelu_tanh_full_range(a.v[e]))) * gt.v[e];
        store_bf16x8(y + r * ldy + c, o);
    }
}

// ------------------------------------------------------------------ embedding gather, one workgroup per row
__global__ __launch_bounds__(256) void embedding_kernel(const int64_t* __restrict__ ids, const uint16_t* __restrict__ table,
                                                        int64_t ld_table, int64_t vocab, uint16_t* __restrict__ out, int64_t ldo,
                                                        int D) {
    const int64_t row = blockIdx.x;
    const int64_t id = ids[row];
    const bool ok = id >= 0 && id < vocab;                   // an id outside the table is never turned into an address
    const uint16_t* src = table + (ok ? id : 0) * ld_table;
    uint16_t* dst = out + row * ldo;
    for (int ch = threadIdx.x; ch < (D >> 3); ch += 256) {
        u32x4 w = {0u, 0u, 0u, 0u};
        if (ok) w = *(const u32x4*)(src + ch * 8);
        *(u32x4*)(dst + ch * 8) = w;
    }
}

}  // namespace t5

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_attention_relbias_bf16(const ltxmi_attn_relbias_args* a, void* stream) {
    LTXMI_REQUIRE(a && a->q && a->k && a->v && a->o, LTXMI_ERR_INVALID_ARG, "ltxmi_attention_relbias_bf16: NULL argument");
    LTXMI_REQUIRE(a->B > 0 && a->H > 0 && a->Lq > 0 && a->Lk > 0, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_attention_relbias_bf16: non-positive shape B=%d H=%d Lq=%d Lk=%d", a->B, a->H, a->Lq, a->Lk);
    LTXMI_REQUIRE(a->head_dim == 64, LTXMI_ERR_UNSUPPORTED, "ltxmi_attention_relbias_bf16: head_dim %d is not 64", a->head_dim);
    LTXMI_REQUIRE(a->Lq <= 512 && a->Lk <= 512, LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_attention_relbias_bf16: Lq=%d, Lk=%d: at most 512 queries and 512 keys", a->Lq, a->Lk);
    const int64_t strides[] = {a->q_stride_b, a->q_stride_l, a->k_stride_b, a->k_stride_l,
                               a->v_stride_b, a->v_stride_l, a->o_stride_b, a->o_stride_l};
    for (int64_t s : strides)
        LTXMI_REQUIRE(s % 8 == 0, LTXMI_ERR_UNSUPPORTED, "ltxmi_attention_relbias_bf16: strides must be multiples of 8 elements");
    LTXMI_REQUIRE((((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->o) & 15) == 0, LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_attention_relbias_bf16: q/k/v/o must be 16-byte aligned");
    LTXMI_REQUIRE((((uintptr_t)a->key_bias | (uintptr_t)a->rel_bias) & 3) == 0, LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_attention_relbias_bf16: key_bias and rel_bias must be 4-byte aligned");
    const int q_tiles = (a->Lq + t5::Q_TILE - 1) / t5::Q_TILE;
    LTXMI_REQUIRE((int64_t)a->B * a->H * q_tiles < (1ll << 31), LTXMI_ERR_UNSUPPORTED, "ltxmi_attention_relbias_bf16: grid too large");
    if (!a->rel_bias) {
        // no relative bias: the library's plain attention, with its arithmetic and its choice of kernel
        ltxmi_attn_args f = {};
        f.q = a->q; f.q_stride_b = a->q_stride_b; f.q_stride_l = a->q_stride_l;
        f.k = a->k; f.k_stride_b = a->k_stride_b; f.k_stride_l = a->k_stride_l;
        f.v = a->v; f.v_stride_b = a->v_stride_b; f.v_stride_l = a->v_stride_l;
        f.o = a->o; f.o_stride_b = a->o_stride_b; f.o_stride_l = a->o_stride_l;
        f.key_bias = a->key_bias; f.bias_stride_b = a->bias_stride_b;
        f.B = a->B; f.H = a->H; f.Lq = a->Lq; f.Lk = a->Lk; f.head_dim = a->head_dim;
        f.softmax_scale = a->softmax_scale;
        return ltxmi_attention_fwd_bf16(&f, stream);
    }
    LTXMI_REQUIRE(a->rel_center >= a->Lq - 1 && a->rel_stride_h >= (int64_t)a->rel_center + a->Lk, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_attention_relbias_bf16: rel_center=%d must be >= Lq - 1 and rel_stride_h=%lld >= rel_center + Lk", a->rel_center,
                  (long long)a->rel_stride_h);
    t5::RelBiasParams p;
    p.q = (const uint16_t*)a->q; p.q_sb = a->q_stride_b; p.q_sl = a->q_stride_l;
    p.k = (const uint16_t*)a->k; p.k_sb = a->k_stride_b; p.k_sl = a->k_stride_l;
    p.v = (const uint16_t*)a->v; p.v_sb = a->v_stride_b; p.v_sl = a->v_stride_l;
    p.o = (uint16_t*)a->o; p.o_sb = a->o_stride_b; p.o_sl = a->o_stride_l;
    p.key_bias = a->key_bias; p.bias_sb = a->bias_stride_b;
    p.rel = a->rel_bias; p.rel_sh = a->rel_stride_h; p.rel_center = a->rel_center;
    p.B = a->B; p.H = a->H; p.Lq = a->Lq; p.Lk = a->Lk; p.q_tiles = q_tiles;
    p.scale = a->softmax_scale;
    hipStream_t s = (hipStream_t)stream;
    const int steps = (a->Lk + 31) / 32;
    if (steps <= 1) return t5::launch_relbias<1>(p, s);
    if (steps <= 2) return t5::launch_relbias<2>(p, s);
    if (steps <= 4) return t5::launch_relbias<4>(p, s);
    if (steps <= 8) return t5::launch_relbias<8>(p, s);
    return t5::launch_relbias<16>(p, s);
}

extern "C" int ltxmi_rmsnorm_weight_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t D,
                                         const void* weight, float eps, void* stream) {
    LTXMI_REQUIRE(x && y && weight, LTXMI_ERR_INVALID_ARG, "ltxmi_rmsnorm_weight_bf16: NULL argument");
    LTXMI_REQUIRE(rows > 0 && D > 0, LTXMI_ERR_INVALID_ARG, "ltxmi_rmsnorm_weight_bf16: non-positive size rows=%d D=%d", rows, D);
    LTXMI_REQUIRE(row_width_ok(D) && row_stride_ok(ldx, D) && row_stride_ok(ldy, D), LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_rmsnorm_weight_bf16: D=%d must be a multiple of 8 and <= 8192 (strides multiples of 8, >= D)", D);
    LTXMI_REQUIRE(aligned16(x, y, weight), LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_rmsnorm_weight_bf16: x, y and weight must be 16-byte aligned");
    // (a launch takes fewer than 2^32 threads: 2^24 - 1 workgroups of 256)
    const int64_t grid = ((int64_t)rows + ROWS_PER_WG - 1) / ROWS_PER_WG;
    LTXMI_REQUIRE(grid < (1ll << 24), LTXMI_ERR_UNSUPPORTED, "ltxmi_rmsnorm_weight_bf16: rows=%d: at most %d rows per call", rows,
                  ROWS_PER_WG * ((1 << 24) - 1));
    hipStream_t s = (hipStream_t)stream;
    dispatch_nch<true>(D, [&](auto nch) {                    // (with the NCH = 8 instance: T5-XXL's d_model, 4096)
        hipLaunchKernelGGL((t5::rmsnorm_weight_kernel<decltype(nch)::value>), dim3((unsigned)grid), dim3(256), 0, s, (const uint16_t*)x,
                           ldx, (uint16_t*)y, ldy, rows, D, (const uint16_t*)weight, eps);
    });
    return check_launch("ltxmi_rmsnorm_weight_bf16");
}

extern "C" int ltxmi_gated_gelu_bf16(const void* h, int64_t ldh, void* y, int64_t ldy, int32_t rows, int32_t F, void* stream) {
    LTXMI_REQUIRE(h && y, LTXMI_ERR_INVALID_ARG, "ltxmi_gated_gelu_bf16: NULL argument");
    LTXMI_REQUIRE(rows > 0 && F > 0, LTXMI_ERR_INVALID_ARG, "ltxmi_gated_gelu_bf16: non-positive size rows=%d F=%d", rows, F);
    LTXMI_REQUIRE(F % 8 == 0 && ldh % 8 == 0 && ldh >= 2 * (int64_t)F && row_stride_ok(ldy, F), LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_gated_gelu_bf16: F=%d must be a multiple of 8 (strides multiples of 8, ldh >= 2 F, ldy >= F)", F);
    LTXMI_REQUIRE(aligned16(h, y), LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_gated_gelu_bf16: h and y must be 16-byte aligned");
    const int64_t total = (int64_t)rows * (F >> 3);
    int64_t grid = (total + t5::GG_THREADS - 1) / t5::GG_THREADS;
    if (grid > t5::GG_MAX_BLOCKS) grid = t5::GG_MAX_BLOCKS;
    hipLaunchKernelGGL(t5::gated_gelu_kernel, dim3((unsigned)grid), dim3(t5::GG_THREADS), 0, (hipStream_t)stream,
                       (const uint16_t*)h, ldh, (uint16_t*)y, ldy, (int64_t)rows, F);
    return check_launch("ltxmi_gated_gelu_bf16");
}

extern "C" int ltxmi_embedding_bf16(const int64_t* ids, const void* table, int64_t ld_table, int64_t vocab, void* out, int64_t ldo,
                                    int32_t rows, int32_t D, void* stream) {
    LTXMI_REQUIRE(ids && table && out, LTXMI_ERR_INVALID_ARG, "ltxmi_embedding_bf16: NULL argument");
    LTXMI_REQUIRE(rows > 0 && D > 0 && vocab > 0, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_embedding_bf16: non-positive size rows=%d D=%d vocab=%lld", rows, D, (long long)vocab);
    LTXMI_REQUIRE(D % 8 == 0 && ld_table % 8 == 0 && ldo % 8 == 0 && ld_table >= D && ldo >= D, LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_embedding_bf16: D=%d must be a multiple of 8 (strides multiples of 8, >= D)", D);
    LTXMI_REQUIRE((((uintptr_t)table | (uintptr_t)out) & 15) == 0 && (((uintptr_t)ids) & 7) == 0, LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_embedding_bf16: table and out must be 16-byte aligned, ids 8-byte aligned");
    LTXMI_REQUIRE(rows < (1 << 24), LTXMI_ERR_UNSUPPORTED, "ltxmi_embedding_bf16: rows=%d: at most %d rows per call (one workgroup each)",
                  rows, (1 << 24) - 1);
    hipLaunchKernelGGL(t5::embedding_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, ids, (const uint16_t*)table,
                       ld_table, vocab, (uint16_t*)out, ldo, D);
    return check_launch("ltxmi_embedding_bf16");
}
