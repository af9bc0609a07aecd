// t5_mx8.hip -- the two row passes of the quantised T5 encoder (include/ltxmi_mx_t5.h): T5LayerNorm and the gated tanh-GELU
// whose output row leaves as MX-FP8.  Each is its bf16 twin of t5.hip up to the bf16 rounding of a chunk, then the chunk step of
// quantize_mx8_kernel (quant_mx8.hip) on those bf16 bits in registers, as norm_mx8.hip does for the DiT's norm: the twins give
// four neighbouring lanes the four 8-element chunks of a 32-element block, so a block's amax is two shuffles.  The bf16 row is
// never written or read back.
//
// The row statistic and the activation are t5.hip's functions restated word for word (that file's kernels are pinned by
// tests/test_kernel_resources.py and stay as they are); tests/test_gpu_mxt_kernels.py holds the results to the two-launch
// composition bit for bit.
#include "mx8.h"
#include "rows.h"
#include "../../include/ltxmi_mx_t5.h"

namespace ltxmi {

namespace t5mx {

// ---- t5.hip's sumsq_chunk and rstd_rounded: the squares added in the order written (reassociation off), the factor through
// double with every step rounded to fp32
__device__ __forceinline__ float sumsq_chunk(float s, const float (&v)[8]) {
#pragma clang fp reassociate(off)
#pragma unroll
    for (int e = 0; e < 8; ++e) s = s + v[e] * v[e];
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
// ---- t5.hip's gelu_tanh_full_range
__device__ __forceinline__ float gelu_tanh_full_range(float x) {
    const float t = fmaf(0.10294324f, x * x * x, 2.30220820f * x);
    if (t < -32.f) return (x * fast_exp2(t + 64.f)) * 0x1p-64f;
    return gelu_tanh_f(x);
}

// quantize_mx8_kernel's chunk step on the 8 bf16 values w of chunk ch: the lanes l ^ 1, l ^ 2 hold the rest of the block
__device__ __forceinline__ void quantize_chunk(const u32x4& w, uint8_t* qr, uint8_t* sr, int ch, int lane) {
    uint32_t am = 0;                       // |y| as bf16 bits: their integer order is the values' order
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        am = max(am, w[i] & 0x7fffu);
        am = max(am, (w[i] >> 16) & 0x7fffu);
    }
    am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
    am = max(am, (uint32_t)__shfl_xor((int)am, 2, 64));
    const int byte = mx8_scale_byte(am << 16);
    const float inv = mx8_inv_scale(byte);
    u32x2 o8;
    o8[0] = mx8_pack4(bf_lo(w[0]), bf_hi(w[0]), bf_lo(w[1]), bf_hi(w[1]), inv);
    o8[1] = mx8_pack4(bf_lo(w[2]), bf_hi(w[2]), bf_lo(w[3]), bf_hi(w[3]), inv);
    *(u32x2*)(qr + ch * 8) = o8;
    if ((lane & 3) == 0) sr[ch >> 2] = (uint8_t)byte;
}

template <int NCH>
__global__ __launch_bounds__(256) void rmsnorm_weight_mx8_kernel(const uint16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ q,
                                                                 int64_t ldq, uint8_t* __restrict__ sc, int64_t lds, int rows, int D,
                                                                 const uint16_t* __restrict__ w, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nchunk = D >> 3;             // a multiple of 4: the four lanes of a block are in a chunk step together
    const uint16_t* xr = x + (int64_t)row * ldx;
    Chunk c[NCH];
    float s2 = 0.f;
    LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
        c[j] = load_bf16x8(xr + ch * 8);
        s2 = sumsq_chunk(s2, c[j].v);
    }
    const float rstd = rstd_rounded(wave_sum(s2), D, eps);
    uint8_t* qr = q + (int64_t)row * ldq;
    uint8_t* sr = sc + (int64_t)row * lds;
    LTXMI_FOR_ROW_CHUNKS(NCH, lane, nchunk, j, ch) {
        const Chunk wt = load_bf16x8(w + ch * 8);
        u32x4 y;                           // the bf16 words rmsnorm_weight_kernel stores
#pragma unroll
        for (int i = 0; i < 4; ++i)
            y[i] = pack_bf16(bf2f(f2bf(c[j].v[2 * i] * rstd)) * wt.v[2 * i], bf2f(f2bf(c[j].v[2 * i + 1] * rstd)) * wt.v[2 * i + 1]);
        quantize_chunk(y, qr, sr, ch, lane);
    }
}

constexpr int GG_THREADS = 256;
constexpr int GG_MAX_BLOCKS = 256 * 8;

// gated_gelu_kernel's walk: thread i takes chunk i of the [rows, F / 8] chunks, so the four chunks of a block (F % 32 == 0) are
// four neighbouring lanes, in the loop together
__global__ __launch_bounds__(GG_THREADS) void gated_gelu_mx8_kernel(const uint16_t* __restrict__ h, int64_t ldh, uint8_t* __restrict__ q,
                                                                    int64_t ldq, uint8_t* __restrict__ sc, int64_t lds, int64_t rows,
                                                                    int F) {
    const int cpr = F >> 3;
    const int64_t total = rows * cpr;
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * GG_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * GG_THREADS) {
        const int64_t r = i / cpr;
        const int ch = (int)(i - r * cpr);
        const Chunk a = load_bf16x8(h + r * ldh + ch * 8), gt = load_bf16x8(h + r * ldh + F + ch * 8);
        u32x4 y;                           // the bf16 words gated_gelu_kernel stores
#pragma unroll
        for (int e = 0; e < 4; ++e)
            y[e] = pack_bf16(bf2f(f2bf(gelu_tanh_full_range(a.v[2 * e]))) * gt.v[2 * e],
                             bf2f(f2bf(gelu_tanh_full_range(a.v[2 * e + 1]))) * gt.v[2 * e + 1]);
        quantize_chunk(y, q + r * ldq, sc + r * lds, ch, lane);
    }
}

}  // namespace t5mx

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_rmsnorm_weight_mx8(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int32_t rows,
                                        int32_t D, const void* weight, float eps, void* stream) {
    const char* what = "ltxmi_rmsnorm_weight_mx8";
    LTXMI_REQUIRE(x && q && scales && weight, LTXMI_ERR_INVALID_ARG, "%s: NULL argument", what);
    LTXMI_REQUIRE(rows > 0 && D > 0, LTXMI_ERR_INVALID_ARG, "%s: non-positive size rows=%d D=%d", what, rows, D);
    LTXMI_REQUIRE(D % LTXMI_MX_BLOCK == 0 && D <= 8192, LTXMI_ERR_UNSUPPORTED, "%s: D=%d must be a multiple of 32 and <= 8192", what, D);
    LTXMI_REQUIRE(row_stride_ok(ldx, D) && ldq % 16 == 0 && ldq >= D && lds >= D / LTXMI_MX_BLOCK, LTXMI_ERR_UNSUPPORTED,
                  "%s: ldx %% 8, ldq %% 16 and every stride >= its row (ldx=%lld ldq=%lld lds=%lld D=%d)", what, (long long)ldx,
                  (long long)ldq, (long long)lds, D);
    LTXMI_REQUIRE(aligned16(x, q, weight), LTXMI_ERR_UNSUPPORTED, "%s: x, q and weight must be 16-byte aligned", what);
    const int64_t grid = ((int64_t)rows + ROWS_PER_WG - 1) / ROWS_PER_WG;
    LTXMI_REQUIRE(grid < (1ll << 24), LTXMI_ERR_UNSUPPORTED, "%s: rows=%d: at most %d rows per call", what, rows,
                  ROWS_PER_WG * ((1 << 24) - 1));
    hipStream_t s = (hipStream_t)stream;
    dispatch_nch<true>(D, [&](auto nch) {
        hipLaunchKernelGGL((t5mx::rmsnorm_weight_mx8_kernel<decltype(nch)::value>), dim3((unsigned)grid), dim3(256), 0, s,
                           (const uint16_t*)x, ldx, (uint8_t*)q, ldq, (uint8_t*)scales, lds, rows, D, (const uint16_t*)weight, eps);
    });
    return check_launch(what);
}

extern "C" int ltxmi_gated_gelu_mx8(const void* h, int64_t ldh, void* q, int64_t ldq, void* scales, int64_t lds, int32_t rows,
                                    int32_t F, void* stream) {
    const char* what = "ltxmi_gated_gelu_mx8";
    LTXMI_REQUIRE(h && q && scales, LTXMI_ERR_INVALID_ARG, "%s: NULL argument", what);
    LTXMI_REQUIRE(rows > 0 && F > 0, LTXMI_ERR_INVALID_ARG, "%s: non-positive size rows=%d F=%d", what, rows, F);
    LTXMI_REQUIRE(F % LTXMI_MX_BLOCK == 0, LTXMI_ERR_UNSUPPORTED, "%s: F=%d must be a multiple of 32", what, F);
    LTXMI_REQUIRE(ldh % 8 == 0 && ldh >= 2 * (int64_t)F && ldq % 16 == 0 && ldq >= F && lds >= F / LTXMI_MX_BLOCK, LTXMI_ERR_UNSUPPORTED,
                  "%s: ldh %% 8, ldq %% 16 and every stride >= its row (ldh=%lld >= 2 F, ldq=%lld, lds=%lld, F=%d)", what,
                  (long long)ldh, (long long)ldq, (long long)lds, F);
    LTXMI_REQUIRE(aligned16(h, q), LTXMI_ERR_UNSUPPORTED, "%s: h and q must be 16-byte aligned", what);
    const int64_t total = (int64_t)rows * (F >> 3);
    int64_t grid = (total + t5mx::GG_THREADS - 1) / t5mx::GG_THREADS;
    if (grid > t5mx::GG_MAX_BLOCKS) grid = t5mx::GG_MAX_BLOCKS;
    hipLaunchKernelGGL(t5mx::gated_gelu_mx8_kernel, dim3((unsigned)grid), dim3(t5mx::GG_THREADS), 0, (hipStream_t)stream,
                       (const uint16_t*)h, ldh, (uint8_t*)q, ldq, (uint8_t*)scales, lds, (int64_t)rows, F);
    return check_launch(what);
}
