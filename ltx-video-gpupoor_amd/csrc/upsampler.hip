// upsampler.hip -- the HBM-bound pieces of the multi-scale bridge between pass 1 and pass 2
// (LatentUpsampler, latent_upsampler.py:15-149; adain_filter_latent, pipeline_ltx_video.py:1709-1737):
// GroupNorm(32) (+ residual) + SiLU over channels-last activations, the pixel shuffle after the
// upsampling convolution (2-D; N-D with the temporal modes' frame trim), and the per-channel AdaIN statistics transfer.  The convolutions themselves
// are the implicit GEMM of gemm.hip (kernel_t / time_pad_zeros options).
#include <math.h>

#include "common.h"

namespace ltxmi {

constexpr int UP_THREADS = 256;

// ---------------------------------------------------------------- GroupNorm, channels-last
// x [Bn, S, C]: per (sample, row block, channel) SHIFTED sum / sum of squares -> part[Bn][blocks][C][2] (fp32), the shift
// being the channel's value in the sample's first row: with d = x - pivot the sums stay of the order of the data's spread,
// so the variance does not drown in mean^2 (E[x^2] - mean^2 in fp32 lost it once |mean| was a few hundred standard
// deviations), and the activation is still read only once for the statistics.  Thread -> (row offset, 8-channel slot); a
// block reduces its rows through LDS and writes ONE pair per channel into its own slot: no atomics, so the result does not
// depend on the order in which blocks finish.  C/8 is a power of two <= 256.
__global__ void gn_stats_kernel(const uint16_t* __restrict__ x, float* __restrict__ part, int64_t S, int C,
                                int rows_per_block) {
    __shared__ float red[UP_THREADS][17];                 // [thread][8 sums + 8 squares], padded
    const int slots = C >> 3;
    const int rpi = UP_THREADS / slots;                    // rows per iteration
    const int slot = threadIdx.x % slots, roff = threadIdx.x / slots;
    const int64_t b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    int64_t r1 = r0 + rows_per_block;
    if (r1 > S) r1 = S;
    float s[8], q[8], pv[8];
    {
        const u32x4 w = *(const u32x4*)(x + b * S * C + slot * 8);
#pragma unroll
        for (int k = 0; k < 4; ++k) { pv[2 * k] = bf_lo(w[k]); pv[2 * k + 1] = bf_hi(w[k]); }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = q[k] = 0.f;
    for (int64_t r = r0 + roff; r < r1; r += rpi) {
        const u32x4 w = *(const u32x4*)(x + (b * S + r) * C + slot * 8);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float lo = bf_lo(w[k]) - pv[2 * k], hi = bf_hi(w[k]) - pv[2 * k + 1];
            s[2 * k] += lo; q[2 * k] += lo * lo;
            s[2 * k + 1] += hi; q[2 * k + 1] += hi * hi;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { red[threadIdx.x][k] = s[k]; red[threadIdx.x][8 + k] = q[k]; }
    __syncthreads();
    // thread t < slots*16 finalises value (slot, k): sum over the rpi row-offset copies, in order
    float* dst = part + (b * gridDim.x + blockIdx.x) * (int64_t)C * 2;
    for (int v = threadIdx.x; v < slots * 16; v += UP_THREADS) {
        const int sl = v >> 4, k = v & 15;
        float acc = 0.f;
        for (int j = 0; j < rpi; ++j) acc += red[j * slots + sl][k];
        const int ch = sl * 8 + (k & 7);
        dst[(ch << 1) + (k >> 3)] = acc;
    }
}

// part[Bn][blocks][C][2] -> stat[Bn][G][2] = (mean, rstd) over S * C/G values; one workgroup per (sample, group).
// The block partials of a channel are added in block order (a fixed subset per thread, then the threads in order), each
// channel becomes (mean_c, M2_c) about its own mean, and the channels of the group are combined by the parallel-variance
// formula M2 = sum M2_c + S sum (mean_c - mean)^2.  In double: a few thousand values per group, nothing on the clock.
constexpr int GN_MAX_CG = 2048;
__global__ __launch_bounds__(UP_THREADS) void gn_finalize_kernel(const uint16_t* __restrict__ x,
                                                                 const float* __restrict__ part, float* __restrict__ stat,
                                                                 int C, int G, int64_t S, int blocks, float eps) {
    __shared__ double ts[UP_THREADS], tq[UP_THREADS];
    __shared__ double ch_mean[GN_MAX_CG], ch_m2[GN_MAX_CG];
    const int t = threadIdx.x;
    const int b = blockIdx.x / G, g = blockIdx.x % G, cg = C / G;      // cg is a power of two
    const int lanes = cg < UP_THREADS ? cg : UP_THREADS;               // channels in flight
    const int tpc = UP_THREADS / lanes;                                // threads per channel
    const int cl = t % lanes, sub = t / lanes;
    for (int c0 = 0; c0 < cg; c0 += lanes) {
        const int c = g * cg + c0 + cl;
        double s = 0.0, q = 0.0;
        for (int blk = sub; blk < blocks; blk += tpc) {
            const float* p = part + (((int64_t)b * blocks + blk) * C + c) * 2;
            s += (double)p[0];
            q += (double)p[1];
        }
        ts[t] = s;
        tq[t] = q;
        __syncthreads();
        if (sub == 0) {
            for (int j = 1; j < tpc; ++j) { s += ts[j * lanes + cl]; q += tq[j * lanes + cl]; }
            const double pivot = (double)bf2f(x[(int64_t)b * S * C + c]);
            ch_mean[c0 + cl] = pivot + s / (double)S;
            ch_m2[c0 + cl] = q - s * s / (double)S;
        }
        __syncthreads();
    }
    if (t == 0) {
        double ms = 0.0;
        for (int c = 0; c < cg; ++c) ms += ch_mean[c];
        const double mean = ms / cg;
        double m2 = 0.0;
        for (int c = 0; c < cg; ++c) {
            const double d = ch_mean[c] - mean;
            m2 += ch_m2[c] + (double)S * d * d;
        }
        const double var = fmax(m2 / ((double)S * cg), 0.0);           // biased, like nn.GroupNorm
        stat[blockIdx.x * 2] = (float)mean;
        stat[blockIdx.x * 2 + 1] = rsqrtf((float)var + eps);
    }
}

// y = silu((x - mean) * rstd * gamma + beta (+ residual))
__global__ void gn_apply_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y,
                                const uint16_t* __restrict__ res, const float* __restrict__ stat,
                                const uint16_t* __restrict__ gamma, const uint16_t* __restrict__ beta, int64_t S, int C,
                                int G, int64_t total_chunks) {
    const int slots = C >> 3, cg = C / G;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total_chunks;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int slot = (int)(i % slots);
        const int64_t row = i / slots;
        const int64_t b = row / S;
        const u32x4 w = *(const u32x4*)(x + i * 8);
        const u32x4 gm = *(const u32x4*)(gamma + slot * 8);
        const u32x4 bt = *(const u32x4*)(beta + slot * 8);
        u32x4 rr = {0u, 0u, 0u, 0u};
        if (res) rr = *(const u32x4*)(res + i * 8);
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c0 = slot * 8 + 2 * k;
            const float* st0 = stat + (b * G + c0 / cg) * 2;
            const float* st1 = stat + (b * G + (c0 + 1) / cg) * 2;
            float lo = (bf_lo(w[k]) - st0[0]) * st0[1] * bf_lo(gm[k]) + bf_lo(bt[k]);
            float hi = (bf_hi(w[k]) - st1[0]) * st1[1] * bf_hi(gm[k]) + bf_hi(bt[k]);
            if (res) { lo += bf_lo(rr[k]); hi += bf_hi(rr[k]); }
            o[k] = pack_bf16(silu_f(lo), silu_f(hi));
        }
        *(u32x4*)(y + i * 8) = o;
    }
}

// ---------------------------------------------------------------- 2-D pixel shuffle, channels-last
// x [R, H, W, 4C] with channel (p1*2 + p2)*C + c (conv rows packed that way) -> y [R, 2H, 2W, C]
// = PixelShuffleND(2) "b (c p1 p2) h w -> b c (h p1) (w p2)" (pixel_shuffle.py:12-21); 16-byte copies.
__global__ void pixel_shuffle2d_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int H, int W, int C,
                                       int64_t total_chunks) {
    const int slots = C >> 3;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total_chunks;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int slot = (int)(i % slots);
        int64_t r = i / slots;
        const int xo = (int)(r % (2 * W)); r /= 2 * W;
        const int yo = (int)(r % (2 * H));
        const int64_t f = r / (2 * H);
        const int p = (yo & 1) * 2 + (xo & 1);
        const int64_t src = (((f * H + (yo >> 1)) * W + (xo >> 1)) * 4 + p) * C + slot * 8;
        *(u32x4*)(y + i * 8) = *(const u32x4*)(x + src);
    }
}

// ---------------------------------------------------------------- N-D pixel shuffle + frame trim, channels-last
// x [B, T, H, W, pt*ps*ps*C] with channel ((p1*ps + p2)*ps + p3)*C + c (conv rows packed that way) ->
// y [B, pt*T - drop, ps*H, ps*W, C] = PixelShuffleND(1 | 2 | 3) (pixel_shuffle.py:12-33) followed by the temporal
// modes' x[:, :, 1:] (latent_upsampler.py:136-138).  A thread owns one 16-byte chunk of y; the trim is the `+ drop` on
// the output frame, so the source slice t*pt + p1 < drop is never touched.  lt / ls = log2(pt) / log2(ps) in {0, 1}.
__global__ void pixel_shuffle_nd_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int64_t T, int64_t H,
                                        int64_t W, int C, int lt, int ls, int drop, int64_t total_chunks) {
    const int64_t slots = C >> 3;
    const int64_t To = (T << lt) - drop, Ho = H << ls, Wo = W << ls;
    const int pmask_t = (1 << lt) - 1, pmask_s = (1 << ls) - 1;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total_chunks;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot = i % slots;
        int64_t r = i / slots;
        const int64_t xo = r % Wo; r /= Wo;
        const int64_t yo = r % Ho; r /= Ho;
        const int64_t to = r % To + drop;
        const int64_t b = r / To;
        const int64_t p = ((((to & pmask_t) << ls) + (yo & pmask_s)) << ls) + (xo & pmask_s);
        const int64_t pos = ((b * T + (to >> lt)) * H + (yo >> ls)) * W + (xo >> ls);
        const int64_t src = ((pos << (lt + 2 * ls)) + p) * C + slot * 8;
        *(u32x4*)(y + i * 8) = *(const u32x4*)(x + src);
    }
}

// ---------------------------------------------------------------- AdaIN (adain_filter_latent)
template <typename T> __device__ __forceinline__ float ld(const T* p, int64_t i);
template <> __device__ __forceinline__ float ld<float>(const float* p, int64_t i) { return p[i]; }
template <> __device__ __forceinline__ float ld<uint16_t>(const uint16_t* p, int64_t i) { return bf2f(p[i]); }
__device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void st(uint16_t* p, int64_t i, float v) { p[i] = f2bf(v); }
template <> __device__ __forceinline__ float ld<_Float16>(const _Float16* p, int64_t i) { return (float)p[i]; }
__device__ __forceinline__ void st(_Float16* p, int64_t i, float v) { p[i] = (_Float16)v; }

__device__ __forceinline__ void block_sum2(float& a, float& b) {
    __shared__ float red[2][UP_THREADS / 64];
    a = wave_sum(a);
    b = wave_sum(b);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    a = b = 0.f;
    for (int k = 0; k < UP_THREADS / 64; ++k) { a += red[0][k]; b += red[1][k]; }
}

// One block per (b, c): latents [B*C, n], reference [B*C, m] (NCDHW planes are contiguous).
// out = lerp(x, (x - mean_x) / sd_x * sd_r + mean_r, factor), sd = torch.std (unbiased).
template <typename T>
__global__ void adain_kernel(const T* __restrict__ x, const T* __restrict__ ref, T* __restrict__ out, int64_t n,
                             int64_t m, float factor) {
    const T* xp = x + (int64_t)blockIdx.x * n;
    const T* rp = ref + (int64_t)blockIdx.x * m;
    T* op = out + (int64_t)blockIdx.x * n;
    // two-pass statistics (mean, then centred squares): planes are small and L2-resident
    float sx = 0.f, sr = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += UP_THREADS) sx += ld(xp, i);
    for (int64_t i = threadIdx.x; i < m; i += UP_THREADS) sr += ld(rp, i);
    block_sum2(sx, sr);
    const float mx = sx / (float)n, mr = sr / (float)m;
    float qx = 0.f, qr = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += UP_THREADS) { const float d = ld(xp, i) - mx; qx += d * d; }
    for (int64_t i = threadIdx.x; i < m; i += UP_THREADS) { const float d = ld(rp, i) - mr; qr += d * d; }
    block_sum2(qx, qr);
    const float sdx = sqrtf(qx / (float)(n - 1)), sdr = sqrtf(qr / (float)(m - 1));
    const float scale = sdr / sdx;
    for (int64_t i = threadIdx.x; i < n; i += UP_THREADS) {
        const float v = ld(xp, i);
        const float tform = (v - mx) * scale + mr;
        st(op, i, v + factor * (tform - v));
    }
}

// Tile cross-fade of the tiled VAE paths: b[o, z, i] = a[o, La - extent + z, i] * (1 - z / extent) + b[o, z, i] * (z / extent)
// for z < extent, with both tensors viewed as [outer][L][inner] around the blended axis (vae.py:193-221 blend_z / _v / _h).
template <typename T>
__global__ void tile_blend_kernel(const T* __restrict__ a, T* __restrict__ b, int64_t outer, int64_t La, int64_t Lb,
                                  int64_t inner, int extent) {
    const int64_t total = outer * extent * inner;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx % inner, r = idx / inner;
        const int z = (int)(r % extent);
        const int64_t o = r / extent;
        // both weights rounded once, as the reference's Python doubles are when they meet the tensor: 1.0f - w would carry
        // w's rounding into a weight that is small near the end of the band (1e-6 of it at extent 33)
        const float w = (float)z / (float)extent, w1 = (float)(extent - z) / (float)extent;
        const int64_t ia = (o * La + (La - extent + z)) * inner + i, ib = (o * Lb + z) * inner + i;
        const float va = ld(a, ia), vb = ld(b, ib);
        st(b, ib, va * w1 + vb * w);
    }
}

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_groupnorm_silu_bf16(const void* x, void* y, const void* residual, int32_t samples, int64_t S,
                                         int32_t C, int32_t groups, const void* gamma, const void* beta, float eps,
                                         float* workspace, void* stream) {
    LTXMI_REQUIRE(x && y && gamma && beta && workspace, LTXMI_ERR_INVALID_ARG, "ltxmi_groupnorm_silu_bf16: NULL argument");
    LTXMI_REQUIRE(samples > 0 && S > 0 && C > 0 && groups > 0, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_groupnorm_silu_bf16: non-positive size");
    const int slots = C / 8;
    LTXMI_REQUIRE(C % 8 == 0 && slots <= UP_THREADS && (slots & (slots - 1)) == 0 && C % groups == 0,
                  LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_groupnorm_silu_bf16: C=%d must be 8 * 2^k <= 2048 and divisible by groups=%d", C, groups);
    hipStream_t s = (hipStream_t)stream;
    // ~2048 blocks over the (rows, samples) grid
    int64_t want = 2048 / samples;
    if (want < 1) want = 1;
    int64_t rpb = (S + want - 1) / want;
    const int rpi = UP_THREADS / slots;
    rpb = (rpb + rpi - 1) / rpi * rpi;
    const unsigned gx = (unsigned)((S + rpb - 1) / rpb);       // <= want = max(1, 2048 / samples)
    float* part = workspace;                                   // [samples][gx][C][2], every entry written by gn_stats
    float* stat = workspace + (int64_t)samples * want * C * 2; // [samples][groups][2]
    hipLaunchKernelGGL(gn_stats_kernel, dim3(gx, samples), dim3(UP_THREADS), 0, s, (const uint16_t*)x, part, S, C,
                       (int)rpb);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(samples * groups), dim3(UP_THREADS), 0, s, (const uint16_t*)x, part, stat,
                       C, groups, S, (int)gx, eps);
    const int64_t chunks = (int64_t)samples * S * slots;
    int64_t g = (chunks + UP_THREADS - 1) / UP_THREADS;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)g), dim3(UP_THREADS), 0, s, (const uint16_t*)x, (uint16_t*)y,
                       (const uint16_t*)residual, stat, (const uint16_t*)gamma, (const uint16_t*)beta, S, C, groups,
                       chunks);
    return check_launch("ltxmi_groupnorm_silu_bf16");
}

extern "C" int ltxmi_pixel_shuffle2d_ndhwc_bf16(const void* x, void* y, int64_t frames, int32_t H, int32_t W,
                                                int32_t C, void* stream) {
    LTXMI_REQUIRE(x && y, LTXMI_ERR_INVALID_ARG, "ltxmi_pixel_shuffle2d_ndhwc_bf16: NULL argument");
    LTXMI_REQUIRE(frames > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_pixel_shuffle2d_ndhwc_bf16: bad sizes (C=%d must be a multiple of 8)", C);
    const int64_t chunks = frames * 4 * H * W * (C / 8);
    int64_t g = (chunks + UP_THREADS - 1) / UP_THREADS;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(pixel_shuffle2d_kernel, dim3((unsigned)g), dim3(UP_THREADS), 0, (hipStream_t)stream,
                       (const uint16_t*)x, (uint16_t*)y, H, W, C, chunks);
    return check_launch("ltxmi_pixel_shuffle2d_ndhwc_bf16");
}

extern "C" int ltxmi_pixel_shuffle_nd_ndhwc_bf16(const void* x, void* y, int32_t B, int32_t T, int32_t H, int32_t W,
                                                 int32_t C, int32_t pt, int32_t ps, int32_t drop_first, void* stream) {
    LTXMI_REQUIRE(x && y, LTXMI_ERR_INVALID_ARG, "ltxmi_pixel_shuffle_nd_ndhwc_bf16: NULL argument");
    LTXMI_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_pixel_shuffle_nd_ndhwc_bf16: bad sizes (C=%d must be a multiple of 8)", C);
    LTXMI_REQUIRE((pt == 1 || pt == 2) && (ps == 1 || ps == 2) && pt * ps > 1, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_pixel_shuffle_nd_ndhwc_bf16: pt=%d, ps=%d must each be 1 or 2 and not both 1", pt, ps);
    LTXMI_REQUIRE((drop_first == 0 || drop_first == 1) && drop_first < pt, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_pixel_shuffle_nd_ndhwc_bf16: drop_first=%d must be 0 or 1, and 1 only with pt = 2", drop_first);
    const int64_t chunks = (int64_t)B * ((int64_t)pt * T - drop_first) * ps * H * ps * W * (C / 8);
    int64_t g = (chunks + UP_THREADS - 1) / UP_THREADS;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(pixel_shuffle_nd_kernel, dim3((unsigned)g), dim3(UP_THREADS), 0, (hipStream_t)stream,
                       (const uint16_t*)x, (uint16_t*)y, (int64_t)T, (int64_t)H, (int64_t)W, C, pt - 1, ps - 1, drop_first,
                       chunks);
    return check_launch("ltxmi_pixel_shuffle_nd_ndhwc_bf16");
}

extern "C" int ltxmi_tile_blend(const void* a, void* b, int32_t dtype, int64_t outer, int64_t len_a, int64_t len_b,
                                int64_t inner, int32_t extent, void* stream) {
    LTXMI_REQUIRE(dtype >= 0 && dtype <= 2, LTXMI_ERR_INVALID_ARG, "ltxmi_tile_blend: dtype %d not in {0 fp32, 1 bf16, 2 fp16}", dtype);
    LTXMI_REQUIRE(a && b, LTXMI_ERR_INVALID_ARG, "ltxmi_tile_blend: NULL argument");
    LTXMI_REQUIRE(outer > 0 && inner > 0 && extent > 0 && extent <= len_a && extent <= len_b, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_tile_blend: need outer, inner > 0 and 0 < extent <= both lengths (got %d, %lld, %lld)", extent,
                  (long long)len_a, (long long)len_b);
    const int64_t total = outer * extent * inner;
    const int grid = (int)((total + UP_THREADS - 1) / UP_THREADS < 65535 ? (total + UP_THREADS - 1) / UP_THREADS : 65535);
    if (dtype == 1)
        hipLaunchKernelGGL(tile_blend_kernel<uint16_t>, dim3(grid), dim3(UP_THREADS), 0, (hipStream_t)stream,
                           (const uint16_t*)a, (uint16_t*)b, outer, len_a, len_b, inner, extent);
    else if (dtype == 2)
        hipLaunchKernelGGL(tile_blend_kernel<_Float16>, dim3(grid), dim3(UP_THREADS), 0, (hipStream_t)stream,
                           (const _Float16*)a, (_Float16*)b, outer, len_a, len_b, inner, extent);
    else
        hipLaunchKernelGGL(tile_blend_kernel<float>, dim3(grid), dim3(UP_THREADS), 0, (hipStream_t)stream,
                           (const float*)a, (float*)b, outer, len_a, len_b, inner, extent);
    return check_launch("ltxmi_tile_blend");
}

extern "C" int ltxmi_adain_filter(const void* latents, const void* reference, void* out, int32_t is_bf16,
                                  int32_t planes, int64_t n, int64_t n_ref, float factor, void* stream) {
    LTXMI_REQUIRE(latents && reference && out, LTXMI_ERR_INVALID_ARG, "ltxmi_adain_filter: NULL argument");
    LTXMI_REQUIRE(planes > 0 && n > 1 && n_ref > 1, LTXMI_ERR_INVALID_ARG,
                  "ltxmi_adain_filter: need planes > 0 and more than one value per plane");
    if (is_bf16)
        hipLaunchKernelGGL(adain_kernel<uint16_t>, dim3(planes), dim3(UP_THREADS), 0, (hipStream_t)stream,
                           (const uint16_t*)latents, (const uint16_t*)reference, (uint16_t*)out, n, n_ref, factor);
    else
        hipLaunchKernelGGL(adain_kernel<float>, dim3(planes), dim3(UP_THREADS), 0, (hipStream_t)stream,
                           (const float*)latents, (const float*)reference, (float*)out, n, n_ref, factor);
    return check_launch("ltxmi_adain_filter");
}
