// quant_mx8.hip -- bf16 rows -> MX-FP8 (e4m3 elements, one E8M0 scale byte per 32 elements of a row; include/ltxmi_mx.h).
// One wave per row as the row kernels of rowops.hip: lane l owns the 8-element chunks l, l + 64, ... (16-byte loads, 8-byte
// stores), four neighbouring lanes own one block and agree on its amax with two shuffles.  Every input byte is read once.
#include "mx8.h"
#include "rows.h"

namespace ltxmi {

__global__ __launch_bounds__(256) void quantize_mx8_kernel(const uint16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ q,
                                                           int64_t ldq, uint8_t* __restrict__ sc, int64_t lds, int rows, int K) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint16_t* xr = x + (int64_t)row * ldx;
    uint8_t* qr = q + (int64_t)row * ldq;
    uint8_t* sr = sc + (int64_t)row * lds;
    const int nchunk = K >> 3;             // a multiple of 4: the four lanes of a block are in the loop together
    for (int ch = lane; ch < nchunk; ch += 64) {
        const u32x4 w = *(const u32x4*)(xr + ch * 8);
        uint32_t am = 0;                   // |x| as bf16 bits: their integer order is the values' order
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            am = max(am, w[i] & 0x7fffu);
            am = max(am, (w[i] >> 16) & 0x7fffu);
        }
        am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
        am = max(am, (uint32_t)__shfl_xor((int)am, 2, 64));
        const int byte = mx8_scale_byte(am << 16);
        const float inv = mx8_inv_scale(byte);
        u32x2 o;
        o[0] = mx8_pack4(bf_lo(w[0]), bf_hi(w[0]), bf_lo(w[1]), bf_hi(w[1]), inv);
        o[1] = mx8_pack4(bf_lo(w[2]), bf_hi(w[2]), bf_lo(w[3]), bf_hi(w[3]), inv);
        *(u32x2*)(qr + ch * 8) = o;
        if ((lane & 3) == 0) sr[ch >> 2] = (uint8_t)byte;
    }
}

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_quantize_mx8_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int32_t rows,
                                       int32_t K, void* stream) {
    LTXMI_REQUIRE(x && q && scales, LTXMI_ERR_INVALID_ARG, "ltxmi_quantize_mx8_bf16: NULL argument");
    LTXMI_REQUIRE(rows > 0 && K > 0, LTXMI_ERR_INVALID_ARG, "ltxmi_quantize_mx8_bf16: non-positive size rows=%d K=%d", rows, K);
    LTXMI_REQUIRE(K % LTXMI_MX_BLOCK == 0, LTXMI_ERR_UNSUPPORTED, "ltxmi_quantize_mx8_bf16: K=%d must be a multiple of 32", K);
    LTXMI_REQUIRE(row_stride_ok(ldx, K) && ldq % 16 == 0 && ldq >= K && lds >= K / LTXMI_MX_BLOCK, LTXMI_ERR_UNSUPPORTED,
                  "ltxmi_quantize_mx8_bf16: ldx %% 8, ldq %% 16 and every stride >= its row (ldx=%lld ldq=%lld lds=%lld K=%d)",
                  (long long)ldx, (long long)ldq, (long long)lds, K);
    LTXMI_REQUIRE(aligned16(x, q), LTXMI_ERR_UNSUPPORTED, "ltxmi_quantize_mx8_bf16: x and q must be 16-byte aligned");
    const int64_t grid = ((int64_t)rows + ROWS_PER_WG - 1) / ROWS_PER_WG;
    hipLaunchKernelGGL(quantize_mx8_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, ldx,
                       (uint8_t*)q, ldq, (uint8_t*)scales, lds, rows, K);
    return check_launch("ltxmi_quantize_mx8_bf16");
}
