// gemm_mx8_rss.hip -- ltxmi_gemm_mx8_rowsumsq (include/ltxmi_mx_attn.h): the plain bf16-output form of the MX-FP8 GEMM kernel
// (gemm_mx8_body.h, gemm_mx8_kernel.inc) with its row-sum flag on.  A wave's 128 x 64 sub-tile is one 64-column block per row,
// so the sum of squares of a row's stored bf16 values is 32 in-lane squares, one shuffle with the lane 32 away and one 4-byte
// store.
#include "gemm_mx8_body.h"
#include "../../include/ltxmi_mx_attn.h"

namespace ltxmi {

__global__ __launch_bounds__(MX_NW * 64) void gemm_mx8_rowsumsq_kernel(Mx8RssParams p) {
    constexpr int EPI = LTXMI_EPI_NONE;
    constexpr bool MXOUT = false, RSS = true;
#include "gemm_mx8_kernel.inc"
}

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_gemm_mx8_rowsumsq(const ltxmi_gemm_mx8_args* a, float* rowsumsq, int32_t rowsumsq_cols, int64_t rowsumsq_ld,
                                       void* stream) {
    const char* what = "ltxmi_gemm_mx8_rowsumsq";
    Mx8RssParams p;
    if (const int rc = mx8_check_args(a, what, p)) return rc;
    if (const int rc = mx8_check_rss(a, rowsumsq, rowsumsq_cols, rowsumsq_ld, what, p)) return rc;
    return launch_with_lds<gemm_mx8_rowsumsq_kernel>(p, dim3(p.tiles_m * p.tiles_n), dim3(MX_NW * 64), MX_SMEM, (hipStream_t)stream, what);
}
