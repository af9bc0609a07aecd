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
    LTXMI_REQUIRE(rowsumsq, LTXMI_ERR_INVALID_ARG, "%s: NULL rowsumsq", what);
    LTXMI_REQUIRE(a->epilogue == LTXMI_EPI_NONE && !a->Cq, LTXMI_ERR_INVALID_ARG,
                  "%s: the row sums go with epilogue NONE and a bf16 C (epilogue %d%s)", what, a->epilogue, a->Cq ? ", Cq set" : "");
    LTXMI_REQUIRE(rowsumsq_cols > 0 && rowsumsq_cols % 64 == 0 && rowsumsq_cols <= a->N, LTXMI_ERR_INVALID_ARG,
                  "%s: rowsumsq_cols=%d must be a positive multiple of 64 and <= N=%d", what, rowsumsq_cols, a->N);
    LTXMI_REQUIRE(rowsumsq_ld >= rowsumsq_cols / 64, LTXMI_ERR_INVALID_ARG, "%s: rowsumsq_ld=%lld is shorter than rowsumsq_cols / 64 = %d",
                  what, (long long)rowsumsq_ld, rowsumsq_cols / 64);
    LTXMI_REQUIRE((((uintptr_t)rowsumsq) & 3) == 0, LTXMI_ERR_UNSUPPORTED, "%s: rowsumsq must be 4-byte aligned", what);
    // a masked lane stores at 0xfffffff0, which has to lie outside the descriptor (gemm_mx8_body.h)
    LTXMI_REQUIRE((int64_t)a->M * rowsumsq_ld * 4 < (1ll << 32) - 256, LTXMI_ERR_UNSUPPORTED,
                  "%s: rowsumsq must span less than 2^32 - 256 bytes", what);
    p.rss = rowsumsq; p.rss_ld = rowsumsq_ld; p.rss_cols = rowsumsq_cols;
    return launch_with_lds<gemm_mx8_rowsumsq_kernel>(p, dim3(p.tiles_m * p.tiles_n), dim3(MX_NW * 64), MX_SMEM, (hipStream_t)stream, what);
}
