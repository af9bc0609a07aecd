// gemm_mx8.hip -- ltxmi_gemm_mx8 (include/ltxmi_mx.h): the six instances of the MX-FP8 GEMM kernel; gemm_mx8_body.h says how it
// works.
#include "gemm_mx8_body.h"

namespace ltxmi {

// MXOUT: write e4m3 + scales (Cq, Cs) instead of bf16 (C)
template <int EPI, bool MXOUT>
__global__ __launch_bounds__(MX_NW * 64) void gemm_mx8_kernel(Mx8Params p) {
    constexpr bool RSS = false;
#include "gemm_mx8_kernel.inc"
}

template <bool MXOUT>
static int launch_mx8(const Mx8Params& p, int epi, hipStream_t stream, const char* what) {
    const int grid = p.tiles_m * p.tiles_n;
    auto go = [&](auto e) {
        return launch_with_lds<gemm_mx8_kernel<decltype(e)::value, MXOUT>>(p, dim3(grid), dim3(MX_NW * 64), MX_SMEM, stream, what);
    };
    switch (epi) {
        case LTXMI_EPI_NONE: return go(epi_t<LTXMI_EPI_NONE>{});
        case LTXMI_EPI_GELU_TANH: return go(epi_t<LTXMI_EPI_GELU_TANH>{});
        default: break;
    }
    if constexpr (!MXOUT) {
        if (epi == LTXMI_EPI_GATE_RESIDUAL) return go(epi_t<LTXMI_EPI_GATE_RESIDUAL>{});
        if (epi == EPI_RESIDUAL) return go(epi_t<EPI_RESIDUAL>{});
    }
    set_error("%s: bad epilogue %d", what, epi);
    return LTXMI_ERR_INVALID_ARG;
}

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_gemm_mx8(const ltxmi_gemm_mx8_args* a, void* stream) {
    const char* what = "ltxmi_gemm_mx8";
    Mx8Params p;
    if (const int rc = mx8_check_args(a, what, p)) return rc;
    const int epi = (a->epilogue == LTXMI_EPI_GATE_RESIDUAL && !a->gate_table) ? EPI_RESIDUAL : a->epilogue;
    return a->Cq ? launch_mx8<true>(p, epi, (hipStream_t)stream, what) : launch_mx8<false>(p, epi, (hipStream_t)stream, what);
}
