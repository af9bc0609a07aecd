// gemm_mx8_body.h -- what the MX-FP8 GEMM kernels share: C[M,N] = epilogue(sum_k (Aq 2^ea)[m,k] (Wq 2^ew)[n,k] + bias[n]) on the
// block-scaled MFMA of gfx950 (v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands: twice the bf16 rate per clock), fp32
// accumulation.  The kernels' arguments, the tile constants and the checks of ltxmi_gemm_mx8_args are here; the kernel's
// statements are gemm_mx8_kernel.inc, which gemm_mx8.hip includes into gemm_mx8_kernel<EPI, MXOUT> (include/ltxmi_mx.h) and
// gemm_mx8_rss.hip into the row-sum kernel (include/ltxmi_mx_attn.h).  gemm_mx8_pair2.hip (include/ltxmi_mx_lora.h) restates the
// K loop for two operand pairs and shares the epilogue's text, gemm_mx8_epilogue.inc.
//
// The tile kernel of gemm.hip carried over: 256 x 256 output tiles, 8 waves (2 x 4, 128 x 64 each), a K-tile of 128 e4m3 bytes
// per row -- as many LDS bytes per row as that kernel's 64 bf16 -- so the LDS image (128-byte rows, 16-byte chunk c of row r at
// slot c ^ (r & 7), the XOR applied to the LDS-DMA's SOURCE address and again on the read), the two stages with one
// __syncthreads() per K-tile are those of gemm_bf16_nt_kernel.
//
// The scaled 32x32x64 MFMA, as established with exact data by tests/test_gpu_mx8_kernels.py::test_layout_probe:
//   operand   lane l (r = l & 31, h = l >> 5) holds row r; bytes 0..15 of its 8 registers are k = 16 h + 0..15, bytes 16..31 are
//             k = 32 + 16 h + 0..15: the 16-byte chunks h and h + 2 of the row's 64 bytes, half of block 0 and half of block 1;
//   scale     lane l supplies the E8M0 byte of (row r, block h of the k-step) in bits [7:0] of the scale register (opsel 0);
//   C/D       the 32x32 bf16 map: column = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h.
// As in gemm.hip the WEIGHTS are the MFMA's A operand and the activations its B operand, so a lane holds 4 CONSECUTIVE output
// columns of one output row per register group (8-byte bf16 / 4-byte e4m3 stores), and the 32 columns of an MX output block are
// the 16 registers of one accumulator in the two lanes l, l ^ 32: the block amax is 15 in-lane maxima and one shuffle.
//
// A K-tile's scales are one 32-bit word per row (K % 128 == 0): each stage carries them behind the operand images, 256 + 256
// words, fetched by one 4-byte-per-lane LDS-DMA instruction per wave.
#pragma once
#include "epilogue.h"
#include "mx8.h"

namespace ltxmi {

typedef __attribute__((ext_vector_type(8))) int i32x8;      // one scaled-MFMA A/B fragment: 32 e4m3 bytes

struct Mx8Params {
    const uint8_t* A; int64_t lda; const uint8_t* As; int64_t lda_s;
    const uint8_t* W; int64_t ldw; const uint8_t* Ws; int64_t ldw_s;
    const uint16_t* bias;
    uint16_t* C; int64_t ldc;
    uint8_t* Cq; int64_t ldcq; uint8_t* Cs; int64_t ldc_s;
    int M, N, K;
    const uint16_t* R; int64_t ldr;
    const uint16_t* gate_table; const uint16_t* gate_temb; int64_t gate_ld; int rows_per_group;
    int tiles_m, tiles_n;
};
// the row-sum kernel's arguments: rss[m * rss_ld + n / 64] for the columns n < rss_cols (rss_cols % 64 == 0)
struct Mx8RssParams : Mx8Params {
    float* rss; int64_t rss_ld; int rss_cols;
};
// what the kernel text reads them through: a kernel without row sums compiles that (discarded) code against nothing
struct Mx8NoRss {
    float* rss; int64_t rss_ld; int rss_cols;
};
__device__ __forceinline__ const Mx8RssParams& mx8_rss(const Mx8RssParams& p) { return p; }
__device__ __forceinline__ Mx8NoRss mx8_rss(const Mx8Params&) { return Mx8NoRss{nullptr, 0, 0}; }

constexpr int MX_BM = 256, MX_BN = 256, MX_BK = 128;       // MX_BK: e4m3 elements = bytes of a row per K-tile
constexpr int MX_WAVES_M = 2, MX_WAVES_N = 4, MX_NW = MX_WAVES_M * MX_WAVES_N;
constexpr int MX_A_BYTES = MX_BM * MX_BK, MX_B_BYTES = MX_BN * MX_BK, MX_SC_BYTES = (MX_BM + MX_BN) * 4;
constexpr int MX_STAGE_BYTES = MX_A_BYTES + MX_B_BYTES + MX_SC_BYTES;
constexpr int MX_SMEM = 2 * MX_STAGE_BYTES;                 // 135168 B: one workgroup per CU
static_assert(MX_NW * 64 == MX_BM + MX_BN, "one scale word per row: one 4-byte LDS-DMA lane per row of the two images");

// ---- host: the checks of ltxmi_gemm_mx8_args (include/ltxmi_mx.h) and the kernel arguments they lead to, for every entry that
// takes the struct.  Returns LTXMI_OK with p filled, or the negative status with the error text set; nothing is launched.
static inline int mx8_check_args(const ltxmi_gemm_mx8_args* a, const char* what, Mx8Params& p) {
    LTXMI_REQUIRE(a && a->Aq && a->A_scales && a->Wq && a->W_scales, LTXMI_ERR_INVALID_ARG, "%s: NULL argument", what);
    LTXMI_REQUIRE((a->C != nullptr) != (a->Cq != nullptr), LTXMI_ERR_INVALID_ARG, "%s: exactly one of C and Cq must be set", what);
    LTXMI_REQUIRE(!a->Cq || a->C_scales, LTXMI_ERR_INVALID_ARG, "%s: Cq without C_scales", what);
    LTXMI_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, LTXMI_ERR_INVALID_ARG, "%s: non-positive size M=%d N=%d K=%d", what, a->M, a->N,
                  a->K);
    const bool epi_ok = a->epilogue == LTXMI_EPI_NONE || a->epilogue == LTXMI_EPI_GELU_TANH ||
                        (a->epilogue == LTXMI_EPI_GATE_RESIDUAL && !a->Cq);
    LTXMI_REQUIRE(epi_ok, LTXMI_ERR_INVALID_ARG, "%s: bad epilogue %d%s", what, a->epilogue, a->Cq ? " for the MX output" : "");
    const bool resid = a->epilogue == LTXMI_EPI_GATE_RESIDUAL;
    if (resid) {
        LTXMI_REQUIRE(a->residual && a->ldr >= a->N && a->ldr % 4 == 0, LTXMI_ERR_INVALID_ARG,
                      "%s: GATE_RESIDUAL needs a residual with ldr >= N, ldr %% 4 == 0", what);
        if (a->gate_table)
            LTXMI_REQUIRE(a->gate_temb && a->rows_per_group > 0 && a->gate_ld % 4 == 0, LTXMI_ERR_INVALID_ARG,
                          "%s: gate_table given without gate_temb / rows_per_group", what);
    }
    LTXMI_REQUIRE(a->K % MX_BK == 0, LTXMI_ERR_UNSUPPORTED, "%s: K=%d must be a multiple of 128", what, a->K);
    LTXMI_REQUIRE(a->N % LTXMI_MX_BLOCK == 0, LTXMI_ERR_UNSUPPORTED, "%s: N=%d must be a multiple of 32", what, a->N);
    const int kb = a->K / LTXMI_MX_BLOCK, nblk = a->N / LTXMI_MX_BLOCK;
    LTXMI_REQUIRE(a->lda % 16 == 0 && a->ldw % 16 == 0 && a->lda >= a->K && a->ldw >= a->K &&
                      (((uintptr_t)a->Aq | (uintptr_t)a->Wq) & 15) == 0,
                  LTXMI_ERR_UNSUPPORTED, "%s: Aq and Wq must be 16-byte aligned with lda, ldw %% 16 == 0 and >= K", what);
    LTXMI_REQUIRE((int64_t)MX_BM * a->lda < (1ll << 31) && (int64_t)MX_BN * a->ldw < (1ll << 31), LTXMI_ERR_UNSUPPORTED,
                  "%s: 256 rows of Aq / Wq must span less than 2^31 bytes", what);
    LTXMI_REQUIRE(a->lda_s % 4 == 0 && a->ldw_s % 4 == 0 && a->lda_s >= kb && a->ldw_s >= kb &&
                      (((uintptr_t)a->A_scales | (uintptr_t)a->W_scales) & 3) == 0,
                  LTXMI_ERR_UNSUPPORTED, "%s: the scale arrays must be 4-byte aligned with lda_s, ldw_s %% 4 == 0 and >= K / 32", what);
    LTXMI_REQUIRE((((uintptr_t)a->bias) & 7) == 0, LTXMI_ERR_UNSUPPORTED, "%s: bias must be 8-byte aligned", what);
    if (a->C)
        LTXMI_REQUIRE(a->ldc % 4 == 0 && a->ldc >= a->N && (((uintptr_t)a->C) & 7) == 0, LTXMI_ERR_UNSUPPORTED,
                      "%s: C must be 8-byte aligned with ldc %% 4 == 0 and >= N", what);
    else
        LTXMI_REQUIRE(a->ldcq % 4 == 0 && a->ldcq >= a->N && a->ldc_s >= nblk && (((uintptr_t)a->Cq) & 3) == 0, LTXMI_ERR_UNSUPPORTED,
                      "%s: Cq must be 4-byte aligned with ldcq %% 4 == 0 and >= N, ldc_s >= N / 32", what);
    // the stores go through 32-bit offsets into descriptors that end with the last element; a masked lane stores at 0xfffffff0
    // (+ at most 48), which has to lie outside every descriptor
    constexpr int64_t SPAN = (1ll << 32) - 256;
    LTXMI_REQUIRE(a->C ? (int64_t)a->M * a->ldc * 2 < SPAN : ((int64_t)a->M * a->ldcq < SPAN && (int64_t)a->M * a->ldc_s < SPAN),
                  LTXMI_ERR_UNSUPPORTED, "%s: the output (and its scales) must span less than 2^32 - 256 bytes", what);
    if (resid)
        LTXMI_REQUIRE((((uintptr_t)a->residual | (uintptr_t)a->gate_table | (a->gate_table ? (uintptr_t)a->gate_temb : (uintptr_t)0)) & 7) == 0,
                      LTXMI_ERR_UNSUPPORTED, "%s: residual, gate_table and gate_temb must be 8-byte aligned", what);
    p = Mx8Params{};
    p.A = (const uint8_t*)a->Aq; p.lda = a->lda; p.As = (const uint8_t*)a->A_scales; p.lda_s = a->lda_s;
    p.W = (const uint8_t*)a->Wq; p.ldw = a->ldw; p.Ws = (const uint8_t*)a->W_scales; p.ldw_s = a->ldw_s;
    p.bias = (const uint16_t*)a->bias;
    p.C = (uint16_t*)a->C; p.ldc = a->ldc;
    p.Cq = (uint8_t*)a->Cq; p.ldcq = a->ldcq; p.Cs = (uint8_t*)a->C_scales; p.ldc_s = a->ldc_s;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.R = (const uint16_t*)a->residual; p.ldr = a->ldr;
    p.gate_table = (const uint16_t*)a->gate_table; p.gate_temb = (const uint16_t*)a->gate_temb; p.gate_ld = a->gate_ld;
    p.rows_per_group = a->rows_per_group > 0 ? a->rows_per_group : 1;
    p.tiles_m = (a->M + MX_BM - 1) / MX_BM;
    p.tiles_n = (a->N + MX_BN - 1) / MX_BN;
    LTXMI_REQUIRE((int64_t)p.tiles_m * p.tiles_n < (1ll << 31), LTXMI_ERR_UNSUPPORTED, "%s: too many tiles", what);
    return LTXMI_OK;
}

// ---- host: the checks of the row sums of squares (include/ltxmi_mx_attn.h) for a struct mx8_check_args has passed; fills p's
// three fields
static inline int mx8_check_rss(const ltxmi_gemm_mx8_args* a, float* rowsumsq, int32_t rowsumsq_cols, int64_t rowsumsq_ld,
                                const char* what, Mx8RssParams& p) {
    LTXMI_REQUIRE(rowsumsq, LTXMI_ERR_INVALID_ARG, "%s: NULL rowsumsq", what);
    LTXMI_REQUIRE(a->epilogue == LTXMI_EPI_NONE && !a->Cq, LTXMI_ERR_INVALID_ARG,
                  "%s: the row sums go with epilogue NONE and a bf16 C (epilogue %d%s)", what, a->epilogue, a->Cq ? ", Cq set" : "");
    LTXMI_REQUIRE(rowsumsq_cols > 0 && rowsumsq_cols % 64 == 0 && rowsumsq_cols <= a->N, LTXMI_ERR_INVALID_ARG,
                  "%s: rowsumsq_cols=%d must be a positive multiple of 64 and <= N=%d", what, rowsumsq_cols, a->N);
    LTXMI_REQUIRE(rowsumsq_ld >= rowsumsq_cols / 64, LTXMI_ERR_INVALID_ARG, "%s: rowsumsq_ld=%lld is shorter than rowsumsq_cols / 64 = %d",
                  what, (long long)rowsumsq_ld, rowsumsq_cols / 64);
    LTXMI_REQUIRE((((uintptr_t)rowsumsq) & 3) == 0, LTXMI_ERR_UNSUPPORTED, "%s: rowsumsq must be 4-byte aligned", what);
    // a masked lane stores at 0xfffffff0, which has to lie outside the descriptor (above)
    LTXMI_REQUIRE((int64_t)a->M * rowsumsq_ld * 4 < (1ll << 32) - 256, LTXMI_ERR_UNSUPPORTED,
                  "%s: rowsumsq must span less than 2^32 - 256 bytes", what);
    p.rss = rowsumsq; p.rss_ld = rowsumsq_ld; p.rss_cols = rowsumsq_cols;
    return LTXMI_OK;
}

}  // namespace ltxmi
