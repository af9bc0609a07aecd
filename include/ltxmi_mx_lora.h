/*
 * ltxmi_mx_lora.h -- fourth extension header of libltxmi.so: LoRA adapters applied unmerged on MX-FP8 linears.
 *
 * include/ltxmi.h is the frozen base ABI, include/ltxmi_mx.h the first extension (the number format, the quantiser, the GEMM
 * and its argument struct, which the entry below reuses unchanged), include/ltxmi_mx_attn.h the second (the row sums of
 * squares); the conventions are theirs (device pointers, `stream` a hipStream_t passed as void*, 0 = LTXMI_OK / negative =
 * ltxmi_status with the text in ltxmi_last_error(), "ld*" row strides in ELEMENTS of the array they belong to).  The header is
 * written in the subset ltxmi/_abi.py reads; ltxmi/_lib_mxl.py binds it.  LTXMI_MXL_VERSION counts this header's own
 * revisions; the library's version string is that of ltxmi.h.
 */
#ifndef LTXMI_MX_LORA_H
#define LTXMI_MX_LORA_H

#include "ltxmi_mx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LTXMI_MXL_VERSION "1"

/* The second operand pair of ltxmi_gemm_mx8_pair2, both sides in MX-FP8 like the first: what ltxmi_gemm_pair is to
 * ltxmi_gemm_bf16.  A2q = MX(x . down^T) [M, groups * K2] (ltxmi_gemm_mx8 with Cq output), W2q = the quantised scaled up
 * matrices [N, K2]; output column n reads the K2 columns of A2q from g * K2 on, g = n / group_cols. */
typedef struct ltxmi_gemm_mx8_pair {
    const void* A2q;       int64_t lda2;    /* [M, groups*K2] e4m3                                */
    const void* A2_scales; int64_t lda2_s;  /* [M, groups*K2/32] E8M0                             */
    const void* W2q;       int64_t ldw2;    /* [N, K2] e4m3                                       */
    const void* W2_scales; int64_t ldw2_s;  /* [N, K2/32] E8M0                                    */
    int32_t K2;                             /* multiple of 128                                    */
    int32_t group_cols;                     /* 0 (one group) or a multiple of 256 that divides N  */
} ltxmi_gemm_mx8_pair;

/* C[M,N] = epilogue( Aq . Wq^T + A2q[:, g K2 .. (g+1) K2) . W2q^T + bias ), g = n / group_cols: ltxmi_gemm_mx8 with the pair's
 * K2 / 128 K-tiles accumulated behind the K / 128 of `args` into the same fp32 accumulators, in that order.  The result is bit
 * for bit what ltxmi_gemm_mx8 (with rowsumsq: ltxmi_gemm_mx8_rowsumsq) gives on the materialised concatenation [Aq | A2q_g],
 * [Wq | W2q] with K + K2.  Every output form and epilogue of ltxmi_gemm_mx8 is taken; with a non-NULL rowsumsq the call is
 * ltxmi_gemm_mx8_rowsumsq's (epilogue NONE, bf16 C) and the three arguments have its meaning, with a NULL rowsumsq they are
 * ignored.  Replaces, on a quantised linear, base_layer(x) + lora_B(lora_A(x)) * scaling of an unmerged adapter.
 * Refuses everything ltxmi_gemm_mx8 refuses for `args` and, with rowsumsq, everything ltxmi_gemm_mx8_rowsumsq refuses, and
 * LTXMI_ERR_INVALID_ARG: a NULL pair, A2q, A2_scales, W2q or W2_scales; K2 <= 0 or K2 % 128 != 0; group_cols < 0, % 256 != 0
 * or not dividing N.
 * LTXMI_ERR_UNSUPPORTED: lda2 or ldw2 % 16 != 0, lda2 < groups * K2, ldw2 < K2; lda2_s or ldw2_s % 4 != 0, lda2_s < groups *
 * K2 / 32, ldw2_s < K2 / 32; A2q or W2q not 16-byte aligned, A2_scales or W2_scales not 4-byte aligned; 256 rows of A2q, W2q
 * or of any of the four scale arrays spanning 2^31 bytes or more.
 * All of it is checked before anything is launched, without a device.  There is one kernel form (256 x 256 tiles). */
int ltxmi_gemm_mx8_pair2(const ltxmi_gemm_mx8_args* args, const ltxmi_gemm_mx8_pair* pair, float* rowsumsq,
                         int32_t rowsumsq_cols, int64_t rowsumsq_ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LTXMI_MX_LORA_H */
