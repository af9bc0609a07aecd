/*
 * ltxmi_mx_attn.h -- second extension header of libltxmi.so: what the MX-FP8 attention projections need beside ltxmi_mx.h.
 *
 * include/ltxmi.h is the frozen base ABI and include/ltxmi_mx.h the first extension (the number format, the quantiser, the GEMM
 * and its argument struct, which the entries below reuse unchanged); the conventions are theirs (device pointers, `stream` a
 * hipStream_t passed as void*, 0 = LTXMI_OK / negative = ltxmi_status with the text in ltxmi_last_error(), "ld*" row strides in
 * ELEMENTS of the array they belong to).  The header is written in the subset ltxmi/_abi.py reads; ltxmi/_lib_mxa.py binds it.
 * LTXMI_MXA_VERSION counts this header's own revisions; the library's version string is that of ltxmi.h.
 */
#ifndef LTXMI_MX_ATTN_H
#define LTXMI_MX_ATTN_H

#include "ltxmi_mx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LTXMI_MXA_VERSION "1"

/* ltxmi_gemm_mx8 with epilogue NONE and a bf16 C, plus, for the output columns < rowsumsq_cols,
 * rowsumsq[m * rowsumsq_ld + n / 64] = sum over that 64-column block of (bf16 C[m, n])^2 in fp32:
 * the meaning of ltxmi_gemm_args.rowsumsq.  Replaces the packed q/k/v projection of a block's self-attention and to_q of its
 * cross-attention (ltx_video/models/transformers/attention.py:1040) when the model's attention is quantised: the sums are
 * what q's RMSNorm (:1041) is computed from.  Blocks at or past rowsumsq_cols and rows at or past M are not written.
 * Refuses everything ltxmi_gemm_mx8 refuses for the same struct, and
 * LTXMI_ERR_INVALID_ARG: a NULL rowsumsq; an epilogue other than NONE; Cq set; rowsumsq_cols <= 0, % 64 != 0 or > N;
 * rowsumsq_ld < rowsumsq_cols / 64.
 * LTXMI_ERR_UNSUPPORTED: rowsumsq not 4-byte aligned; M * rowsumsq_ld * 4 bytes of 2^32 - 256 or more.
 * All of it is checked before anything is launched, without a device. */
int ltxmi_gemm_mx8_rowsumsq(const ltxmi_gemm_mx8_args* args, float* rowsumsq, int32_t rowsumsq_cols,
                            int64_t rowsumsq_ld, void* stream);

/* ltxmi_norm_modulate_bf16 followed by ltxmi_quantize_mx8_bf16 in one row pass: y is rounded to bf16,
 * then quantised by the rule of ltxmi_mx.h; q [rows, D] e4m3, scales [rows, D / 32] E8M0.
 * Bit-identical to the two launches; the bf16 y is never written.  Replaces norm1 and the modulation in front of a block's
 * self-attention (ltx_video/models/transformers/attention.py:233-252) when attn1's q/k/v projection is quantised.
 * LTXMI_ERR_INVALID_ARG: a NULL pointer, non-positive rows, D or rows_per_group, a kind outside ltxmi_norm_kind.
 * LTXMI_ERR_UNSUPPORTED: D % 32 != 0 or D > 8192; ldx or temb_ld % 8 != 0; ldq % 16 != 0; a stride shorter than its row
 * (ldx, ldq < D, lds < D / 32); x or q not 16-byte aligned. */
int ltxmi_norm_modulate_mx8(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds,
                            int32_t rows, int32_t D, float eps, int32_t kind,
                            const void* scale_table, const void* scale_temb,
                            const void* shift_table, const void* shift_temb,
                            int64_t temb_ld, int32_t rows_per_group, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LTXMI_MX_ATTN_H */
