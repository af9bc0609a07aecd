/*
 * ltxmi_mx_t5.h -- third extension header of libltxmi.so: what the MX-FP8 T5 text encoder needs beside ltxmi_mx.h.
 *
 * include/ltxmi.h is the frozen base ABI, include/ltxmi_mx.h the first extension (the number format, the quantiser, the GEMM and
 * its argument struct, which the entries below reuse unchanged) and include/ltxmi_mx_attn.h the second; the conventions are
 * theirs (device pointers, `stream` a hipStream_t passed as void*, 0 = LTXMI_OK / negative = ltxmi_status with the text in
 * ltxmi_last_error(), "ld*" row strides in ELEMENTS of the array they belong to).  The header is written in the subset
 * ltxmi/_abi.py reads; ltxmi/_lib_mxt.py binds it.  LTXMI_MXT_VERSION counts this header's own revisions; the library's version
 * string is that of ltxmi.h.
 */
#ifndef LTXMI_MX_T5_H
#define LTXMI_MX_T5_H

#include "ltxmi_mx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LTXMI_MXT_VERSION "1"

/* The tile forms of ltxmi_gemm_mx8_skinny (rows of activations x columns of weights per workgroup), the depth of their LDS
 * ring in K-tiles of 128, and the entry's row limit. */
#define LTXMI_MXT_FORM_AUTO 0
#define LTXMI_MXT_FORM_128X64 1
#define LTXMI_MXT_FORM_64X64 2
#define LTXMI_MXT_STAGES 3
#define LTXMI_MXT_MAX_ROWS 512

/* ltxmi_gemm_mx8 for few rows (M <= LTXMI_MXT_MAX_ROWS): the projections of the T5 encoder (q/k/v, o, wi_0/wi_1, wo of
 * transformers' modeling_t5.py, which the reference pipeline calls at pipeline_ltx_video.py:405-417) when the encoder is
 * quantised.  Small output tiles, each walking all of K in one workgroup through a ring of LTXMI_MXT_STAGES K-tiles; the k-steps
 * go in ascending order into one fp32 accumulator with the operand and scale lane maps of ltxmi_gemm_mx8, so C is bit-identical
 * to ltxmi_gemm_mx8's for the same struct.
 * form: LTXMI_MXT_FORM_AUTO chooses by shape (128 x 64 tiles where M > 256 and they make at least 256 workgroups, else 64 x 64:
 * the measured choice at the T5 shapes);
 * another value forces that form.  Both forms run every shape the entry accepts.
 * Refuses everything ltxmi_gemm_mx8 refuses for the same struct, and
 * LTXMI_ERR_UNSUPPORTED: M > LTXMI_MXT_MAX_ROWS; Cq set (bf16 output only); an epilogue other than NONE and GATE_RESIDUAL; a
 * gate_table; a bias together with GATE_RESIDUAL (the order of the two additions in ltxmi_gemm_mx8 is its compiler's choice);
 * a form that names no tile form.
 * All of it is checked before anything is launched, without a device. */
int ltxmi_gemm_mx8_skinny(const ltxmi_gemm_mx8_args* args, int32_t form, void* stream);

/* The checks and the plan of ltxmi_gemm_mx8_skinny without the launch (host arithmetic only): the form id that would run
 * (> 0), or the negative status with the error text set. */
int ltxmi_gemm_mx8_skinny_form(const ltxmi_gemm_mx8_args* args, int32_t form);

/* ltxmi_rmsnorm_weight_bf16 followed by ltxmi_quantize_mx8_bf16 in one row pass: T5LayerNorm (modeling_t5.py) whose row
 * y = bf16(bf16(x * rstd) * weight) leaves as q [rows, D] e4m3 and scales [rows, D / 32] E8M0.  Bit-identical to the two
 * launches (the row factor is summed in ltxmi_rmsnorm_weight_bf16's order); the bf16 y is never written.
 * LTXMI_ERR_INVALID_ARG: a NULL pointer, non-positive rows or D.
 * LTXMI_ERR_UNSUPPORTED: D % 32 != 0 or D > 8192; ldx % 8 != 0; ldq % 16 != 0; a stride shorter than its row (ldx, ldq < D,
 * lds < D / 32); x, q or weight not 16-byte aligned; more than 4 * (2^24 - 1) rows. */
int ltxmi_rmsnorm_weight_mx8(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds,
                             int32_t rows, int32_t D, const void* weight, float eps, void* stream);

/* ltxmi_gated_gelu_bf16 followed by ltxmi_quantize_mx8_bf16 in one pass: h [rows, 2F] bf16 (the output of the stacked
 * [wi_0; wi_1] projection) -> y = bf16(bf16(gelu_tanh(h[:, :F])) * h[:, F:]) as q [rows, F] e4m3 and scales [rows, F / 32]
 * E8M0 (T5DenseGatedActDense of modeling_t5.py in front of wo).  Bit-identical to the two launches; the bf16 y is never written.
 * LTXMI_ERR_INVALID_ARG: a NULL pointer, non-positive rows or F.
 * LTXMI_ERR_UNSUPPORTED: F % 32 != 0; ldh % 8 != 0 or < 2 F; ldq % 16 != 0 or < F; lds < F / 32; h or q not 16-byte aligned. */
int ltxmi_gated_gelu_mx8(const void* h, int64_t ldh, void* q, int64_t ldq, void* scales, int64_t lds,
                         int32_t rows, int32_t F, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LTXMI_MX_T5_H */
