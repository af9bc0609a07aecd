/*
 * ltxmi_mx.h -- extension header of libltxmi.so: the MX-FP8 (OCP microscaling, e4m3 elements) entries.
 *
 * include/ltxmi.h is the frozen base ABI; the entries below are exported by the same library and follow the same
 * conventions (device pointers, `stream` a hipStream_t passed as void*, 0 = LTXMI_OK / negative = ltxmi_status with the text in
 * ltxmi_last_error(), argument structs zero-initialised, "ld*" row strides in ELEMENTS of the array they belong to).  The
 * header is written in the subset ltxmi/_abi.py reads; ltxmi/_lib_mx.py binds it.  LTXMI_MX_VERSION counts this header's own
 * revisions; the library's version string is that of ltxmi.h.
 *
 * The number format
 *   block     32 consecutive elements along K of one row;
 *   scale     one E8M0 byte per block, byte = e + 127, the block's values are q * 2^e;
 *   e         the smallest integer with amax * 2^-e <= 448, read from the bits of amax = m * 2^k, m in [1, 2):
 *             e = k - 8 if m <= 1.75 else k - 7, clamped to [-127, 127]; an all-zero block has byte 0 and elements 0;
 *   elements  OCP e4m3fn, q = RNE(x * 2^-e) (saturating at +-448, which the rule above never reaches).
 */
#ifndef LTXMI_MX_H
#define LTXMI_MX_H

#include "ltxmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LTXMI_MX_VERSION "1"
#define LTXMI_MX_BLOCK 32

/* x [rows, K] bf16 (row stride ldx) -> q [rows, K] e4m3 bytes (row stride ldq) and scales [rows, K / 32] E8M0 bytes (row stride
 * lds).  One row pass: every byte of x is read once.  Replaces nothing of the reference (its quantised mode is a checkpoint
 * format, inference.py:96-100); it feeds ltxmi_gemm_mx8 with the weights (once) and with FF1's input (every call).
 * LTXMI_ERR_INVALID_ARG: a NULL pointer, non-positive rows or K.  LTXMI_ERR_UNSUPPORTED: K % 32 != 0, x not 16-byte aligned or
 * ldx % 8 != 0, q not 16-byte aligned or ldq % 16 != 0, a stride shorter than its row (ldx, ldq < K, lds < K / 32). */
int ltxmi_quantize_mx8_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int32_t rows,
                            int32_t K, void* stream);

/* C[M,N] = epilogue( sum_k (Aq * 2^ea)[m,k] * (Wq * 2^ew)[n,k] + bias[n] ), fp32 accumulation on the block-scaled MFMA
 * (v_mfma_scale_f32_32x32x64_f8f6f4, e4m3 operands).  Replaces ff.net[0] (Linear + GELU-tanh) and ff.net[2] of a block
 * (ltx_video/models/transformers/attention.py:339-340) with the gate and residual that follow (:345-351) when the model's
 * feed-forward is quantised.
 * Output, one of
 *   C  (bf16)         epilogue NONE, GELU_TANH or GATE_RESIDUAL, with the meaning, the fields and the gate indexing of
 *                     ltxmi_gemm_args;
 *   Cq + C_scales     epilogue NONE or GELU_TANH: the fp32 value (no bf16 rounding in between) is quantised by the rule above
 *                     over each 32-column block of a row and stored as e4m3 bytes [M,N] and E8M0 bytes [M,N/32].
 * LTXMI_ERR_INVALID_ARG: a NULL Aq, A_scales, Wq or W_scales; neither or both of C and Cq; Cq without C_scales; non-positive M, N
 * or K; an epilogue outside {NONE, GELU_TANH, GATE_RESIDUAL}, GATE_RESIDUAL with Cq; GATE_RESIDUAL without a residual or with
 * ldr < N or ldr % 4 != 0; a gate_table without gate_temb, with rows_per_group <= 0 or gate_ld % 4 != 0.
 * LTXMI_ERR_UNSUPPORTED: K % 128 != 0, N % 32 != 0; Aq or Wq not 16-byte aligned, lda or ldw % 16 != 0 or < K; a scale array not
 * 4-byte aligned, lda_s or ldw_s % 4 != 0 or < K / 32; C or bias not 8-byte aligned, ldc % 4 != 0 or < N; Cq not 4-byte aligned,
 * ldcq % 4 != 0 or < N, ldc_s < N / 32; residual, gate_table or gate_temb not 8-byte aligned; 256 rows of Aq or Wq spanning
 * 2^31 bytes or more, the output (M * ldc * 2, or M * ldcq and M * ldc_s bytes) 2^32 - 256 or more.
 * All of it is checked before anything is launched, without a device.  There is one kernel form (256 x 256 tiles). */
typedef struct ltxmi_gemm_mx8_args {
    const void* Aq;       int64_t lda;      /* [M,K] e4m3                                         */
    const void* A_scales; int64_t lda_s;    /* [M,K/32] E8M0                                      */
    const void* Wq;       int64_t ldw;      /* [N,K] e4m3                                         */
    const void* W_scales; int64_t ldw_s;    /* [N,K/32] E8M0                                      */
    const void* bias;                       /* [N] bf16 or NULL                                   */
    void*       C;        int64_t ldc;      /* [M,N] bf16, or NULL with Cq set                    */
    void*       Cq;       int64_t ldcq;     /* [M,N] e4m3, or NULL with C set                     */
    void*       C_scales; int64_t ldc_s;    /* [M,N/32] E8M0, with Cq                             */
    int32_t M, N, K;
    int32_t epilogue;                       /* ltxmi_epilogue                                     */
    const void* residual; int64_t ldr;      /* [M,N] bf16, GATE_RESIDUAL only; may alias C        */
    const void* gate_table;                 /* [N] bf16 or NULL (gate = 1)                        */
    const void* gate_temb;                  /* bf16, row g at gate_temb + g*gate_ld               */
    int64_t     gate_ld;
    int32_t     rows_per_group;
} ltxmi_gemm_mx8_args;

int ltxmi_gemm_mx8(const ltxmi_gemm_mx8_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LTXMI_MX_H */
