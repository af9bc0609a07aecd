// The compiler's own reading of include/ltxmi.h, as JSON on stdout: sizeof of every struct, offsetof and size of every field, the
// value of every enum constant and integer #define, and LTXMI_VERSION.  Includes nothing but the header and links no library
// (`make -C ltx-video-gpupoor_amd/csrc abi_layout`).  tests/test_abi_binding.py compares the ctypes binding, which is parsed
// from the same header, with this output; a struct, field or constant the header gains is added here (the test compares the
// two lists both ways, so a forgotten one fails).
#include <cstddef>
#include <cstdio>

#include "ltxmi.h"

#define STR2(x) #x
#define STR(x) STR2(x)
static const char* sep = "";
static const char* fsep = "";
#define OPEN  printf("%s\n    \"%s\": {\"size\": %zu, \"fields\": {", sep, STR(STRUCT), sizeof(STRUCT)); sep = ","; fsep = "";
#define FIELD(f)  printf("%s\"%s\": [%zu, %zu]", fsep, #f, offsetof(STRUCT, f), sizeof(((STRUCT*)0)->f)); fsep = ", ";
#define CLOSE printf("}}");
#define CONST(c)  printf("%s\n    \"%s\": %lld", sep, #c, (long long)(c)); sep = ",";

int main() {
    printf("{\n  \"version\": \"%s\",\n  \"structs\": {", LTXMI_VERSION);
#define STRUCT ltxmi_gemm_args
    OPEN FIELD(A) FIELD(lda) FIELD(W) FIELD(ldw) FIELD(bias) FIELD(C) FIELD(ldc) FIELD(M) FIELD(N) FIELD(K) FIELD(epilogue) FIELD(residual) FIELD(ldr) FIELD(gate_table) FIELD(gate_temb)
    FIELD(gate_ld) FIELD(rows_per_group) FIELD(algo) FIELD(rowsumsq) FIELD(rowsumsq_cols) FIELD(rowsumsq_ld) FIELD(a_kblock) FIELD(a_kblock_stride) CLOSE
#undef STRUCT
#define STRUCT ltxmi_gemm_pair
    OPEN FIELD(A2) FIELD(lda2) FIELD(W2) FIELD(ldw2) FIELD(K2) FIELD(group_cols) CLOSE
#undef STRUCT
#define STRUCT ltxmi_attn_args
    OPEN FIELD(q) FIELD(q_stride_b) FIELD(q_stride_l) FIELD(k) FIELD(k_stride_b) FIELD(k_stride_l) FIELD(v) FIELD(v_stride_b) FIELD(v_stride_l)
    FIELD(o) FIELD(o_stride_b) FIELD(o_stride_l) FIELD(key_bias) FIELD(bias_stride_b) FIELD(B) FIELD(H) FIELD(Lq) FIELD(Lk) FIELD(head_dim) FIELD(softmax_scale)
    FIELD(q_rowsumsq) FIELD(q_rowsumsq_stride_b) FIELD(q_rowsumsq_stride_l) FIELD(q_rowsumsq_blocks) FIELD(q_norm_weight) FIELD(q_norm_eps)
    FIELD(rope_cos) FIELD(rope_sin) FIELD(rope_stride_b) FIELD(rope_stride_l) FIELD(o_segment_len) FIELD(o_stride_segment)
    FIELD(q_rstd) FIELD(q_rstd_stride_b) FIELD(q_rstd_stride_l) FIELD(redo_counter) FIELD(force_exact) FIELD(lse) FIELD(lse_stride_b) FIELD(lse_stride_h) CLOSE
#undef STRUCT
#define STRUCT ltxmi_attn_merge_args
    OPEN FIELD(n) FIELD(o_part) FIELD(o_part_stride_b) FIELD(o_part_stride_l) FIELD(lse_part) FIELD(lse_part_stride_b) FIELD(lse_part_stride_h)
    FIELD(o) FIELD(o_stride_b) FIELD(o_stride_l) FIELD(lse) FIELD(lse_stride_b) FIELD(lse_stride_h) FIELD(B) FIELD(H) FIELD(Lq) FIELD(head_dim) CLOSE
#undef STRUCT
#define STRUCT ltxmi_conv3d_args
    OPEN FIELD(x) FIELD(w) FIELD(bias) FIELD(y) FIELD(B) FIELD(T) FIELD(H) FIELD(W) FIELD(Cin) FIELD(Cout) FIELD(causal) FIELD(pad_replicate) FIELD(d2s) FIELD(residual)
    FIELD(res_channels) FIELD(add) FIELD(stride_t) FIELD(stride_hw) FIELD(tpad) FIELD(out_T) FIELD(kernel_t) FIELD(time_pad_zeros) FIELD(algo)
    FIELD(post_norm) FIELD(post_scale) FIELD(post_shift) FIELD(post_eps) FIELD(y_norm) FIELD(workspace) FIELD(workspace_bytes) CLOSE
#undef STRUCT
#define STRUCT ltxmi_conv3d_route_info
    OPEN FIELD(route) FIELD(epilogue) FIELD(ksplit) FIELD(swap_hw) FIELD(finalize_blocks) CLOSE
#undef STRUCT
#define STRUCT ltxmi_attn_relbias_args
    OPEN FIELD(q) FIELD(q_stride_b) FIELD(q_stride_l) FIELD(k) FIELD(k_stride_b) FIELD(k_stride_l) FIELD(v) FIELD(v_stride_b) FIELD(v_stride_l)
    FIELD(o) FIELD(o_stride_b) FIELD(o_stride_l) FIELD(key_bias) FIELD(bias_stride_b) FIELD(B) FIELD(H) FIELD(Lq) FIELD(Lk) FIELD(head_dim) FIELD(softmax_scale)
    FIELD(rel_bias) FIELD(rel_stride_h) FIELD(rel_center) CLOSE
#undef STRUCT
    printf("\n  },\n  \"constants\": {");
    sep = "";
    CONST(LTXMI_OK) CONST(LTXMI_ERR_INVALID_ARG) CONST(LTXMI_ERR_UNSUPPORTED) CONST(LTXMI_ERR_LAUNCH)
    CONST(LTXMI_EPI_NONE) CONST(LTXMI_EPI_GELU_TANH) CONST(LTXMI_EPI_SILU) CONST(LTXMI_EPI_GATE_RESIDUAL)
    CONST(LTXMI_GEMM_TILE128) CONST(LTXMI_GEMM_TILE256) CONST(LTXMI_GEMM_PERSISTENT256) CONST(LTXMI_GEMM_PAIR2_TILE128) CONST(LTXMI_GEMM_PAIR2_TILE256)
    CONST(LTXMI_NORM_RMS) CONST(LTXMI_NORM_LAYER)
    CONST(LTXMI_ATTN_MERGE_MAX)
    CONST(LTXMI_PAD_ZEROS) CONST(LTXMI_PAD_REPLICATE) CONST(LTXMI_PAD_REFLECT)
    CONST(LTXMI_CONV_GEMM128) CONST(LTXMI_CONV_GEMM256) CONST(LTXMI_CONV_DIRECT8) CONST(LTXMI_CONV_DIRECT4)
    CONST(LTXMI_GUIDANCE_WORKSPACE_FLOATS)
    CONST(LTXMI_BLEND_F32) CONST(LTXMI_BLEND_BF16) CONST(LTXMI_BLEND_F16)
    printf("\n  }\n}\n");
    return 0;
}
