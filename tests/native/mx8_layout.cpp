// The compiler's own reading of include/ltxmi_mx.h, as JSON on stdout, in the form of tests/native/abi_layout.cpp: sizeof of the
// struct, offsetof and size of every field, the header's integer #define and LTXMI_MX_VERSION.  Includes nothing but the header
// and links no library (`make -C ltx-video-gpupoor_amd/csrc mx8_layout`).  tests/test_mx8_abi.py compares the ctypes binding,
// which ltxmi/_lib_mx.py parses from the same header, with this output, both ways.
#include <cstddef>
#include <cstdio>

#include "ltxmi_mx.h"

#define STRUCT ltxmi_gemm_mx8_args
static const char* fsep = "";
#define FIELD(f)  printf("%s\"%s\": [%zu, %zu]", fsep, #f, offsetof(STRUCT, f), sizeof(((STRUCT*)0)->f)); fsep = ", ";

int main() {
    printf("{\n  \"version\": \"%s\",\n  \"structs\": {\n    \"ltxmi_gemm_mx8_args\": {\"size\": %zu, \"fields\": {", LTXMI_MX_VERSION, sizeof(STRUCT));
    FIELD(Aq) FIELD(lda) FIELD(A_scales) FIELD(lda_s) FIELD(Wq) FIELD(ldw) FIELD(W_scales) FIELD(ldw_s) FIELD(bias) FIELD(C) FIELD(ldc)
    FIELD(Cq) FIELD(ldcq) FIELD(C_scales) FIELD(ldc_s) FIELD(M) FIELD(N) FIELD(K) FIELD(epilogue) FIELD(residual) FIELD(ldr)
    FIELD(gate_table) FIELD(gate_temb) FIELD(gate_ld) FIELD(rows_per_group)
    printf("}}\n  },\n  \"constants\": {\"LTXMI_MX_BLOCK\": %d}\n}\n", LTXMI_MX_BLOCK);
    return 0;
}
