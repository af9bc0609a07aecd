// mxt_host_asan.cpp -- drives the HOST side of the entries of include/ltxmi_mx_t5.h (ltxmi_gemm_mx8_skinny and its plan,
// ltxmi_rmsnorm_weight_mx8, ltxmi_gated_gelu_mx8) under AddressSanitizer.
//
// A stand-alone program (its own main), built by `make -C ltx-video-gpupoor_amd/csrc asan` against libltxmi_asan.so (host code
// instrumented, device code not) and run by tests/test_mxt_native_asan.py with NO device visible, so nothing is ever launched:
// a call either is refused by the entry check (LTXMI_ERR_INVALID_ARG / _UNSUPPORTED) or runs the whole launcher -- the shared
// checks of ltxmi_gemm_mx8_args, the plan, the parameter block, the chunk dispatch, the LDS reservation's per-device state -- up
// to the HIP call that reports the missing device (LTXMI_ERR_LAUNCH).  ASan aborts the process on any host-side out-of-bounds
// access on the way; the driver checks every status and that a failure left a message in ltxmi_last_error().
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ltxmi_mx_t5.h"

static int g_calls = 0, g_bad = 0;

static void expect(int rc, int want, const char* what) {
    ++g_calls;
    const char* msg = ltxmi_last_error();
    if (rc != want || (want < 0 && !(msg && msg[0]))) {
        ++g_bad;
        fprintf(stderr, "UNEXPECTED %s: rc %d (wanted %d), message '%s'\n", what, rc, want, msg ? msg : "(null)");
    }
}

int main() {
    // host memory only: the pointers are valid and aligned, and no host code dereferences them
    std::vector<uint16_t> buf(1u << 20, 0);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(buf.data()) + 63) & ~uintptr_t(63));

    // ---- the skinny GEMM and its plan
    ltxmi_gemm_mx8_args a;
    auto reset = [&](int M, int N, int K) {
        memset(&a, 0, sizeof a);
        a.Aq = base; a.lda = K; a.A_scales = base + (1 << 17); a.lda_s = K / 32;
        a.Wq = base + (1 << 18); a.ldw = K; a.W_scales = base + (3 << 17); a.ldw_s = K / 32;
        a.C = base + (1 << 19); a.ldc = N;
        a.M = M; a.N = N; a.K = K; a.epilogue = LTXMI_EPI_NONE;
    };
    expect(ltxmi_gemm_mx8_skinny(nullptr, 0, nullptr), LTXMI_ERR_INVALID_ARG, "skinny: NULL struct");
    expect(ltxmi_gemm_mx8_skinny_form(nullptr, 0), LTXMI_ERR_INVALID_ARG, "plan: NULL struct");
    memset(&a, 0, sizeof a);
    expect(ltxmi_gemm_mx8_skinny(&a, 0, nullptr), LTXMI_ERR_INVALID_ARG, "skinny: zeroed struct");
    const int shapes[][3] = {{1, 32, 128}, {33, 288, 384}, {200, 288, 896}, {512, 4096, 4096}, {256, 12288, 4096}, {512, 20480, 4096},
                             {512, 4096, 10240}, {64, 4096, 10240}};
    for (const auto& sh : shapes)
        for (int form = 0; form <= 2; ++form) {
            reset(sh[0], sh[1], sh[2]);
            const int plan = ltxmi_gemm_mx8_skinny_form(&a, form);
            // a forced form is the form that runs; the choice by shape is one of the two
            expect(plan, form ? form : (plan == LTXMI_MXT_FORM_128X64 ? plan : LTXMI_MXT_FORM_64X64), "plan: accepted shape");
            expect(ltxmi_gemm_mx8_skinny(&a, form, nullptr), LTXMI_ERR_LAUNCH, "skinny: accepted shape");
            a.bias = base + (1 << 16);
            expect(ltxmi_gemm_mx8_skinny(&a, form, nullptr), LTXMI_ERR_LAUNCH, "skinny: accepted, with a bias");
            a.bias = nullptr; a.epilogue = LTXMI_EPI_GATE_RESIDUAL; a.residual = a.C; a.ldr = a.ldc;
            expect(ltxmi_gemm_mx8_skinny(&a, form, nullptr), LTXMI_ERR_LAUNCH, "skinny: accepted, residual in place");
        }
    // refused by the shared checks
    reset(300, 288, 256); a.Aq = nullptr;
    expect(ltxmi_gemm_mx8_skinny(&a, 0, nullptr), LTXMI_ERR_INVALID_ARG, "skinny: NULL Aq");
    reset(300, 288, 192);
    expect(ltxmi_gemm_mx8_skinny(&a, 0, nullptr), LTXMI_ERR_UNSUPPORTED, "skinny: K 192");
    reset(300, 264, 256);
    expect(ltxmi_gemm_mx8_skinny_form(&a, 0), LTXMI_ERR_UNSUPPORTED, "plan: N 264");
    reset(300, 288, 256); a.ldc = 280;
    expect(ltxmi_gemm_mx8_skinny(&a, 0, nullptr), LTXMI_ERR_UNSUPPORTED, "skinny: ldc below N");
    // refused by its own
    reset(513, 288, 256);
    expect(ltxmi_gemm_mx8_skinny(&a, 0, nullptr), LTXMI_ERR_UNSUPPORTED, "skinny: 513 rows");
    expect(ltxmi_gemm_mx8_skinny_form(&a, 1), LTXMI_ERR_UNSUPPORTED, "plan: 513 rows");
    reset(300, 288, 256);
    expect(ltxmi_gemm_mx8_skinny(&a, 3, nullptr), LTXMI_ERR_UNSUPPORTED, "skinny: form 3");
    expect(ltxmi_gemm_mx8_skinny_form(&a, -1), LTXMI_ERR_UNSUPPORTED, "plan: form -1");
    reset(300, 288, 256); a.epilogue = LTXMI_EPI_GELU_TANH;
    expect(ltxmi_gemm_mx8_skinny(&a, 0, nullptr), LTXMI_ERR_UNSUPPORTED, "skinny: GELU");
    reset(300, 288, 256); a.C = nullptr; a.Cq = base + (1 << 19); a.ldcq = 288; a.C_scales = base + (5 << 17); a.ldc_s = 9;
    expect(ltxmi_gemm_mx8_skinny(&a, 0, nullptr), LTXMI_ERR_UNSUPPORTED, "skinny: Cq set");
    reset(300, 288, 256); a.epilogue = LTXMI_EPI_GATE_RESIDUAL; a.residual = a.C; a.ldr = 288; a.bias = base + (1 << 16);
    expect(ltxmi_gemm_mx8_skinny(&a, 0, nullptr), LTXMI_ERR_UNSUPPORTED, "skinny: bias with a residual");
    a.bias = nullptr; a.gate_table = base + (1 << 16); a.gate_temb = base + (1 << 16); a.rows_per_group = 1;
    expect(ltxmi_gemm_mx8_skinny(&a, 0, nullptr), LTXMI_ERR_UNSUPPORTED, "skinny: gate table");

    // ---- the fused row passes
    void* x = base;
    void* q = base + (1 << 19);
    void* s = base + (1 << 18);
    void* w = base + (1 << 17);
    for (int D : {32, 64, 512, 544, 2048, 2080, 4096, 4128, 8192})
        expect(ltxmi_rmsnorm_weight_mx8(x, D + 8, q, D + 16, s, D / 32 + 3, 301, D, w, 1e-6f, nullptr), LTXMI_ERR_LAUNCH,
               "rmsnorm_mx8: accepted width");
    expect(ltxmi_rmsnorm_weight_mx8(x, 64, q, 64, s, 2, 4 * ((1 << 24) - 1), 64, w, 1e-6f, nullptr), LTXMI_ERR_LAUNCH, "rmsnorm_mx8: most rows");
    expect(ltxmi_rmsnorm_weight_mx8(x, 64, q, 64, s, 2, 4 * ((1 << 24) - 1) + 1, 64, w, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED,
           "rmsnorm_mx8: too many rows");
    expect(ltxmi_rmsnorm_weight_mx8(nullptr, 64, q, 64, s, 2, 4, 64, w, 1e-6f, nullptr), LTXMI_ERR_INVALID_ARG, "rmsnorm_mx8: NULL x");
    expect(ltxmi_rmsnorm_weight_mx8(x, 64, q, 64, s, 2, 4, 64, nullptr, 1e-6f, nullptr), LTXMI_ERR_INVALID_ARG, "rmsnorm_mx8: NULL weight");
    expect(ltxmi_rmsnorm_weight_mx8(x, 64, q, 64, s, 2, 0, 64, w, 1e-6f, nullptr), LTXMI_ERR_INVALID_ARG, "rmsnorm_mx8: rows 0");
    expect(ltxmi_rmsnorm_weight_mx8(x, 1000, q, 1008, s, 32, 4, 1000, w, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "rmsnorm_mx8: D 1000");
    expect(ltxmi_rmsnorm_weight_mx8(x, 8224, q, 8224, s, 257, 4, 8224, w, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "rmsnorm_mx8: D 8224");
    expect(ltxmi_rmsnorm_weight_mx8(x, 64, q, 72, s, 2, 4, 64, w, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "rmsnorm_mx8: ldq % 16");
    expect(ltxmi_rmsnorm_weight_mx8(x, 64, q, 64, s, 1, 4, 64, w, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "rmsnorm_mx8: lds below D / 32");
    expect(ltxmi_rmsnorm_weight_mx8(base + 8, 64, q, 64, s, 2, 4, 64, w, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "rmsnorm_mx8: x off 16 bytes");

    for (int F : {32, 64, 2080, 10240})
        for (int rows : {1, 301, 1 << 20})
            expect(ltxmi_gated_gelu_mx8(x, 2 * F + 8, q, F + 16, s, F / 32 + 3, rows, F, nullptr), LTXMI_ERR_LAUNCH, "gelu_mx8: accepted");
    expect(ltxmi_gated_gelu_mx8(x, 128, q, 64, s, 2, 2147483647, 64, nullptr), LTXMI_ERR_LAUNCH, "gelu_mx8: 2^31 - 1 rows");
    expect(ltxmi_gated_gelu_mx8(nullptr, 128, q, 64, s, 2, 4, 64, nullptr), LTXMI_ERR_INVALID_ARG, "gelu_mx8: NULL h");
    expect(ltxmi_gated_gelu_mx8(x, 128, q, 64, nullptr, 2, 4, 64, nullptr), LTXMI_ERR_INVALID_ARG, "gelu_mx8: NULL scales");
    expect(ltxmi_gated_gelu_mx8(x, 128, q, 64, s, 2, 4, 0, nullptr), LTXMI_ERR_INVALID_ARG, "gelu_mx8: F 0");
    expect(ltxmi_gated_gelu_mx8(x, 2000, q, 1008, s, 32, 4, 1000, nullptr), LTXMI_ERR_UNSUPPORTED, "gelu_mx8: F 1000");
    expect(ltxmi_gated_gelu_mx8(x, 120, q, 64, s, 2, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "gelu_mx8: ldh below 2 F");
    expect(ltxmi_gated_gelu_mx8(x, 128, q, 48, s, 2, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "gelu_mx8: ldq below F");
    expect(ltxmi_gated_gelu_mx8(x, 128, q, 64, s, 1, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "gelu_mx8: lds below F / 32");
    expect(ltxmi_gated_gelu_mx8(x, 128, base + 8, 64, s, 2, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "gelu_mx8: q off 16 bytes");

    printf("mxt_host_asan: %d calls, %d unexpected\n", g_calls, g_bad);
    return g_bad ? 1 : 0;
}
