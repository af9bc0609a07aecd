// mxa_host_asan.cpp -- drives the HOST side of the entries of include/ltxmi_mx_attn.h (ltxmi_gemm_mx8_rowsumsq,
// ltxmi_norm_modulate_mx8) under AddressSanitizer.
//
// A stand-alone program (its own main), built by `make -C ltx-video-gpupoor_amd/csrc asan` against libltxmi_asan.so (host code
// instrumented, device code not) and run by tests/test_mxa_native_asan.py with NO device visible, so nothing is ever launched:
// a call either is refused by the entry check (LTXMI_ERR_INVALID_ARG / _UNSUPPORTED) or runs the whole launcher -- the shared
// checks of ltxmi_gemm_mx8_args, the parameter block, the chunk dispatch, the LDS reservation's per-device state -- up to the HIP
// call that reports the missing device (LTXMI_ERR_LAUNCH).  ASan aborts the process on any host-side out-of-bounds access on the
// way; the driver checks every status and that a failure left a message in ltxmi_last_error().
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ltxmi_mx_attn.h"

static int g_calls = 0, g_bad = 0;

static void expect(int rc, int want, const char* what) {
    ++g_calls;
    const char* msg = ltxmi_last_error();
    if (rc != want || !(msg && msg[0])) {
        ++g_bad;
        fprintf(stderr, "UNEXPECTED %s: rc %d (wanted %d), message '%s'\n", what, rc, want, msg ? msg : "(null)");
    }
}

int main() {
    // host memory only: the pointers are valid and aligned, and no host code dereferences them
    std::vector<uint16_t> buf(1u << 20, 0);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(buf.data()) + 63) & ~uintptr_t(63));
    float* rss = reinterpret_cast<float*>(base + (7 << 17));

    // ---- GEMM with row sums
    ltxmi_gemm_mx8_args a;
    auto reset = [&](int M, int N, int K) {
        memset(&a, 0, sizeof a);
        a.Aq = base; a.lda = K; a.A_scales = base + (1 << 17); a.lda_s = K / 32;
        a.Wq = base + (1 << 18); a.ldw = K; a.W_scales = base + (3 << 17); a.ldw_s = K / 32;
        a.bias = base + (1 << 16);
        a.C = base + (1 << 19); a.ldc = N;
        a.M = M; a.N = N; a.K = K; a.epilogue = LTXMI_EPI_NONE;
    };
    expect(ltxmi_gemm_mx8_rowsumsq(nullptr, rss, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: NULL struct");
    memset(&a, 0, sizeof a);
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: zeroed struct");
    const int shapes[][4] = {{1, 64, 128, 64}, {1, 288, 256, 64}, {300, 288, 256, 256}, {520, 544, 384, 320}, {14976, 6144, 2048, 2048},
                             {14976, 2048, 2048, 2048}, {14976, 12288, 4096, 4096}, {257, 8224, 128, 8192}};
    for (const auto& sh : shapes) {
        reset(sh[0], sh[1], sh[2]);
        expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, sh[3], sh[3] / 64, nullptr), LTXMI_ERR_LAUNCH, "rowsumsq: accepted shape");
        a.bias = nullptr;
        expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, (sh[1] + 63) / 64 + 3, nullptr), LTXMI_ERR_LAUNCH, "rowsumsq: accepted, no bias, one block");
    }
    // refused by the shared checks
    reset(300, 288, 256); a.Aq = nullptr;
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: NULL Aq");
    reset(300, 288, 256); a.C = nullptr;
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: no output");
    reset(300, 288, 192);
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, 1, nullptr), LTXMI_ERR_UNSUPPORTED, "rowsumsq: K 192");
    reset(300, 264, 256);
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, 1, nullptr), LTXMI_ERR_UNSUPPORTED, "rowsumsq: N 264");
    reset(300, 288, 256); a.ldc = 280;
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, 1, nullptr), LTXMI_ERR_UNSUPPORTED, "rowsumsq: ldc below N");
    // refused by its own
    reset(300, 288, 256);
    expect(ltxmi_gemm_mx8_rowsumsq(&a, nullptr, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: NULL rowsumsq");
    reset(300, 288, 256); a.epilogue = LTXMI_EPI_GELU_TANH;
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: GELU");
    reset(300, 288, 256); a.epilogue = LTXMI_EPI_GATE_RESIDUAL; a.residual = a.C; a.ldr = 288;
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: GATE_RESIDUAL");
    reset(300, 288, 256); a.C = nullptr; a.Cq = base + (1 << 19); a.ldcq = 288; a.C_scales = base + (5 << 17); a.ldc_s = 9;
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: Cq set");
    reset(300, 288, 256);
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 0, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: cols 0");
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, -64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: cols -64");
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 96, 2, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: cols % 64");
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 320, 5, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: cols past N");
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 256, 3, nullptr), LTXMI_ERR_INVALID_ARG, "rowsumsq: ld below cols / 64");
    expect(ltxmi_gemm_mx8_rowsumsq(&a, reinterpret_cast<float*>(base + 2), 64, 1, nullptr), LTXMI_ERR_UNSUPPORTED, "rowsumsq: off 4 bytes");
    expect(ltxmi_gemm_mx8_rowsumsq(&a, rss, 64, (int64_t)1 << 22, nullptr), LTXMI_ERR_UNSUPPORTED, "rowsumsq: sums of 2^32 bytes");

    // ---- fused norm + quantise
    void* x = base;
    void* q = base + (1 << 19);
    void* s = base + (1 << 18);
    void* t = base + (1 << 17);
    for (int D : {32, 64, 512, 544, 2048, 2080, 4096, 8192})
        for (int kind : {LTXMI_NORM_RMS, LTXMI_NORM_LAYER})
            expect(ltxmi_norm_modulate_mx8(x, D + 8, q, D + 16, s, D / 32 + 3, 301, D, 1e-6f, kind, t, t, t, t, 6 * D, 13, nullptr),
                   LTXMI_ERR_LAUNCH, "norm_mx8: accepted width");
    expect(ltxmi_norm_modulate_mx8(x, 2048, q, 2048, s, 64, 2147483647, 2048, 1e-6f, LTXMI_NORM_RMS, t, t, t, t, 0, 1, nullptr),
           LTXMI_ERR_LAUNCH, "norm_mx8: 2^31 - 1 rows");
#define NM(X, LDX, Q, LDQ, S, LDS, ROWS, D, KIND, T, TLD, RPG) \
    ltxmi_norm_modulate_mx8(X, LDX, Q, LDQ, S, LDS, ROWS, D, 1e-6f, KIND, T, t, t, t, TLD, RPG, nullptr)
    expect(NM(nullptr, 64, q, 64, s, 2, 4, 64, 0, t, 64, 1), LTXMI_ERR_INVALID_ARG, "norm_mx8: NULL x");
    expect(NM(x, 64, nullptr, 64, s, 2, 4, 64, 0, t, 64, 1), LTXMI_ERR_INVALID_ARG, "norm_mx8: NULL q");
    expect(NM(x, 64, q, 64, nullptr, 2, 4, 64, 0, t, 64, 1), LTXMI_ERR_INVALID_ARG, "norm_mx8: NULL scales");
    expect(NM(x, 64, q, 64, s, 2, 4, 64, 0, nullptr, 64, 1), LTXMI_ERR_INVALID_ARG, "norm_mx8: NULL table");
    expect(NM(x, 64, q, 64, s, 2, 0, 64, 0, t, 64, 1), LTXMI_ERR_INVALID_ARG, "norm_mx8: rows 0");
    expect(NM(x, 64, q, 64, s, 2, 4, -32, 0, t, 64, 1), LTXMI_ERR_INVALID_ARG, "norm_mx8: D -32");
    expect(NM(x, 64, q, 64, s, 2, 4, 64, 0, t, 64, 0), LTXMI_ERR_INVALID_ARG, "norm_mx8: rows_per_group 0");
    expect(NM(x, 64, q, 64, s, 2, 4, 64, 2, t, 64, 1), LTXMI_ERR_INVALID_ARG, "norm_mx8: kind 2");
    expect(NM(x, 64, q, 64, s, 2, 4, 64, -1, t, 64, 1), LTXMI_ERR_INVALID_ARG, "norm_mx8: kind -1");
    expect(NM(x, 64, q, 64, s, 2, 4, 48, 0, t, 64, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: D 48");
    expect(NM(x, 8224, q, 8224, s, 257, 4, 8224, 0, t, 8224, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: D 8224");
    expect(NM(x, 56, q, 64, s, 2, 4, 64, 0, t, 64, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: ldx below D");
    expect(NM(x, 68, q, 64, s, 2, 4, 64, 0, t, 64, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: ldx % 8");
    expect(NM(x, 64, q, 72, s, 2, 4, 64, 0, t, 64, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: ldq % 16");
    expect(NM(x, 64, q, 48, s, 2, 4, 64, 0, t, 64, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: ldq below D");
    expect(NM(x, 64, q, 64, s, 1, 4, 64, 0, t, 64, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: lds below D / 32");
    expect(NM(x, 64, q, 64, s, 2, 4, 64, 0, t, 68, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: temb_ld % 8");
    expect(NM(base + 8, 64, q, 64, s, 2, 4, 64, 0, t, 64, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: x off 16 bytes");
    expect(NM(x, 64, base + 8, 64, s, 2, 4, 64, 0, t, 64, 1), LTXMI_ERR_UNSUPPORTED, "norm_mx8: q off 16 bytes");
#undef NM

    printf("mxa_host_asan: %d calls, %d unexpected\n", g_calls, g_bad);
    return g_bad ? 1 : 0;
}
