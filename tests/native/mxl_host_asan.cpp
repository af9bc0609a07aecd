// mxl_host_asan.cpp -- drives the HOST side of the entry of include/ltxmi_mx_lora.h (ltxmi_gemm_mx8_pair2) under
// AddressSanitizer.
//
// A stand-alone program (its own main), built by `make -C ltx-video-gpupoor_amd/csrc asan` against libltxmi_asan.so (host code
// instrumented, device code not) and run by tests/test_mxl_native_asan.py with NO device visible, so nothing is ever launched:
// a call either is refused by the entry check (LTXMI_ERR_INVALID_ARG / _UNSUPPORTED) or runs the whole launcher -- the shared
// checks of ltxmi_gemm_mx8_args and of the row sums, the pair's own, the parameter block, the dispatch over the seven instances,
// the LDS reservation's per-device state -- up to the HIP call that reports the missing device (LTXMI_ERR_LAUNCH).  ASan aborts
// the process on any host-side out-of-bounds access on the way; the driver checks every status and that a failure left a
// message in ltxmi_last_error().
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ltxmi_mx_lora.h"

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

    ltxmi_gemm_mx8_args a;
    ltxmi_gemm_mx8_pair p;
    auto reset = [&](int M, int N, int K, int K2, int group_cols) {
        memset(&a, 0, sizeof a);
        a.Aq = base; a.lda = K; a.A_scales = base + (1 << 17); a.lda_s = K / 32;
        a.Wq = base + (1 << 18); a.ldw = K; a.W_scales = base + (3 << 17); a.ldw_s = K / 32;
        a.bias = base + (1 << 16);
        a.C = base + (1 << 19); a.ldc = N;
        a.M = M; a.N = N; a.K = K; a.epilogue = LTXMI_EPI_NONE;
        const int groups = group_cols ? N / group_cols : 1;
        memset(&p, 0, sizeof p);
        p.A2q = base + (1 << 15); p.lda2 = (int64_t)groups * K2; p.A2_scales = base + (3 << 15); p.lda2_s = (int64_t)groups * K2 / 32;
        p.W2q = base + (5 << 15); p.ldw2 = K2; p.W2_scales = base + (7 << 15); p.ldw2_s = K2 / 32;
        p.K2 = K2; p.group_cols = group_cols;
    };
    auto mx_out = [&](int N) {
        a.C = nullptr; a.Cq = base + (1 << 19); a.ldcq = N; a.C_scales = base + (5 << 17); a.ldc_s = N / 32;
    };
    expect(ltxmi_gemm_mx8_pair2(nullptr, nullptr, nullptr, 0, 0, nullptr), LTXMI_ERR_INVALID_ARG, "NULL structs");
    memset(&a, 0, sizeof a);
    memset(&p, 0, sizeof p);
    expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_INVALID_ARG, "zeroed structs");

    // ---- accepted: every instance at every shape, up to the launch
    const int shapes[][5] = {{1, 288, 128, 128, 0},      {300, 288, 256, 128, 0},      {520, 544, 384, 256, 0},
                             {300, 768, 256, 128, 256},  {300, 1024, 256, 128, 512},   {14976, 6144, 2048, 128, 2048},
                             {14976, 2048, 8192, 256, 0}, {14976, 12288, 4096, 128, 4096}};
    for (const auto& sh : shapes) {
        const int N = sh[1];
        reset(sh[0], N, sh[2], sh[3], sh[4]);
        expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_LAUNCH, "accepted: NONE");
        expect(ltxmi_gemm_mx8_pair2(&a, &p, rss, 64, (N + 63) / 64 + 3, nullptr), LTXMI_ERR_LAUNCH, "accepted: row sums, one block");
        expect(ltxmi_gemm_mx8_pair2(&a, &p, rss, N / 64 * 64, N / 64, nullptr), LTXMI_ERR_LAUNCH, "accepted: row sums, every block");
        a.epilogue = LTXMI_EPI_GELU_TANH; a.bias = nullptr;
        expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_LAUNCH, "accepted: GELU, no bias");
        a.epilogue = LTXMI_EPI_GATE_RESIDUAL; a.residual = a.C; a.ldr = N;
        expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_LAUNCH, "accepted: residual without a gate");
        a.gate_table = base + (1 << 16); a.gate_temb = base + (1 << 16); a.gate_ld = 0; a.rows_per_group = 7;
        expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_LAUNCH, "accepted: gate + residual");
        reset(sh[0], N, sh[2], sh[3], sh[4]); mx_out(N);
        expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_LAUNCH, "accepted: MX output");
        a.epilogue = LTXMI_EPI_GELU_TANH;
        expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_LAUNCH, "accepted: MX output, GELU");
    }

    // ---- refused by the shared checks
    reset(300, 288, 256, 128, 0); a.Aq = nullptr;
    expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_INVALID_ARG, "NULL Aq");
    reset(300, 288, 192, 128, 0);
    expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_UNSUPPORTED, "K 192");
    reset(300, 288, 256, 128, 0); mx_out(288); a.epilogue = LTXMI_EPI_GATE_RESIDUAL; a.residual = base; a.ldr = 288;
    expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), LTXMI_ERR_INVALID_ARG, "GATE_RESIDUAL with Cq");
    reset(300, 288, 256, 128, 0); a.epilogue = LTXMI_EPI_GELU_TANH;
    expect(ltxmi_gemm_mx8_pair2(&a, &p, rss, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "row sums with GELU");
    reset(300, 288, 256, 128, 0); mx_out(288);
    expect(ltxmi_gemm_mx8_pair2(&a, &p, rss, 64, 1, nullptr), LTXMI_ERR_INVALID_ARG, "row sums with Cq");
    reset(300, 288, 256, 128, 0);
    expect(ltxmi_gemm_mx8_pair2(&a, &p, rss, 96, 2, nullptr), LTXMI_ERR_INVALID_ARG, "cols % 64");
    expect(ltxmi_gemm_mx8_pair2(&a, &p, rss, 320, 5, nullptr), LTXMI_ERR_INVALID_ARG, "cols past N");
    expect(ltxmi_gemm_mx8_pair2(&a, &p, rss, 256, 3, nullptr), LTXMI_ERR_INVALID_ARG, "ld below cols / 64");
    expect(ltxmi_gemm_mx8_pair2(&a, &p, reinterpret_cast<float*>(base + 2), 64, 1, nullptr), LTXMI_ERR_UNSUPPORTED, "rowsumsq off 4 bytes");
    expect(ltxmi_gemm_mx8_pair2(&a, &p, rss, 64, (int64_t)1 << 22, nullptr), LTXMI_ERR_UNSUPPORTED, "sums of 2^32 bytes");

    // ---- refused by the pair's own
    expect(ltxmi_gemm_mx8_pair2(&a, nullptr, nullptr, 0, 0, nullptr), LTXMI_ERR_INVALID_ARG, "NULL pair");
#define REFUSE(SET, WANT, WHAT)                                                          \
    reset(300, 768, 256, 128, 256);                                                      \
    SET;                                                                                 \
    expect(ltxmi_gemm_mx8_pair2(&a, &p, nullptr, 0, 0, nullptr), WANT, WHAT)
    REFUSE(p.A2q = nullptr, LTXMI_ERR_INVALID_ARG, "NULL A2q");
    REFUSE(p.A2_scales = nullptr, LTXMI_ERR_INVALID_ARG, "NULL A2_scales");
    REFUSE(p.W2q = nullptr, LTXMI_ERR_INVALID_ARG, "NULL W2q");
    REFUSE(p.W2_scales = nullptr, LTXMI_ERR_INVALID_ARG, "NULL W2_scales");
    REFUSE(p.K2 = 0, LTXMI_ERR_INVALID_ARG, "K2 0");
    REFUSE(p.K2 = -128, LTXMI_ERR_INVALID_ARG, "K2 -128");
    REFUSE(p.K2 = 64, LTXMI_ERR_INVALID_ARG, "K2 64");
    REFUSE(p.group_cols = -256, LTXMI_ERR_INVALID_ARG, "group_cols -256");
    REFUSE(p.group_cols = 128, LTXMI_ERR_INVALID_ARG, "group_cols 128");
    REFUSE(p.group_cols = 512, LTXMI_ERR_INVALID_ARG, "group_cols 512 does not divide 768");
    REFUSE(p.lda2 = 392, LTXMI_ERR_UNSUPPORTED, "lda2 % 16");
    REFUSE(p.ldw2 = 136, LTXMI_ERR_UNSUPPORTED, "ldw2 % 16");
    REFUSE(p.lda2 = 256, LTXMI_ERR_UNSUPPORTED, "lda2 below groups * K2");
    REFUSE(p.ldw2 = 112, LTXMI_ERR_UNSUPPORTED, "ldw2 below K2");
    REFUSE(p.lda2_s = 14, LTXMI_ERR_UNSUPPORTED, "lda2_s % 4");
    REFUSE(p.ldw2_s = 6, LTXMI_ERR_UNSUPPORTED, "ldw2_s % 4");
    REFUSE(p.lda2_s = 8, LTXMI_ERR_UNSUPPORTED, "lda2_s below groups * K2 / 32");
    REFUSE(p.ldw2_s = 0, LTXMI_ERR_UNSUPPORTED, "ldw2_s below K2 / 32");
    REFUSE(p.A2q = base + 8, LTXMI_ERR_UNSUPPORTED, "A2q off 16 bytes");
    REFUSE(p.W2q = base + 8, LTXMI_ERR_UNSUPPORTED, "W2q off 16 bytes");
    REFUSE(p.A2_scales = base + 2, LTXMI_ERR_UNSUPPORTED, "A2_scales off 4 bytes");
    REFUSE(p.W2_scales = base + 2, LTXMI_ERR_UNSUPPORTED, "W2_scales off 4 bytes");
    REFUSE(p.lda2 = (int64_t)1 << 23, LTXMI_ERR_UNSUPPORTED, "256 rows of A2q span 2^31 bytes");
    REFUSE(p.ldw2 = (int64_t)1 << 23, LTXMI_ERR_UNSUPPORTED, "256 rows of W2q span 2^31 bytes");
    REFUSE(p.lda2_s = (int64_t)1 << 23, LTXMI_ERR_UNSUPPORTED, "256 rows of A2_scales span 2^31 bytes");
    REFUSE(p.ldw2_s = (int64_t)1 << 23, LTXMI_ERR_UNSUPPORTED, "256 rows of W2_scales span 2^31 bytes");
    REFUSE(a.lda_s = (int64_t)1 << 23, LTXMI_ERR_UNSUPPORTED, "256 rows of A_scales span 2^31 bytes");
    REFUSE(a.ldw_s = (int64_t)1 << 23, LTXMI_ERR_UNSUPPORTED, "256 rows of W_scales span 2^31 bytes");
#undef REFUSE

    printf("mxl_host_asan: %d calls, %d unexpected\n", g_calls, g_bad);
    return g_bad ? 1 : 0;
}
