// mx8_host_asan.cpp -- drives the HOST side of the MX-FP8 entries of include/ltxmi_mx.h (ltxmi_quantize_mx8_bf16, ltxmi_gemm_mx8)
// under AddressSanitizer.
//
// A stand-alone program (its own main), built by `make -C ltx-video-gpupoor_amd/csrc asan` against libltxmi_asan.so (host code
// instrumented, device code not) and run by tests/test_mx8_native_asan.py with NO device visible, so nothing is ever launched:
// a call either is refused by the entry check (LTXMI_ERR_INVALID_ARG / _UNSUPPORTED) or runs the whole launcher -- parameter block,
// instance choice, grid arithmetic, the LDS reservation's per-device state -- up to the HIP call that reports the missing device
// (LTXMI_ERR_LAUNCH).  ASan aborts the process on any host-side out-of-bounds access on the way; the driver checks every status
// and that a failure left a message in ltxmi_last_error().
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ltxmi_mx.h"

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
    void* p = base;
    void* q = base + (1 << 19);
    void* s = base + (1 << 18);

    // ---- quantiser
    for (int K : {32, 64, 2048, 2080, 8192, 16384})
        expect(ltxmi_quantize_mx8_bf16(p, K + 8, q, K + 16, s, K / 32 + 3, 301, K, nullptr), LTXMI_ERR_LAUNCH, "quantize: accepted width");
    expect(ltxmi_quantize_mx8_bf16(p, 4096, q, 4096, s, 128, 2147483647, 4096, nullptr), LTXMI_ERR_LAUNCH, "quantize: 2^31 - 1 rows");
    expect(ltxmi_quantize_mx8_bf16(nullptr, 64, q, 64, s, 2, 4, 64, nullptr), LTXMI_ERR_INVALID_ARG, "quantize: NULL x");
    expect(ltxmi_quantize_mx8_bf16(p, 64, nullptr, 64, s, 2, 4, 64, nullptr), LTXMI_ERR_INVALID_ARG, "quantize: NULL q");
    expect(ltxmi_quantize_mx8_bf16(p, 64, q, 64, nullptr, 2, 4, 64, nullptr), LTXMI_ERR_INVALID_ARG, "quantize: NULL scales");
    expect(ltxmi_quantize_mx8_bf16(p, 64, q, 64, s, 2, 0, 64, nullptr), LTXMI_ERR_INVALID_ARG, "quantize: rows 0");
    expect(ltxmi_quantize_mx8_bf16(p, 64, q, 64, s, 2, 4, -32, nullptr), LTXMI_ERR_INVALID_ARG, "quantize: K -32");
    expect(ltxmi_quantize_mx8_bf16(p, 64, q, 64, s, 2, 4, 48, nullptr), LTXMI_ERR_UNSUPPORTED, "quantize: K 48");
    expect(ltxmi_quantize_mx8_bf16(p, 60, q, 64, s, 2, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "quantize: ldx below K");
    expect(ltxmi_quantize_mx8_bf16(p, 68, q, 64, s, 2, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "quantize: ldx % 8");
    expect(ltxmi_quantize_mx8_bf16(p, 64, q, 72, s, 2, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "quantize: ldq % 16");
    expect(ltxmi_quantize_mx8_bf16(p, 64, q, 64, s, 1, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "quantize: lds below K / 32");
    expect(ltxmi_quantize_mx8_bf16(base + 8, 64, q, 64, s, 2, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "quantize: x off 16 bytes");
    expect(ltxmi_quantize_mx8_bf16(p, 64, base + 8, 64, s, 2, 4, 64, nullptr), LTXMI_ERR_UNSUPPORTED, "quantize: q off 16 bytes");

    // ---- GEMM
    ltxmi_gemm_mx8_args a;
    auto reset = [&](int M, int N, int K, int epi, bool mx) {
        memset(&a, 0, sizeof a);
        a.Aq = base; a.lda = K; a.A_scales = base + (1 << 17); a.lda_s = K / 32;
        a.Wq = base + (1 << 18); a.ldw = K; a.W_scales = base + (3 << 17); a.ldw_s = K / 32;
        a.bias = base + (1 << 16);
        if (mx) { a.Cq = base + (1 << 19); a.ldcq = N; a.C_scales = base + (5 << 17); a.ldc_s = N / 32; }
        else { a.C = base + (1 << 19); a.ldc = N; }
        a.M = M; a.N = N; a.K = K; a.epilogue = epi;
        if (epi == LTXMI_EPI_GATE_RESIDUAL) { a.residual = a.C; a.ldr = N; }
    };
    expect(ltxmi_gemm_mx8(nullptr, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: NULL struct");
    memset(&a, 0, sizeof a);
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: zeroed struct");
    const int shapes[][3] = {{1, 32, 128}, {300, 288, 256}, {2048, 4096, 8192}, {14976, 8192, 2048}, {14976, 16384, 4096}, {257, 8224, 128}};
    for (const auto& sh : shapes) {
        for (int epi : {LTXMI_EPI_NONE, LTXMI_EPI_GELU_TANH, LTXMI_EPI_GATE_RESIDUAL}) {
            reset(sh[0], sh[1], sh[2], epi, false);
            expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_LAUNCH, "gemm: accepted shape, bf16 output");
            a.bias = nullptr;
            expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_LAUNCH, "gemm: accepted shape, no bias");
            if (epi == LTXMI_EPI_GATE_RESIDUAL) {
                a.gate_table = base + (1 << 15); a.gate_temb = base + (1 << 14); a.gate_ld = 6 * sh[1]; a.rows_per_group = 37;
                expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_LAUNCH, "gemm: accepted shape, gated");
            } else {
                reset(sh[0], sh[1], sh[2], epi, true);
                expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_LAUNCH, "gemm: accepted shape, MX output");
            }
        }
    }
    // refused
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.Aq = nullptr;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: NULL Aq");
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.W_scales = nullptr;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: NULL W_scales");
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.C = nullptr;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: no output");
    reset(300, 288, 256, LTXMI_EPI_NONE, true); a.C = base;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: both outputs");
    reset(300, 288, 256, LTXMI_EPI_NONE, true); a.C_scales = nullptr;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: Cq without C_scales");
    reset(0, 288, 256, LTXMI_EPI_NONE, false);
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: M 0");
    reset(300, 288, 256, LTXMI_EPI_SILU, false);
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: SILU");
    reset(300, 288, 256, 9, false);
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: epilogue 9");
    reset(300, 288, 256, LTXMI_EPI_GATE_RESIDUAL, true);
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: GATE_RESIDUAL with the MX output");
    reset(300, 288, 256, LTXMI_EPI_GATE_RESIDUAL, false); a.residual = nullptr;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: GATE_RESIDUAL without a residual");
    reset(300, 288, 256, LTXMI_EPI_GATE_RESIDUAL, false); a.gate_table = base;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_INVALID_ARG, "gemm: gate_table without gate_temb");
    reset(300, 288, 192, LTXMI_EPI_NONE, false);
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: K 192");
    reset(300, 264, 256, LTXMI_EPI_NONE, false);
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: N 264");
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.lda = 264;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: lda % 16");
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.Wq = base + 8;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: Wq off 16 bytes");
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.lda_s = 10;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: lda_s % 4");
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.W_scales = base + 2;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: W_scales off 4 bytes");
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.ldc = 280;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: ldc below N");
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.bias = base + 4;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: bias off 8 bytes");
    reset(300, 288, 256, LTXMI_EPI_NONE, true); a.ldc_s = 8;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: ldc_s below N / 32");
    reset(300, 288, 256, LTXMI_EPI_NONE, false); a.lda = (int64_t)1 << 24;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: 256 rows of Aq past 2^31 bytes");

    reset(4096, 288, 256, LTXMI_EPI_NONE, false); a.ldc = (int64_t)1 << 19;
    expect(ltxmi_gemm_mx8(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "gemm: C of 2^32 bytes");

    printf("mx8_host_asan: %d calls, %d unexpected\n", g_calls, g_bad);
    return g_bad ? 1 : 0;
}
