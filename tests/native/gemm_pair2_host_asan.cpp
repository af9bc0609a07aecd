// gemm_pair2_host_asan.cpp -- drives the HOST side of ltxmi_gemm_pair2_bf16 / ltxmi_gemm_pair2_kernel_id under AddressSanitizer.
//
// A stand-alone program (its own main), built by `make -C ltx-video-gpupoor_amd/csrc asan` against libltxmi_asan.so (host code
// instrumented, device code not) and run by tests/test_lora_native_asan.py with NO device visible, so nothing is ever
// launched: a call either is refused by the entry check (LTXMI_ERR_INVALID_ARG / _UNSUPPORTED) or runs the whole launcher --
// kernel choice, parameter block, grid arithmetic, per-device state -- up to the HIP call that reports the missing device
// (LTXMI_ERR_LAUNCH).  ASan aborts the process on any host-side out-of-bounds access on the way; the driver checks every
// status, that a failure left a message in ltxmi_last_error(), and that the id query agrees with the launch.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ltxmi.h"

static int g_calls = 0, g_bad = 0;

// the id query answers `want_id`; the launch then is refused with the same status, or (accepted) fails at the missing device
static void expect(const ltxmi_gemm_args* a, const ltxmi_gemm_pair* p, int want_id, const char* what) {
    ++g_calls;
    const int id = ltxmi_gemm_pair2_kernel_id(a, p);
    const char* msg_id = ltxmi_last_error();
    const bool id_ok = id == want_id && (id >= 0 || (msg_id && msg_id[0]));
    const int rc = ltxmi_gemm_pair2_bf16(a, p, nullptr);
    const char* msg = ltxmi_last_error();
    const int want_rc = want_id < 0 ? want_id : LTXMI_ERR_LAUNCH;
    if (!id_ok || rc != want_rc || !(msg && msg[0])) {
        ++g_bad;
        fprintf(stderr, "UNEXPECTED %s: id %d (wanted %d), launch rc %d (wanted %d), message '%s'\n", what, id, want_id, rc, want_rc,
                msg ? msg : "(null)");
    }
}

int main() {
    // host memory only: the pointers are valid, and no host code dereferences them
    std::vector<uint16_t> buf(1u << 20, 0);
    char* base = reinterpret_cast<char*>(buf.data());
    void* p = base;

    ltxmi_gemm_args g;
    ltxmi_gemm_pair q;
    auto reset = [&]() {
        memset(&g, 0, sizeof g);
        memset(&q, 0, sizeof q);
        g.A = p; g.W = p; g.C = p; g.lda = 2048; g.ldw = 2048; g.ldc = 6144; g.M = 14976; g.N = 6144; g.K = 2048;
        q.A2 = p; q.W2 = p; q.lda2 = 384; q.ldw2 = 128; q.K2 = 128; q.group_cols = 2048;
    };

    expect(nullptr, nullptr, LTXMI_ERR_INVALID_ARG, "NULL, NULL");
    reset();
    expect(&g, nullptr, LTXMI_ERR_INVALID_ARG, "NULL pair");
    expect(nullptr, &q, LTXMI_ERR_INVALID_ARG, "NULL args");
    memset(&q, 0, sizeof q);
    expect(&g, &q, LTXMI_ERR_INVALID_ARG, "zeroed pair");
    memset(&g, 0, sizeof g);
    expect(&g, &q, LTXMI_ERR_INVALID_ARG, "zeroed both");

    // accepted: the packed QKV projection of a step with a rank-128 adapter, every epilogue's launcher, both forms
    reset();
    expect(&g, &q, 4, "qkv by shape");
    g.algo = 128; expect(&g, &q, 3, "qkv algo 128");
    g.algo = 256; expect(&g, &q, 4, "qkv algo 256");
    g.algo = 7; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "algo 7");
    for (int algo : {128, 256}) {
        reset();
        g.algo = algo;
        const int id = algo == 128 ? 3 : 4;
        g.bias = p; expect(&g, &q, id, "bias");
        g.epilogue = LTXMI_EPI_GELU_TANH; expect(&g, &q, id, "gelu");
        g.epilogue = LTXMI_EPI_SILU; expect(&g, &q, id, "silu");
        g.epilogue = LTXMI_EPI_GATE_RESIDUAL;
        expect(&g, &q, LTXMI_ERR_INVALID_ARG, "gate without residual");
        g.residual = p; g.ldr = 6144; expect(&g, &q, id, "residual without gate");
        g.gate_table = p; g.gate_temb = p; g.gate_ld = 6 * 6144; g.rows_per_group = 4992; expect(&g, &q, id, "gate + residual");
        g.rows_per_group = 0; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "gate with rows_per_group 0");
        g.epilogue = 99; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "epilogue 99");
        g.epilogue = 0;
        g.rowsumsq = reinterpret_cast<float*>(base); g.rowsumsq_cols = 2048; g.rowsumsq_ld = 32; expect(&g, &q, id, "row sums");
        g.rowsumsq_cols = 2000; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "rowsumsq_cols % 64");
        // NULL rowsumsq with garbage in its companions: off, whatever they hold
        g.rowsumsq = nullptr; g.rowsumsq_cols = 0x7fffff00; g.rowsumsq_ld = -12345; expect(&g, &q, id, "NULL rowsumsq, garbage cols / ld");
    }
    // by shape: the thresholds of the 256x256 form, and a tile that would straddle two groups
    reset(); g.M = 767; expect(&g, &q, 3, "M 767");
    reset(); g.M = 1; g.N = 8; g.ldc = 8; q.group_cols = 0; q.lda2 = 128; expect(&g, &q, 3, "1 x 8");
    reset(); g.M = 2048; g.N = 3840; g.ldc = 3840; q.group_cols = 0; q.lda2 = 128; expect(&g, &q, 3, "120 tiles");
    reset(); q.group_cols = 128; q.lda2 = 48 * 128; expect(&g, &q, 3, "group_cols 128");
    g.algo = 256; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "group_cols 128 forced onto 256-column tiles");
    // extreme accepted geometry: the launcher's arithmetic at the edge of the 32-bit offsets
    reset(); g.M = 1 << 30; g.lda = (1 << 22) - 8; g.ldw = (1 << 22) - 8; q.lda2 = (1 << 22) - 8; q.ldw2 = (1 << 22) - 8;
    g.ldc = int64_t(1) << 40;
    expect(&g, &q, 4, "largest pitches");

    // refused second pairs
    reset(); q.A2 = nullptr; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "NULL A2");
    reset(); q.W2 = nullptr; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "NULL W2");
    for (int k2 : {0, -64, 32, 96, 0x7fffffc1}) {
        reset(); q.K2 = k2; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "bad K2");
    }
    for (int gcols : {-2048, 64, 192, 4096, 6144 * 2, 0x7fffff80}) {
        reset(); q.group_cols = gcols; q.lda2 = 1 << 20; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "bad group_cols");
    }
    reset(); g.a_kblock = 1024; g.a_kblock_stride = 14976 * 1024; g.lda = 1024; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "K-blocked A");
    reset(); g.a_kblock = 1000; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "a_kblock not dividing K");
    reset(); q.A2 = base + 8; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "A2 + 8 bytes");
    reset(); q.W2 = base + 8; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "W2 + 8 bytes");
    reset(); q.lda2 = 388; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "lda2 % 8");
    reset(); q.ldw2 = 132; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "ldw2 % 8");
    reset(); q.lda2 = 376; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "lda2 < groups * K2");
    reset(); q.ldw2 = 120; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "ldw2 < K2");
    reset(); q.lda2 = -384; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "negative lda2");
    for (int which = 0; which < 4; ++which) {
        reset();
        (which == 0 ? g.lda : which == 1 ? g.ldw : which == 2 ? q.lda2 : q.ldw2) = 1 << 22;
        expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "a 256-row panel of 2 GiB");
    }
    // the first pair's own refusals pass through
    reset(); g.K = 2047; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "K % 64");
    reset(); g.N = 6140; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "N % 8");
    reset(); g.M = 0; expect(&g, &q, LTXMI_ERR_INVALID_ARG, "M 0");
    reset(); g.A = base + 8; expect(&g, &q, LTXMI_ERR_UNSUPPORTED, "A + 8 bytes");

    printf("gemm_pair2_host_asan: %d calls, %d unexpected\n", g_calls, g_bad);
    return g_bad ? 1 : 0;
}
