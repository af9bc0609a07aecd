// t5_host_asan.cpp -- drives the HOST side of the four T5 entries (ltxmi_attention_relbias_bf16, ltxmi_rmsnorm_weight_bf16,
// ltxmi_gated_gelu_bf16, ltxmi_embedding_bf16) under AddressSanitizer.
//
// A stand-alone program (its own main), built by `make -C ltx-video-gpupoor_amd/csrc asan` against libltxmi_asan.so (host code
// instrumented, device code not) and run by tests/test_t5_native_asan.py with NO device visible, so nothing is ever launched:
// a call either is refused by the entry check (LTXMI_ERR_INVALID_ARG / _UNSUPPORTED) or runs the whole launcher -- instance
// choice, parameter block, grid arithmetic, the LDS reservation's per-device state -- up to the HIP call that reports the missing
// device (LTXMI_ERR_LAUNCH).  ASan aborts the process on any host-side out-of-bounds access on the way; the driver checks every
// status and that a failure left a message in ltxmi_last_error().
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ltxmi.h"

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

    // ---- attention with a relative bias
    ltxmi_attn_relbias_args a;
    auto reset = [&](int B, int H, int Lq, int Lk) {
        memset(&a, 0, sizeof a);
        a.q = base; a.k = base + 128 * H; a.v = base + 256 * H; a.o = base + (1 << 19);
        a.q_stride_l = a.k_stride_l = a.v_stride_l = 3 * H * 64;
        a.q_stride_b = a.k_stride_b = a.v_stride_b = (int64_t)512 * 3 * H * 64;
        a.o_stride_l = H * 64; a.o_stride_b = (int64_t)512 * H * 64;
        a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.head_dim = 64; a.softmax_scale = 1.0f;
        a.rel_bias = reinterpret_cast<const float*>(base + (1 << 18)); a.rel_center = Lq - 1; a.rel_stride_h = Lq + Lk - 1;
        a.key_bias = reinterpret_cast<const float*>(base + (1 << 17)); a.bias_stride_b = Lk;
    };
    expect(ltxmi_attention_relbias_bf16(nullptr, nullptr), LTXMI_ERR_INVALID_ARG, "attention: NULL struct");
    memset(&a, 0, sizeof a);
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_INVALID_ARG, "attention: zeroed struct");
    // accepted: every instance (1, 2, 4, 8, 16 steps of 32 keys), ragged sizes, the XXL workload, no key bias, no relative bias
    const int shapes[][4] = {{1, 1, 1, 1}, {2, 3, 24, 24}, {1, 3, 63, 63}, {2, 1, 64, 64}, {1, 3, 65, 65}, {2, 64, 128, 128},
                             {2, 64, 256, 256}, {1, 1, 257, 257}, {1, 3, 512, 512}, {2, 3, 100, 200}, {2, 3, 512, 1}, {1, 2, 1, 512}};
    for (const auto& s : shapes) {
        reset(s[0], s[1], s[2], s[3]);
        expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_LAUNCH, "attention: accepted shape");
        a.key_bias = nullptr;
        expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_LAUNCH, "attention: accepted shape, no key bias");
        a.rel_bias = nullptr; a.rel_center = 0; a.rel_stride_h = 0;
        expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_LAUNCH, "attention: accepted shape, plain attention");
    }
    reset(2, 64, 256, 256); a.rel_center = 300; a.rel_stride_h = 700;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_LAUNCH, "attention: a centre and a stride of the caller's");
    // refused
    reset(2, 2, 24, 24); a.head_dim = 128;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "attention: head_dim 128");
    reset(2, 2, 513, 24);
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "attention: Lq 513");
    reset(2, 2, 24, 513);
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "attention: Lk 513");
    reset(2, 2, 24, 513); a.rel_bias = nullptr;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "attention: Lk 513 without a relative bias");
    reset(2, 2, 24, 24); a.rel_center = 22;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_INVALID_ARG, "attention: centre below Lq - 1");
    reset(2, 2, 24, 24); a.rel_stride_h = 46;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_INVALID_ARG, "attention: stride below centre + Lk");
    reset(2, 2, 24, 24); a.Lk = 0;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_INVALID_ARG, "attention: Lk 0");
    reset(2, 2, 24, 24); a.B = -1;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_INVALID_ARG, "attention: B -1");
    reset(2, 2, 24, 24); a.v = nullptr;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_INVALID_ARG, "attention: NULL v");
    reset(2, 2, 24, 24); a.k_stride_l = 388;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "attention: stride % 8");
    reset(2, 2, 24, 24); a.q = base + 8;
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "attention: q off 16 bytes");
    reset(2, 2, 24, 24); a.rel_bias = reinterpret_cast<const float*>(base + 2);
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "attention: rel_bias off 4 bytes");
    reset(65536, 65535, 24, 24);
    expect(ltxmi_attention_relbias_bf16(&a, nullptr), LTXMI_ERR_UNSUPPORTED, "attention: grid too large");

    // ---- T5LayerNorm
    for (int D : {8, 512, 520, 2048, 2056, 4096, 4104, 8192})
        expect(ltxmi_rmsnorm_weight_bf16(p, D, base + (1 << 19), D + 8, 513, D, p, 1e-6f, nullptr), LTXMI_ERR_LAUNCH, "norm: accepted width");
    expect(ltxmi_rmsnorm_weight_bf16(p, 4096, base + (1 << 19), 4096, 4 * ((1 << 24) - 1), 4096, p, 1e-6f, nullptr), LTXMI_ERR_LAUNCH,
           "norm: the most rows a launch takes");
    expect(ltxmi_rmsnorm_weight_bf16(p, 4096, base + (1 << 19), 4096, 4 * ((1 << 24) - 1) + 1, 4096, p, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED,
           "norm: one row more");
    expect(ltxmi_rmsnorm_weight_bf16(p, 4096, base + (1 << 19), 4096, 2147483647, 4096, p, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "norm: 2^31 - 1 rows");
    expect(ltxmi_rmsnorm_weight_bf16(nullptr, 128, p, 128, 4, 128, p, 1e-6f, nullptr), LTXMI_ERR_INVALID_ARG, "norm: NULL x");
    expect(ltxmi_rmsnorm_weight_bf16(p, 128, p, 128, 4, 128, nullptr, 1e-6f, nullptr), LTXMI_ERR_INVALID_ARG, "norm: NULL weight");
    expect(ltxmi_rmsnorm_weight_bf16(p, 128, p, 128, 0, 128, p, 1e-6f, nullptr), LTXMI_ERR_INVALID_ARG, "norm: rows 0");
    expect(ltxmi_rmsnorm_weight_bf16(p, 128, p, 128, 4, 0, p, 1e-6f, nullptr), LTXMI_ERR_INVALID_ARG, "norm: D 0");
    expect(ltxmi_rmsnorm_weight_bf16(p, 128, p, 128, 4, 100, p, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "norm: D 100");
    expect(ltxmi_rmsnorm_weight_bf16(p, 8200, p, 8200, 4, 8200, p, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "norm: D 8200");
    expect(ltxmi_rmsnorm_weight_bf16(p, 64, p, 128, 4, 128, p, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "norm: ldx below D");
    expect(ltxmi_rmsnorm_weight_bf16(base + 8, 128, p, 128, 4, 128, p, 1e-6f, nullptr), LTXMI_ERR_UNSUPPORTED, "norm: x off 16 bytes");

    // ---- gated GELU: one trip, the grid cap, many trips
    expect(ltxmi_gated_gelu_bf16(p, 16, base + (1 << 19), 8, 1, 8, nullptr), LTXMI_ERR_LAUNCH, "gated: one chunk");
    expect(ltxmi_gated_gelu_bf16(p, 20480, base + (1 << 19), 10240, 512, 10240, nullptr), LTXMI_ERR_LAUNCH, "gated: the XXL shape");
    expect(ltxmi_gated_gelu_bf16(p, 20488, base + (1 << 19), 10248, 2147483647, 10240, nullptr), LTXMI_ERR_LAUNCH, "gated: 2^31 - 1 rows");
    expect(ltxmi_gated_gelu_bf16(nullptr, 16, p, 8, 1, 8, nullptr), LTXMI_ERR_INVALID_ARG, "gated: NULL h");
    expect(ltxmi_gated_gelu_bf16(p, 16, p, 8, 0, 8, nullptr), LTXMI_ERR_INVALID_ARG, "gated: rows 0");
    expect(ltxmi_gated_gelu_bf16(p, 16, p, 8, 1, -8, nullptr), LTXMI_ERR_INVALID_ARG, "gated: F -8");
    expect(ltxmi_gated_gelu_bf16(p, 24, p, 16, 1, 12, nullptr), LTXMI_ERR_UNSUPPORTED, "gated: F 12");
    expect(ltxmi_gated_gelu_bf16(p, 8, p, 8, 1, 8, nullptr), LTXMI_ERR_UNSUPPORTED, "gated: ldh below 2 F");
    expect(ltxmi_gated_gelu_bf16(p, 16, base + 4, 8, 1, 8, nullptr), LTXMI_ERR_UNSUPPORTED, "gated: y off 16 bytes");

    // ---- embedding
    const int64_t* ids = reinterpret_cast<const int64_t*>(base + (1 << 17));
    expect(ltxmi_embedding_bf16(ids, p, 4096, 32128, base + (1 << 19), 4096, 512, 4096, nullptr), LTXMI_ERR_LAUNCH, "embedding: the XXL shape");
    expect(ltxmi_embedding_bf16(ids, p, 16, 1, base + (1 << 19), 8, (1 << 24) - 1, 8, nullptr), LTXMI_ERR_LAUNCH, "embedding: 2^24 - 1 rows");
    expect(ltxmi_embedding_bf16(ids, p, 16, 1, base + (1 << 19), 8, 1 << 24, 8, nullptr), LTXMI_ERR_UNSUPPORTED, "embedding: 2^24 rows");
    expect(ltxmi_embedding_bf16(ids, p, 16, 1, base + (1 << 19), 8, 2147483647, 8, nullptr), LTXMI_ERR_UNSUPPORTED, "embedding: 2^31 - 1 rows");
    expect(ltxmi_embedding_bf16(nullptr, p, 128, 64, p, 128, 4, 128, nullptr), LTXMI_ERR_INVALID_ARG, "embedding: NULL ids");
    expect(ltxmi_embedding_bf16(ids, p, 128, 0, p, 128, 4, 128, nullptr), LTXMI_ERR_INVALID_ARG, "embedding: vocab 0");
    expect(ltxmi_embedding_bf16(ids, p, 128, 64, p, 128, 0, 128, nullptr), LTXMI_ERR_INVALID_ARG, "embedding: rows 0");
    expect(ltxmi_embedding_bf16(ids, p, 128, 64, p, 128, 4, 124, nullptr), LTXMI_ERR_UNSUPPORTED, "embedding: D 124");
    expect(ltxmi_embedding_bf16(ids, p, 120, 64, p, 128, 4, 128, nullptr), LTXMI_ERR_UNSUPPORTED, "embedding: ld_table below D");
    expect(ltxmi_embedding_bf16(reinterpret_cast<const int64_t*>(base + 4), p, 128, 64, p, 128, 4, 128, nullptr), LTXMI_ERR_UNSUPPORTED,
           "embedding: ids off 8 bytes");

    printf("t5_host_asan: %d calls, %d unexpected\n", g_calls, g_bad);
    return g_bad ? 1 : 0;
}
