// gemm_pair2.hip -- the bf16 "NT" GEMM with a SECOND operand pair that continues the K loop: LoRA adapters applied unmerged.
//
//   C[M,N] = epi( A[M,K] . W[N,K]^T  +  A2[M, g K2 .. (g+1) K2) . W2[N,K2]^T  +  bias[N] ),    g = n / group_cols
//
// (A, W) is the linear as stored in the checkpoint; A2 = bf16(x . down^T) [M, groups * K2] and W2 = the scaled up matrices
// [N, K2] are the adapter (ltxmi/lora.py).  x.W^T + T.B^T is ONE GEMM over [x | T].[W | B]^T, so the second pair is nothing
// but more K-tiles: the stream of an output tile is nk1 + nk2 tiles of 64, tile kt < nk1 from (A, W) at kt * 64, tile
// kt >= nk1 from (A2 + g K2, W2) at (kt - nk1) * 64, and every fused epilogue (GELU, gate + residual, the q row sums of
// squares) sees the adapter inside the accumulator.  The K-tiles are accumulated in that order, two 32-wide MFMA steps each,
// exactly as the kernels of gemm.hip do for a K of K1 + K2: a call here gives the bits ltxmi_gemm_bf16 gives on the
// materialised concatenation [A | A2_g], [W | W2].
//
// Loop: the non-persistent tile kernel's (gemm.hip) -- two LDS stages filled by LDS-DMA, one barrier per K-tile behind an explicit
// s_waitcnt vmcnt(0), the pieces of K-tile kt + 2 issued one group per MFMA row, fragments double-buffered in registers.
// Addressing: the persistent kernel's -- a buffer descriptor per operand and tile (base = the tile's first row [+ g K2 columns],
// num_records = its valid rows) plus ONE 32-bit per-lane offset per operand: the two pairs have different pitches, so that is
// four offset VGPRs, and which pair a K-tile comes from is a wave-uniform select of descriptor, offset and step.  Rows past
// M / N are out of range for the descriptor and arrive as zeros.
#include "gemm_tile.h"

namespace ltxmi {

struct Pair2Params {
    GemmParams g;                            // the first pair, the output and the epilogue's operands, as ltxmi_gemm_bf16 fills them
    const uint16_t* A2; int64_t lda2;
    const uint16_t* W2; int64_t ldw2;
    int K2;
    int group_cols;                          // > 0 (one group: >= N)
};

template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void gemm_bf16_nt_pair2_kernel(Pair2Params pp) {
    const GemmParams& p = pp.g;
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
    constexpr int MI = WM / 16, NI = WN / 16;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2;
    constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int A_INSTR = (BM / 8) / NW;   // LDS-DMA wave-instructions per wave per stage
    constexpr int B_INSTR = (BN / 8) / NW;
    static_assert((BM / 8) % NW == 0 && (BN / 8) % NW == 0, "tile rows must split over the waves");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;

    // ---- XCD-aware tile id, bands of GN N-tiles, M-major inside a band (gemm.hip)
    const int tile = xcd_work_id();
    constexpr int GN = 8;
    const int band_sz = p.tiles_m * GN;
    const int band = tile / band_sz, rem = tile % band_sz;
    const int gn = min(GN, p.tiles_n - band * GN);
    const int tm = rem / gn, tn = band * GN + rem % gn;
    const int m0 = tm * BM, n0 = tn * BN;
    const int grp = n0 / pp.group_cols;       // group_cols % BN == 0: a tile lies in one group

    // ---- LDS-DMA sources: four descriptors (scalars) and four per-lane byte offsets.  Piece q of an operand is rows
    // 8q .. 8q+7 of the tile: the offset of piece 0 (row srow, 16-byte slot sslot ^ srow) plus q * 8 rows.
    using rsrc_t = __amdgpu_buffer_rsrc_t;
    const int srow = lane >> 3, sslot = lane & 7;
    const int rows_m = min(BM, p.M - m0), rows_n = min(BN, p.N - n0);
    const rsrc_t d_a = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + (int64_t)m0 * p.lda), 0,
                                                         (int)(((int64_t)(rows_m - 1) * p.lda + p.K) * 2), 0x00020000);
    const rsrc_t d_w = __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (int64_t)n0 * p.ldw), 0,
                                                         (int)(((int64_t)(rows_n - 1) * p.ldw + p.K) * 2), 0x00020000);
    const rsrc_t d_a2 = __builtin_amdgcn_make_buffer_rsrc((void*)(pp.A2 + (int64_t)m0 * pp.lda2 + (int64_t)grp * pp.K2), 0,
                                                          (int)(((int64_t)(rows_m - 1) * pp.lda2 + pp.K2) * 2), 0x00020000);
    const rsrc_t d_w2 = __builtin_amdgcn_make_buffer_rsrc((void*)(pp.W2 + (int64_t)n0 * pp.ldw2), 0,
                                                          (int)(((int64_t)(rows_n - 1) * pp.ldw2 + pp.K2) * 2), 0x00020000);
    const uint32_t slot16 = (uint32_t)((sslot ^ srow) << 4);
    const uint32_t aoff = (uint32_t)(srow * (int)p.lda * 2) + slot16, woff = (uint32_t)(srow * (int)p.ldw * 2) + slot16;
    const uint32_t a2off = (uint32_t)(srow * (int)pp.lda2 * 2) + slot16, w2off = (uint32_t)(srow * (int)pp.ldw2 * 2) + slot16;
    const int a_step = 16 * (int)p.lda, w_step = 16 * (int)p.ldw;                  // bytes per 8 rows
    const int a2_step = 16 * (int)pp.lda2, w2_step = 16 * (int)pp.ldw2;
    const int nk1 = p.K / BK, nk = nk1 + pp.K2 / BK;                                // nk >= 2

    // one 1-KB LDS-DMA piece (8 rows x 128 B) of a K-tile: pieces 0..A_INSTR-1 are activation rows, the rest weight rows.
    // (ta, tw, av, wv, as, ws, kb): the pair that K-tile comes from -- descriptors, per-lane offsets, steps, byte offset in a row
    auto piece = [&](int buf, rsrc_t ta, rsrc_t tw, uint32_t av, uint32_t wv, int as, int ws, int kb, int g)
                     __attribute__((always_inline)) {
        char* sa = smem + buf * STAGE_BYTES;
        if (g < A_INSTR) {
            const int q = wave * A_INSTR + g;
            blds16(ta, sa + q * 1024, av + (uint32_t)(q * as), kb);
        } else {
            const int q = wave * B_INSTR + (g - A_INSTR);
            blds16(tw, sa + A_BYTES + q * 1024, wv + (uint32_t)(q * ws), kb);
        }
    };
    // the pair of K-tile KT of the stream: wave-uniform selects, no branch
#define LTXMI_PAIR2_PICK(KT)                                                              \
    const bool second = (KT) >= nk1;                                                      \
    const rsrc_t st_a = second ? d_a2 : d_a, st_w = second ? d_w2 : d_w;                  \
    const uint32_t st_av = second ? a2off : aoff, st_wv = second ? w2off : woff;          \
    const int st_as = second ? a2_step : a_step, st_ws = second ? w2_step : w_step;       \
    const int st_kb = ((KT) - (second ? nk1 : 0)) * (BK * 2);
    // (descriptors can be captured by no lambda in the host pass: `piece` gets them by value, the prologue's stages are a macro)
#define LTXMI_PAIR2_STAGE(BUF, KT)                                                                                       \
    {                                                                                                                    \
        LTXMI_PAIR2_PICK(KT)                                                                                             \
        _Pragma("unroll") for (int g = 0; g < A_INSTR + B_INSTR; ++g)                                                    \
            piece(BUF, st_a, st_w, st_av, st_wv, st_as, st_ws, st_kb, g);                                                \
    }

    // ---- fragment read offsets (bytes within a stage), k-step 0: fragment i of a wave sits 16 rows = 2048 bytes below
    // fragment i - 1 with the same (row & 7), so one base per operand plus immediates addresses all of them
    const int frow = lane & 15, fchunk = lane >> 4;
    const int a_off0 = (wm * WM + frow) * 128 + ((fchunk ^ (frow & 7)) << 4);
    const int b_off0 = A_BYTES + (wn * WN + frow) * 128 + ((fchunk ^ (frow & 7)) << 4);
    const int a_off1 = a_off0 ^ 64, b_off1 = b_off0 ^ 64;

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- main loop (gemm.hip's tile kernel): phase A = MFMAs on the k-step-0 fragments || ds_read k-step 1; barrier;
    // phase B = LDS-DMA of tile kt + 2 into the stage just drained, MFMAs on k-step 1 || ds_read k-step 0 of tile kt + 1
    LTXMI_PAIR2_STAGE(0, 0)
    LTXMI_PAIR2_STAGE(1, 1)
#undef LTXMI_PAIR2_STAGE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    bf16x8 af0[MI], bf0[NI], af1[MI], bf1[NI];
#pragma unroll
    for (int i = 0; i < MI; ++i) af0[i] = *(const bf16x8*)(smem + a_off0 + i * 2048);
#pragma unroll
    for (int j = 0; j < NI; ++j) bf0[j] = *(const bf16x8*)(smem + b_off0 + j * 2048);

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const char* s = smem + cur * STAGE_BYTES;
        // what phase B stages, chosen before phase A: scalar work out of the way of the MFMAs behind the barrier
        LTXMI_PAIR2_PICK(kt + 2)
        constexpr int MI_HEAD = MI > 2 ? 2 : 1;
#pragma unroll
        for (int i = 0; i < MI_HEAD; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf0[j], af0[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < MI; ++i) af1[i] = *(const bf16x8*)(s + a_off1 + i * 2048);
#pragma unroll
        for (int j = 0; j < NI; ++j) bf1[j] = *(const bf16x8*)(s + b_off1 + j * 2048);
#pragma unroll
        for (int i = MI_HEAD; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf0[j], af0[i], acc[i][j], 0, 0, 0);
        // phase A's MFMAs stay on this side of the barrier, and the LDS-DMA is waited for explicitly: hipcc's own
        // __syncthreads() lowering waits for lgkmcnt only across the loop back-edge (the note in gemm.hip's tile kernel)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        const bool refill = kt + 2 < nk;
        if (kt + 1 < nk) {
            const char* sn = smem + (cur ^ 1) * STAGE_BYTES;
#pragma unroll
            for (int i = 0; i < MI; ++i) af0[i] = *(const bf16x8*)(sn + a_off0 + i * 2048);
#pragma unroll
            for (int j = 0; j < NI; ++j) bf0[j] = *(const bf16x8*)(sn + b_off0 + j * 2048);
        }
        constexpr int PPR = (A_INSTR + B_INSTR + MI - 1) / MI;        // pieces per MFMA row
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            if (refill) {
#pragma unroll
                for (int q = 0; q < PPR; ++q)
                    if (i * PPR + q < A_INSTR + B_INSTR)
                        piece(cur, st_a, st_w, st_av, st_wv, st_as, st_ws, st_kb, i * PPR + q);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf1[j], af1[i], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef LTXMI_PAIR2_PICK

    // ---- epilogue: the tile kernel's (gemm_tile.h); a missing bias is gemm.hip's zero page with stride 0, and selected to zero
    tile_epilogue<EPI, residual_joins_bias_first(BM), /*BIAS_SELECT=*/true>(epi_args(p), acc, m0 + wm * WM, n0 + wn * WN, lane & 15, (lane >> 4) * 4);
}

template <int BM, int BN, int WAVES_M, int WAVES_N>
static int launch_pair2(const Pair2Params& p0, int epi, hipStream_t stream, const char* what) {
    Pair2Params p = p0;
    p.g.tiles_m = (p.g.M + BM - 1) / BM;
    p.g.tiles_n = (p.g.N + BN - 1) / BN;
    const int grid = p.g.tiles_m * p.g.tiles_n;
    constexpr int threads = WAVES_M * WAVES_N * 64;
    constexpr int smem = 2 * (BM + BN) * BK * 2;
    auto go = [&](auto e) {
        return launch_with_lds<gemm_bf16_nt_pair2_kernel<BM, BN, WAVES_M, WAVES_N, decltype(e)::value>>(p, dim3(grid), dim3(threads),
                                                                                                 smem, stream, what);
    };
    return dispatch_epilogue(epi, go, what);
}

}  // namespace ltxmi

using namespace ltxmi;

// Kernels behind ltxmi_gemm_pair2_bf16, as ltxmi_gemm_pair2_kernel_id reports them (0 .. 2 are ltxmi_gemm_bf16's)
enum { GEMM_PAIR2_TILE128 = 3, GEMM_PAIR2_TILE256 = 4 };

// Validates a two-pair call and picks its kernel: the launch runs what this returns, the id query reports it.  Host arithmetic
// on the two structs only.  The first pair's checks are ltxmi_gemm_bf16's own, made by its own code (ltxmi_gemm_kernel_id).
static int pair2_plan(const ltxmi_gemm_args* a, const ltxmi_gemm_pair* p, const char* what) {
    const int base = ltxmi_gemm_kernel_id(a);
    if (base < 0) return base;
    LTXMI_REQUIRE(p && p->A2 && p->W2, LTXMI_ERR_INVALID_ARG, "%s: NULL second pair", what);
    LTXMI_REQUIRE(p->K2 > 0 && p->K2 % 64 == 0, LTXMI_ERR_INVALID_ARG, "%s: K2=%d must be a positive multiple of 64", what, p->K2);
    LTXMI_REQUIRE(p->group_cols == 0 || (p->group_cols > 0 && a->N % p->group_cols == 0 && p->group_cols % 128 == 0),
                  LTXMI_ERR_INVALID_ARG, "%s: group_cols=%d must be 0 or a multiple of 128 that divides N=%d", what, p->group_cols,
                  a->N);
    LTXMI_REQUIRE(a->algo != 256 || p->group_cols % 256 == 0, LTXMI_ERR_INVALID_ARG,
                  "%s: algo 256 needs group_cols=%d to be a multiple of 256", what, p->group_cols);
    LTXMI_REQUIRE(a->a_kblock == 0, LTXMI_ERR_UNSUPPORTED, "%s: a K-blocked A takes no second pair", what);
    const int64_t groups = p->group_cols ? a->N / p->group_cols : 1;
    LTXMI_REQUIRE(p->lda2 % 8 == 0 && p->ldw2 % 8 == 0 && p->lda2 >= groups * p->K2 && p->ldw2 >= p->K2, LTXMI_ERR_UNSUPPORTED,
                  "%s: bad leading dimensions lda2=%lld ldw2=%lld", what, (long long)p->lda2, (long long)p->ldw2);
    LTXMI_REQUIRE((((uintptr_t)p->A2 | (uintptr_t)p->W2) & 15) == 0, LTXMI_ERR_UNSUPPORTED,
                  "%s: A2 and W2 must be 16-byte aligned", what);
    // the operands go through buffer descriptors with 32-bit byte offsets, a tile of up to 256 rows each
    LTXMI_REQUIRE((int64_t)256 * a->lda * 2 < (1ll << 31) && (int64_t)256 * a->ldw * 2 < (1ll << 31) &&
                      (int64_t)256 * p->lda2 * 2 < (1ll << 31) && (int64_t)256 * p->ldw2 * 2 < (1ll << 31),
                  LTXMI_ERR_UNSUPPORTED, "%s: a 256-row operand panel spans 2 GiB or more", what);
    if (a->algo == 128) return GEMM_PAIR2_TILE128;
    if (a->algo == 256) return GEMM_PAIR2_TILE256;
    const long t256 = (long)((a->M + 255) / 256) * ((a->N + 255) / 256);
    return a->M >= 768 && a->N >= 256 && t256 >= 128 && p->group_cols % 256 == 0 ? GEMM_PAIR2_TILE256 : GEMM_PAIR2_TILE128;
}

extern "C" int ltxmi_gemm_pair2_kernel_id(const ltxmi_gemm_args* a, const ltxmi_gemm_pair* p) {
    return pair2_plan(a, p, "ltxmi_gemm_pair2_kernel_id");
}

extern "C" int ltxmi_gemm_pair2_bf16(const ltxmi_gemm_args* a, const ltxmi_gemm_pair* pr, void* stream) {
    const int kernel = pair2_plan(a, pr, "ltxmi_gemm_pair2_bf16");
    if (kernel < 0) return kernel;
    Pair2Params p = {};
    int epi = 0;
    if (const int rc = gemm_dense_params(&p.g, &epi, a, "ltxmi_gemm_pair2_bf16")) return rc;
    p.A2 = (const uint16_t*)pr->A2; p.lda2 = pr->lda2;
    p.W2 = (const uint16_t*)pr->W2; p.ldw2 = pr->ldw2;
    p.K2 = pr->K2;
    p.group_cols = pr->group_cols ? pr->group_cols : ((a->N + 255) / 256) * 256;
    hipStream_t s = (hipStream_t)stream;
    if (kernel == GEMM_PAIR2_TILE256) return launch_pair2<256, 256, 2, 4>(p, epi, s, "ltxmi_gemm_pair2_bf16");
    return launch_pair2<128, 128, 2, 2>(p, epi, s, "ltxmi_gemm_pair2_bf16");
}
