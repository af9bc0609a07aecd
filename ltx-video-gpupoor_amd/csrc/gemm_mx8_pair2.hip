// gemm_mx8_pair2.hip -- ltxmi_gemm_mx8_pair2 (include/ltxmi_mx_lora.h): the MX-FP8 GEMM with a SECOND operand pair, also in
// MX-FP8, that continues the K loop: LoRA adapters applied unmerged on a quantised linear.
//
//   C[M,N] = epi( Aq . Wq^T  +  A2q[M, g K2 .. (g+1) K2) . W2q^T  +  bias[N] ),    g = n / group_cols
//
// What gemm_pair2.hip is to gemm.hip: x.W^T + T.B^T is ONE GEMM over [x | T].[W | B]^T, so the stream of an output tile is
// nk1 + nk2 K-tiles of 128 bytes, tile kt < nk1 from (A, W) at byte kt * 128 with its scale words at kt * 4, tile kt >= nk1 from
// (A2 + g K2, W2) at (kt - nk1) * 128 with the scale words at (kt - nk1) * 4 (+ g K2 / 32 for A2).  The tiles are accumulated in
// that order, k-steps ascending, into the one set of accumulators, exactly as gemm_mx8_kernel.inc does for a K of K1 + K2: a
// call here gives the bits ltxmi_gemm_mx8 (ltxmi_gemm_mx8_rowsumsq) gives on the materialised concatenation.
//
// TWIN: the fragment maps, the register plan and the K-tile body below are a second copy of gemm_mx8_kernel.inc's.  A fix to
// one of them belongs in the other too.
// Geometry, LDS image, fragment and scale lane maps, the K-tile body (two stages, one barrier per K-tile, the last two tiles
// peeled under compile-time flags, the opaque stage offset) are gemm_mx8_kernel.inc's, restated here; the epilogue is the same
// text (gemm_mx8_epilogue.inc).  A second text and not a switch in gemm_mx8_kernel.inc, because the addressing differs:
// that kernel holds 4 + 4 per-lane source offsets and a 64-bit scale pointer, which a second pair with other pitches would
// double in a kernel that sits at 256 VGPRs.  Here, as in gemm_pair2.hip, every operand of a tile has a buffer descriptor (base
// = the tile's first row [+ the group's columns], num_records ending with its last valid row) and ONE 32-bit per-lane offset,
// the step from piece to piece is a scalar, and which pair a K-tile comes from is a wave-uniform select of descriptor, offset
// and step made ahead of phase A.  Rows past M / N are out of range for the descriptor and arrive as zero bytes: e4m3 +0 under
// the scale byte 0 (2^-127, not the NaN code 0xFF); their results are never stored.
#include "gemm_mx8_body.h"
#include "../../include/ltxmi_mx_lora.h"

namespace ltxmi {

struct Mx8Pair2Params : Mx8RssParams {
    const uint8_t* A2; int64_t lda2; const uint8_t* As2; int64_t lda2_s;
    const uint8_t* W2; int64_t ldw2; const uint8_t* Ws2; int64_t ldw2_s;
    int K2;
    int group_cols;                          // > 0 (one group: >= N)
};

template <int EPI, bool MXOUT, bool RSS>
__global__ __launch_bounds__(MX_NW * 64) void gemm_mx8_pair2_kernel(Mx8Pair2Params p) {
    static_assert(!RSS || (!MXOUT && EPI == LTXMI_EPI_NONE), "the row sums are those of the plain bf16 output");
    constexpr int WM = MX_BM / MX_WAVES_M, WN = MX_BN / MX_WAVES_N;
    constexpr int MI = WM / 32, NI = WN / 32;
    constexpr int A_INSTR = (MX_BM / 8) / MX_NW, B_INSTR = (MX_BN / 8) / MX_NW;
    constexpr bool GATED = (EPI == LTXMI_EPI_GATE_RESIDUAL);
    constexpr bool RESID = (EPI == LTXMI_EPI_GATE_RESIDUAL || EPI == EPI_RESIDUAL);

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / MX_WAVES_N, wn = wave % MX_WAVES_N;

    // tiles in bands of GN N-tiles, M-major inside a band, each XCD a contiguous run of tile ids (gemm.hip)
    const int tile = xcd_work_id();
    constexpr int GN = 8;
    const int band_sz = p.tiles_m * GN;
    const int band = tile / band_sz, rem = tile % band_sz;
    const int gn = min(GN, p.tiles_n - band * GN);
    const int tm = rem / gn, tn = band * GN + rem % gn;
    const int m0 = tm * MX_BM, n0 = tn * MX_BN;
    const int grp = n0 / p.group_cols;       // group_cols % MX_BN == 0: a tile lies in one group

    // ---- LDS-DMA sources: per pair two operand descriptors and the descriptor of the wave's scale rows (waves 0..3 rows
    // wave*64 + lane of A, waves 4..7 rows (wave-4)*64 + lane of W), and three per-lane byte offsets.  Piece q of an operand
    // is rows 8q .. 8q+7 of the tile: the offset of piece 0 (row srow, 16-byte slot sslot ^ srow) plus q * 8 rows.  Every
    // extent is below 2^31 bytes (256 rows of each array: checked on the host).
    using rsrc_t = __amdgpu_buffer_rsrc_t;
    const auto src = [](const uint8_t* base, int64_t bytes) {
        return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
    };
    const int srow = lane >> 3, sslot = lane & 7;
    const int rows_m = min(MX_BM, p.M - m0), rows_n = min(MX_BN, p.N - n0);
    const int kb1 = p.K / 32, kb2 = p.K2 / 32;
    const rsrc_t d_a = src(p.A + (int64_t)m0 * p.lda, (int64_t)(rows_m - 1) * p.lda + p.K);
    const rsrc_t d_w = src(p.W + (int64_t)n0 * p.ldw, (int64_t)(rows_n - 1) * p.ldw + p.K);
    const rsrc_t d_a2 = src(p.A2 + (int64_t)m0 * p.lda2 + (int64_t)grp * p.K2, (int64_t)(rows_m - 1) * p.lda2 + p.K2);
    const rsrc_t d_w2 = src(p.W2 + (int64_t)n0 * p.ldw2, (int64_t)(rows_n - 1) * p.ldw2 + p.K2);
    const bool sc_w = wave >= 4;
    const int sc_rows = sc_w ? rows_n : rows_m;
    const int sc_ld = (int)(sc_w ? p.ldw_s : p.lda_s), sc_ld2 = (int)(sc_w ? p.ldw2_s : p.lda2_s);
    const uint8_t* sc_p = sc_w ? p.Ws + (int64_t)n0 * p.ldw_s : p.As + (int64_t)m0 * p.lda_s;
    const uint8_t* sc_p2 = sc_w ? p.Ws2 + (int64_t)n0 * p.ldw2_s : p.As2 + (int64_t)m0 * p.lda2_s + (int64_t)grp * kb2;
    const rsrc_t d_s = src(sc_p, (int64_t)(sc_rows - 1) * sc_ld + kb1);
    const rsrc_t d_s2 = src(sc_p2, (int64_t)(sc_rows - 1) * sc_ld2 + kb2);
    const uint32_t slot16 = (uint32_t)((sslot ^ srow) << 4);
    const uint32_t aoff = (uint32_t)(srow * (int)p.lda) + slot16, woff = (uint32_t)(srow * (int)p.ldw) + slot16;
    const uint32_t a2off = (uint32_t)(srow * (int)p.lda2) + slot16, w2off = (uint32_t)(srow * (int)p.ldw2) + slot16;
    const uint32_t soff = (uint32_t)(((wave & 3) * 64 + lane) * sc_ld), s2off = (uint32_t)(((wave & 3) * 64 + lane) * sc_ld2);
    const int a_step = 8 * (int)p.lda, w_step = 8 * (int)p.ldw;                    // bytes per 8 rows
    const int a2_step = 8 * (int)p.lda2, w2_step = 8 * (int)p.ldw2;
    const int nk1 = p.K / MX_BK, nk = nk1 + p.K2 / MX_BK;                           // nk >= 2

    // one LDS-DMA piece of a K-tile: pieces 0..A_INSTR-1 are 8 activation rows x 128 B, the next B_INSTR weight rows, the last
    // the wave's 64 scale words.  (ta, tw, ts, av, wv, sv, as, ws, kt): the pair that K-tile comes from -- descriptors,
    // per-lane offsets, steps -- and the tile's index within its pair
    constexpr int PIECES = A_INSTR + B_INSTR + 1;
    auto piece = [&](int buf, rsrc_t ta, rsrc_t tw, rsrc_t ts, uint32_t av, uint32_t wv, uint32_t sv, int as, int ws, int kt, int g)
                     __attribute__((always_inline)) {
        char* sa = smem + buf * MX_STAGE_BYTES;
        if (g < A_INSTR) {
            const int q = wave * A_INSTR + g;
            blds16(ta, sa + q * 1024, av + (uint32_t)(q * as), kt * MX_BK);
        } else if (g < A_INSTR + B_INSTR) {
            const int q = wave * B_INSTR + (g - A_INSTR);
            blds16(tw, sa + MX_A_BYTES + q * 1024, wv + (uint32_t)(q * ws), kt * MX_BK);
        } else {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ts, (lds_void_ptr)(sa + MX_A_BYTES + MX_B_BYTES + wave * 256), 4, (int)sv, kt * 4,
                                                     0, 0);
        }
    };
    // the pair of K-tile KT of the stream: wave-uniform selects, no branch
#define LTXMI_MX_PAIR2_PICK(KT)                                                                                            \
    const bool second = (KT) >= nk1;                                                                                       \
    const rsrc_t st_a = second ? d_a2 : d_a, st_w = second ? d_w2 : d_w, st_s = second ? d_s2 : d_s;                       \
    const uint32_t st_av = second ? a2off : aoff, st_wv = second ? w2off : woff, st_sv = second ? s2off : soff;            \
    const int st_as = second ? a2_step : a_step, st_ws = second ? w2_step : w_step;                                        \
    const int st_kt = (KT) - (second ? nk1 : 0);
    // (descriptors can be captured by no lambda in the host pass: `piece` and `ktile` get them by value, the prologue's stages
    // are a macro)
#define LTXMI_MX_PAIR2_STAGE(BUF, KT)                                                                                      \
    {                                                                                                                      \
        LTXMI_MX_PAIR2_PICK(KT)                                                                                            \
        _Pragma("unroll") for (int g = 0; g < PIECES; ++g)                                                                 \
            piece(BUF, st_a, st_w, st_s, st_av, st_wv, st_sv, st_as, st_ws, st_kt, g);                                     \
    }

    // ---- fragment read offsets within a stage, k-step 0 (gemm_mx8_kernel.inc): lane l reads row l & 31, chunks h and h + 2
    // (k-step 1: + 4); fragment i of a wave is fragment 0 plus i * 4096
    const int frow = lane & 31, fh = lane >> 5;
    const int a_row0 = wm * WM + frow, b_row0 = wn * WN + frow;
    const int a_off = a_row0 * 128 + ((fh ^ (a_row0 & 7)) << 4);
    const int b_off = MX_A_BYTES + b_row0 * 128 + ((fh ^ (b_row0 & 7)) << 4);
    const int a_sc = MX_A_BYTES + MX_B_BYTES + a_row0 * 4, b_sc = MX_A_BYTES + MX_B_BYTES + MX_BM * 4 + b_row0 * 4;
    // sb: the stage's byte offset, kept opaque (see the loop) so that the per-stage addresses are formed at the read
    auto frag = [&](uint32_t sb, int off, int t) __attribute__((always_inline)) {
        const u32x4 lo = *(const u32x4*)(smem + (sb + off) + t * 4096), hi = *(const u32x4*)(smem + (sb + (off ^ 32)) + t * 4096);
        return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    };
    auto scale_word = [&](uint32_t sb, int off, int t) __attribute__((always_inline)) {
        return *(const uint32_t*)(smem + (sb + off) + t * 128);
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    LTXMI_MX_PAIR2_STAGE(0, 0)
    LTXMI_MX_PAIR2_STAGE(1, 1)
#undef LTXMI_MX_PAIR2_STAGE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // a row's scale word of the K-tile holds its 4 blocks; k-step s, lane half h uses byte 2 s + h.  The register plan is
    // gemm_mx8_kernel.inc's: ONE k-step of fragments plus the next k-step's weight fragments beside the 128 accumulators.
    i32x8 af[MI], bf[NI], bfn[NI];
    const int sh0 = 8 * fh, sh1 = 8 * fh + 16;
    uint32_t asw[MI], bsw[NI];
#pragma unroll
    for (int i = 0; i < MI; ++i) { af[i] = frag(0, a_off, i); asw[i] = scale_word(0, a_sc, i); }
#pragma unroll
    for (int j = 0; j < NI; ++j) { bf[j] = frag(0, b_off, j); bsw[j] = scale_word(0, b_sc, j); }

#define LTXMI_MX_MFMA(WF, AF, ACC, WS, AS) \
    ACC = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(WF, AF, ACC, 0, 0, 0, (int)(WS), 0, (int)(AS))

    // One K-tile of the stream (gemm_mx8_kernel.inc's, REFILL / MORE compile-time for its reasons); (ta .. t_kt): where tile
    // kt + 2 comes from, read under REFILL only
    auto ktile = [&](int kt, auto refill_t, auto more_t, rsrc_t ta, rsrc_t tw, rsrc_t ts, uint32_t av, uint32_t wv, uint32_t sv,
                     int as, int ws, int t_kt) __attribute__((always_inline)) {
        constexpr bool refill = decltype(refill_t)::value, more = decltype(more_t)::value;
        const int cur = kt & 1;
        // opaque to the compiler: known as 0 / MX_STAGE_BYTES it unrolls the loop by two and keeps every fragment address of
        // both stages in a register of its own across the loop, and the accumulators spill
        uint32_t sb = cur * MX_STAGE_BYTES, sbn = (cur ^ 1) * MX_STAGE_BYTES;
        asm volatile("" : "+s"(sb), "+s"(sbn));
        uint32_t as1[MI], bs1[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i) as1[i] = (asw[i] >> sh1) & 0xffu;
#pragma unroll
        for (int j = 0; j < NI; ++j) bs1[j] = (bsw[j] >> sh1) & 0xffu;
        // ---- phase A: k-step 0; the k-step-1 fragments of this stage read under it
#pragma unroll
        for (int j = 0; j < NI; ++j) bfn[j] = frag(sb, b_off ^ 64, j);
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int j = 0; j < NI; ++j) LTXMI_MX_MFMA(bf[j], af[i], acc[i][j], (bsw[j] >> sh0) & 0xffu, (asw[i] >> sh0) & 0xffu);
            af[i] = frag(sb, a_off ^ 64, i);
            __builtin_amdgcn_sched_barrier(0);
        }
        // every read of this stage is out; wait for them and for the LDS-DMA of tile kt + 1, then the stage may be refilled
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        // ---- phase B: k-step 1; k-step 0 of tile kt + 1 read from the other stage; tile kt + 2 requested into this one
        if (more) {
#pragma unroll
            for (int j = 0; j < NI; ++j) { bf[j] = frag(sbn, b_off, j); bsw[j] = scale_word(sbn, b_sc, j); }
        }
        constexpr int PPR = (PIECES + MI - 1) / MI;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            if (refill) {
#pragma unroll
                for (int q = 0; q < PPR; ++q)
                    if (i * PPR + q < PIECES) piece(cur, ta, tw, ts, av, wv, sv, as, ws, t_kt, i * PPR + q);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) LTXMI_MX_MFMA(bfn[j], af[i], acc[i][j], bs1[j], as1[i]);
            if (more) { af[i] = frag(sbn, a_off, i); asw[i] = scale_word(sbn, a_sc, i); }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    for (int kt = 0; kt + 2 < nk; ++kt) {
        // what phase B stages, chosen ahead of phase A: scalar work out of the way of the MFMAs behind the barrier
        LTXMI_MX_PAIR2_PICK(kt + 2)
        ktile(kt, std::true_type{}, std::true_type{}, st_a, st_w, st_s, st_av, st_wv, st_sv, st_as, st_ws, st_kt);
    }
    // (nk >= 2 always holds here.  The condition stays, as in gemm_mx8_kernel.inc: it keeps this tile in a block of its own.  With
    // both peeled tiles and the head of the epilogue in ONE block hipcc sinks their phase-B MFMAs below the epilogue's first
    // branch and spills about 100 fragment registers around them.)
    if (nk >= 2) ktile(nk - 2, std::false_type{}, std::true_type{}, d_a, d_w, d_s, aoff, woff, soff, a_step, w_step, 0);
    ktile(nk - 1, std::false_type{}, std::false_type{}, d_a, d_w, d_s, aoff, woff, soff, a_step, w_step, 0);
#undef LTXMI_MX_PAIR2_PICK
#undef LTXMI_MX_MFMA
    asm volatile("" ::: "memory");

#include "gemm_mx8_epilogue.inc"
}

// the seven instances: the six of ltxmi_gemm_mx8 and the row-sum form of ltxmi_gemm_mx8_rowsumsq
static int launch_mx8_pair2(const Mx8Pair2Params& p, int epi, bool mxout, bool rss, hipStream_t stream, const char* what) {
    const int grid = p.tiles_m * p.tiles_n;
    auto go = [&](auto e, auto mx, auto rs) {
        return launch_with_lds<gemm_mx8_pair2_kernel<decltype(e)::value, decltype(mx)::value, decltype(rs)::value>>(
            p, dim3(grid), dim3(MX_NW * 64), MX_SMEM, stream, what);
    };
    const std::true_type yes{};
    const std::false_type no{};
    if (rss) return go(epi_t<LTXMI_EPI_NONE>{}, no, yes);
    if (mxout) {
        if (epi == LTXMI_EPI_NONE) return go(epi_t<LTXMI_EPI_NONE>{}, yes, no);
        if (epi == LTXMI_EPI_GELU_TANH) return go(epi_t<LTXMI_EPI_GELU_TANH>{}, yes, no);
    } else {
        switch (epi) {
            case LTXMI_EPI_NONE: return go(epi_t<LTXMI_EPI_NONE>{}, no, no);
            case LTXMI_EPI_GELU_TANH: return go(epi_t<LTXMI_EPI_GELU_TANH>{}, no, no);
            case LTXMI_EPI_GATE_RESIDUAL: return go(epi_t<LTXMI_EPI_GATE_RESIDUAL>{}, no, no);
            case EPI_RESIDUAL: return go(epi_t<EPI_RESIDUAL>{}, no, no);
            default: break;
        }
    }
    set_error("%s: bad epilogue %d", what, epi);
    return LTXMI_ERR_INVALID_ARG;
}

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_gemm_mx8_pair2(const ltxmi_gemm_mx8_args* a, const ltxmi_gemm_mx8_pair* pr, float* rowsumsq,
                                    int32_t rowsumsq_cols, int64_t rowsumsq_ld, void* stream) {
    const char* what = "ltxmi_gemm_mx8_pair2";
    Mx8Pair2Params p = {};
    if (const int rc = mx8_check_args(a, what, p)) return rc;
    if (rowsumsq)
        if (const int rc = mx8_check_rss(a, rowsumsq, rowsumsq_cols, rowsumsq_ld, what, p)) return rc;
    LTXMI_REQUIRE(pr && pr->A2q && pr->A2_scales && pr->W2q && pr->W2_scales, LTXMI_ERR_INVALID_ARG, "%s: NULL second pair", what);
    LTXMI_REQUIRE(pr->K2 > 0 && pr->K2 % MX_BK == 0, LTXMI_ERR_INVALID_ARG, "%s: K2=%d must be a positive multiple of 128", what,
                  pr->K2);
    LTXMI_REQUIRE(pr->group_cols == 0 || (pr->group_cols > 0 && pr->group_cols % MX_BN == 0 && a->N % pr->group_cols == 0),
                  LTXMI_ERR_INVALID_ARG, "%s: group_cols=%d must be 0 or a multiple of 256 that divides N=%d", what, pr->group_cols,
                  a->N);
    const int64_t groups = pr->group_cols ? a->N / pr->group_cols : 1;
    const int64_t kb2 = pr->K2 / LTXMI_MX_BLOCK;
    LTXMI_REQUIRE(pr->lda2 % 16 == 0 && pr->ldw2 % 16 == 0 && pr->lda2 >= groups * pr->K2 && pr->ldw2 >= pr->K2 &&
                      (((uintptr_t)pr->A2q | (uintptr_t)pr->W2q) & 15) == 0,
                  LTXMI_ERR_UNSUPPORTED, "%s: A2q and W2q must be 16-byte aligned with lda2, ldw2 %% 16 == 0 and >= groups * K2, K2",
                  what);
    LTXMI_REQUIRE(pr->lda2_s % 4 == 0 && pr->ldw2_s % 4 == 0 && pr->lda2_s >= groups * kb2 && pr->ldw2_s >= kb2 &&
                      (((uintptr_t)pr->A2_scales | (uintptr_t)pr->W2_scales) & 3) == 0,
                  LTXMI_ERR_UNSUPPORTED,
                  "%s: the pair's scale arrays must be 4-byte aligned with lda2_s, ldw2_s %% 4 == 0 and >= groups * K2 / 32, K2 / 32", what);
    // every source goes through a buffer descriptor with 32-bit byte offsets, a tile of 256 rows each
    constexpr int64_t PANEL = 1ll << 31;
    LTXMI_REQUIRE(MX_BM * pr->lda2 < PANEL && MX_BN * pr->ldw2 < PANEL && MX_BM * pr->lda2_s < PANEL && MX_BN * pr->ldw2_s < PANEL &&
                      MX_BM * a->lda_s < PANEL && MX_BN * a->ldw_s < PANEL,
                  LTXMI_ERR_UNSUPPORTED, "%s: 256 rows of A2q, W2q or of a scale array must span less than 2^31 bytes", what);
    p.A2 = (const uint8_t*)pr->A2q; p.lda2 = pr->lda2; p.As2 = (const uint8_t*)pr->A2_scales; p.lda2_s = pr->lda2_s;
    p.W2 = (const uint8_t*)pr->W2q; p.ldw2 = pr->ldw2; p.Ws2 = (const uint8_t*)pr->W2_scales; p.ldw2_s = pr->ldw2_s;
    p.K2 = pr->K2;
    p.group_cols = pr->group_cols ? pr->group_cols : p.tiles_n * MX_BN;
    const int epi = (a->epilogue == LTXMI_EPI_GATE_RESIDUAL && !a->gate_table) ? EPI_RESIDUAL : a->epilogue;
    return launch_mx8_pair2(p, epi, a->Cq != nullptr, rowsumsq != nullptr, (hipStream_t)stream, what);
}
