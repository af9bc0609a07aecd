// gemm_mx8.hip -- C[M,N] = epilogue(sum_k (Aq 2^ea)[m,k] (Wq 2^ew)[n,k] + bias[n]) on the block-scaled MFMA of gfx950
// (v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands: twice the bf16 rate per clock), fp32 accumulation.  include/ltxmi_mx.h.
//
// The tile kernel of gemm.hip carried over: 256 x 256 output tiles, 8 waves (2 x 4, 128 x 64 each), a K-tile of 128 e4m3 bytes
// per row -- as many LDS bytes per row as that kernel's 64 bf16 -- so the LDS image (128-byte rows, 16-byte chunk c of row r at
// slot c ^ (r & 7), the XOR applied to the LDS-DMA's SOURCE address and again on the read), the two stages with one
// __syncthreads() per K-tile are those of gemm_bf16_nt_kernel.
//
// The scaled 32x32x64 MFMA, as established with exact data by tests/test_gpu_mx8_kernels.py::test_layout_probe:
//   operand   lane l (r = l & 31, h = l >> 5) holds row r; bytes 0..15 of its 8 registers are k = 16 h + 0..15, bytes 16..31 are
//             k = 32 + 16 h + 0..15: the 16-byte chunks h and h + 2 of the row's 64 bytes, half of block 0 and half of block 1;
//   scale     lane l supplies the E8M0 byte of (row r, block h of the k-step) in bits [7:0] of the scale register (opsel 0);
//   C/D       the 32x32 bf16 map: column = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h.
// As in gemm.hip the WEIGHTS are the MFMA's A operand and the activations its B operand, so a lane holds 4 CONSECUTIVE output
// columns of one output row per register group (8-byte bf16 / 4-byte e4m3 stores), and the 32 columns of an MX output block are
// the 16 registers of one accumulator in the two lanes l, l ^ 32: the block amax is 15 in-lane maxima and one shuffle.
//
// A K-tile's scales are one 32-bit word per row (K % 128 == 0): each stage carries them behind the operand images, 256 + 256
// words, fetched by one 4-byte-per-lane LDS-DMA instruction per wave.
#include "epilogue.h"
#include "mx8.h"

namespace ltxmi {

typedef __attribute__((ext_vector_type(8))) int i32x8;      // one scaled-MFMA A/B fragment: 32 e4m3 bytes

struct Mx8Params {
    const uint8_t* A; int64_t lda; const uint8_t* As; int64_t lda_s;
    const uint8_t* W; int64_t ldw; const uint8_t* Ws; int64_t ldw_s;
    const uint16_t* bias;
    uint16_t* C; int64_t ldc;
    uint8_t* Cq; int64_t ldcq; uint8_t* Cs; int64_t ldc_s;
    int M, N, K;
    const uint16_t* R; int64_t ldr;
    const uint16_t* gate_table; const uint16_t* gate_temb; int64_t gate_ld; int rows_per_group;
    int tiles_m, tiles_n;
};

constexpr int MX_BM = 256, MX_BN = 256, MX_BK = 128;       // MX_BK: e4m3 elements = bytes of a row per K-tile
constexpr int MX_WAVES_M = 2, MX_WAVES_N = 4, MX_NW = MX_WAVES_M * MX_WAVES_N;
constexpr int MX_A_BYTES = MX_BM * MX_BK, MX_B_BYTES = MX_BN * MX_BK, MX_SC_BYTES = (MX_BM + MX_BN) * 4;
constexpr int MX_STAGE_BYTES = MX_A_BYTES + MX_B_BYTES + MX_SC_BYTES;
constexpr int MX_SMEM = 2 * MX_STAGE_BYTES;                 // 135168 B: one workgroup per CU
static_assert(MX_NW * 64 == MX_BM + MX_BN, "one scale word per row: one 4-byte LDS-DMA lane per row of the two images");

// MXOUT: write e4m3 + scales (Cq, Cs) instead of bf16 (C)
template <int EPI, bool MXOUT>
__global__ __launch_bounds__(MX_NW * 64) void gemm_mx8_kernel(Mx8Params p) {
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

    // ---- LDS-DMA sources: a wave-uniform tile origin plus a per-lane 32-bit byte offset (256 rows * ld < 2^31 is checked on
    // the host).  Rows past M / N re-read the last valid row; their results are never stored.
    const uint8_t* a_base = p.A + (int64_t)m0 * p.lda;
    const uint8_t* w_base = p.W + (int64_t)n0 * p.ldw;
    const int srow = lane >> 3, sslot = lane & 7;
    uint32_t a_src[A_INSTR], b_src[B_INSTR];
#pragma unroll
    for (int j = 0; j < A_INSTR; ++j) {
        const int row = (wave * A_INSTR + j) * 8 + srow;
        const int g = min(m0 + row, p.M - 1) - m0;
        a_src[j] = (uint32_t)g * (uint32_t)p.lda + ((sslot ^ (row & 7)) << 4);
    }
#pragma unroll
    for (int j = 0; j < B_INSTR; ++j) {
        const int row = (wave * B_INSTR + j) * 8 + srow;
        const int g = min(n0 + row, p.N - 1) - n0;
        b_src[j] = (uint32_t)g * (uint32_t)p.ldw + ((sslot ^ (row & 7)) << 4);
    }
    // the wave's 64 scale words of a K-tile: waves 0..3 rows wave*64 + lane of A, waves 4..7 rows (wave-4)*64 + lane of W
    const uint8_t* sc_src;
    {
        const int row = (wave & 3) * 64 + lane;
        sc_src = wave < 4 ? p.As + (int64_t)min(m0 + row, p.M - 1) * p.lda_s : p.Ws + (int64_t)min(n0 + row, p.N - 1) * p.ldw_s;
    }

    auto piece = [&](int buf, int kt, int g) {
        char* sa = smem + buf * MX_STAGE_BYTES;
        if (g < A_INSTR) glds16(a_base + (a_src[g] + (uint32_t)(kt * MX_BK)), sa + (wave * A_INSTR + g) * 1024);
        else if (g < A_INSTR + B_INSTR)
            glds16(w_base + (b_src[g - A_INSTR] + (uint32_t)(kt * MX_BK)), sa + MX_A_BYTES + (wave * B_INSTR + g - A_INSTR) * 1024);
        else
            __builtin_amdgcn_global_load_lds((glb_void_ptr)(sc_src + kt * 4), (lds_void_ptr)(sa + MX_A_BYTES + MX_B_BYTES + wave * 256),
                                             4, 0, 0);
    };
    constexpr int PIECES = A_INSTR + B_INSTR + 1;
    auto stage = [&](int buf, int kt) {
#pragma unroll
        for (int g = 0; g < PIECES; ++g) piece(buf, kt, g);
    };

    // ---- fragment read offsets within a stage, k-step 0: lane l reads row l & 31, chunks h and h + 2 (k-step 1: + 4).
    // Rows 32 apart share row & 7, so fragment i of a wave is fragment 0 plus i * 4096 in the instruction's offset field, and
    // one offset per operand (and its ^ 32, ^ 64 forms) is all that is held in registers.
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

    const int nk = p.K / MX_BK;
    stage(0, 0);
    if (nk > 1) stage(1, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // a row's scale word of the K-tile holds its 4 blocks; k-step s, lane half h uses byte 2 s + h.
    // Registers: 128 accumulators leave room for ONE k-step of fragments plus the next k-step's weight fragments.  An activation
    // fragment is re-read for the next k-step right behind the MFMAs that consumed it, so every fragment is still requested a
    // whole k-step (8 MFMAs) ahead of its use.
    i32x8 af[MI], bf[NI], bfn[NI];
    const int sh0 = 8 * fh, sh1 = 8 * fh + 16;
    uint32_t asw[MI], bsw[NI];
#pragma unroll
    for (int i = 0; i < MI; ++i) { af[i] = frag(0, a_off, i); asw[i] = scale_word(0, a_sc, i); }
#pragma unroll
    for (int j = 0; j < NI; ++j) { bf[j] = frag(0, b_off, j); bsw[j] = scale_word(0, b_sc, j); }

#define LTXMI_MX_MFMA(WF, AF, ACC, WS, AS) \
    ACC = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(WF, AF, ACC, 0, 0, 0, (int)(WS), 0, (int)(AS))

    // One K-tile.  REFILL / MORE (tile kt + 2 / kt + 1 exists) are compile-time: with run-time conditions inside, the body falls
    // into basic blocks, hipcc sinks the MFMAs below all of them (sched_barrier orders one block only) and keeps two copies of
    // every fragment alive across the joins.
    auto ktile = [&](int kt, auto refill_t, auto more_t) __attribute__((always_inline)) {
        constexpr bool refill = decltype(refill_t)::value, more = decltype(more_t)::value;
        const int cur = kt & 1;
        // opaque to the compiler: known as 0 / MX_STAGE_BYTES it unrolls the loop by two and keeps every fragment address of both
        // stages in a register of its own across the loop, and the accumulators spill
        uint32_t sb = cur * MX_STAGE_BYTES, sbn = (cur ^ 1) * MX_STAGE_BYTES;
        asm volatile("" : "+s"(sb), "+s"(sbn));
        // (the byte is cut out at the use, not at the read: the read's wait then stands in front of the MFMA, not behind the read)
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
        // every read of this stage is out; wait for them and for the LDS-DMA of tile kt + 1 (the explicit vmcnt wait: see
        // gemm_bf16_nt_kernel), then the stage may be refilled
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
                    if (i * PPR + q < PIECES) piece(cur, kt + 2, i * PPR + q);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) LTXMI_MX_MFMA(bfn[j], af[i], acc[i][j], bs1[j], as1[i]);
            if (more) { af[i] = frag(sbn, a_off, i); asw[i] = scale_word(sbn, a_sc, i); }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    for (int kt = 0; kt + 2 < nk; ++kt) ktile(kt, std::true_type{}, std::true_type{});
    if (nk >= 2) ktile(nk - 2, std::false_type{}, std::true_type{});
    ktile(nk - 1, std::false_type{}, std::false_type{});
#undef LTXMI_MX_MFMA

    // ---- epilogue.  acc[i][j][4 g + e]: row m = m0 + wm*WM + 32 i + (l & 31), column n = n0 + wn*WN + 32 j + 8 g + 4 h + e.
    // Every load is unconditional on a clamped address (gemm_tile.h says why).
    const int ecol = 4 * fh;
    // the outputs through buffer descriptors that end with the last element (sizes below 2^32 bytes: checked on the host)
    const auto rsrc = [](void* base, int64_t bytes) { return __builtin_amdgcn_make_buffer_rsrc(base, 0, (uint32_t)bytes, 0x00020000); };
    __amdgpu_buffer_rsrc_t c_rsrc = rsrc(p.C, MXOUT ? 0 : ((int64_t)(p.M - 1) * p.ldc + p.N) * 2);
    __amdgpu_buffer_rsrc_t cq_rsrc = rsrc(p.Cq, MXOUT ? (int64_t)(p.M - 1) * p.ldcq + p.N : 0);
    __amdgpu_buffer_rsrc_t cs_rsrc = rsrc(p.Cs, MXOUT ? (int64_t)(p.M - 1) * p.ldc_s + p.N / 32 : 0);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int nb = n0 + wn * WN + 32 * j;                    // N % 32 == 0: the 32 columns are in range together
        const bool n_ok = nb < p.N;
        const int nbc = n_ok ? nb : p.N - 32;
        u32x2 bias_v[4], gt_v[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bias_v[g] = p.bias ? *(const u32x2*)(p.bias + nbc + 8 * g + ecol) : u32x2{0u, 0u};
            if (GATED) gt_v[g] = *(const u32x2*)(p.gate_table + nbc + 8 * g + ecol);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = m0 + wm * WM + 32 * i + frow;
            const bool ok = n_ok && m < p.M;
            const int mc = m < p.M ? m : p.M - 1;
            float v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = acc[i][j][e];
            u32x2 ge_v[4], rr_v[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (GATED) ge_v[g] = *(const u32x2*)(p.gate_temb + (int64_t)(mc / p.rows_per_group) * p.gate_ld + nbc + 8 * g + ecol);
                if (RESID) rr_v[g] = *(const u32x2*)(p.R + (int64_t)mc * p.ldr + nbc + 8 * g + ecol);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float* v4 = v + 4 * g;
                add_bf16x4(v4, bias_v[g]);
                if (EPI == LTXMI_EPI_GELU_TANH) {
                    gelu_tanh_pk(v4[0], v4[1]);
                    gelu_tanh_pk(v4[2], v4[3]);
                }
                if (GATED) mul_sum_bf16x4(v4, gt_v[g], ge_v[g]);
                if (RESID) add_bf16x4(v4, rr_v[g]);
            }
            if constexpr (MXOUT) {
                float am = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) am = __builtin_fmaxf(am, __builtin_fabsf(v[e]));
                am = __builtin_fmaxf(am, __shfl_xor(am, 32, 64));
                const int byte = mx8_scale_byte(__float_as_uint(am));
                const float inv = mx8_inv_scale(byte);
                // masked lanes store at an offset outside the descriptor, which the hardware drops: no divergent branch in the
                // epilogue.  (With `if (ok)` around the stores hipcc spilled registers that live across the branch INSIDE it, under
                // the partial EXEC mask, and reloaded them behind it for all lanes: garbage in the ragged tiles of the gated
                // instance, the one with the most spills.)
                const uint32_t off = ok ? (uint32_t)((int64_t)m * p.ldcq + nb + ecol) : 0xfffffff0u;
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    __builtin_amdgcn_raw_buffer_store_b32(mx8_pack4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3], inv), cq_rsrc,
                                                          off, 8 * g, 0);
                const uint32_t soff = (ok && fh == 0) ? (uint32_t)((int64_t)m * p.ldc_s + (nb >> 5)) : 0xfffffff0u;
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)byte, cs_rsrc, soff, 0, 0);
            } else {
                const uint32_t off = ok ? (uint32_t)(((int64_t)m * p.ldc + nb + ecol) * 2) : 0xfffffff0u;
#pragma unroll
                for (int g = 0; g < 4; ++g) __builtin_amdgcn_raw_buffer_store_b64(pack_bf16x4(v + 4 * g), c_rsrc, off, 16 * g, 0);
            }
        }
    }
}

template <bool MXOUT>
static int launch_mx8(const Mx8Params& p, int epi, hipStream_t stream, const char* what) {
    const int grid = p.tiles_m * p.tiles_n;
    auto go = [&](auto e) {
        return launch_with_lds<gemm_mx8_kernel<decltype(e)::value, MXOUT>>(p, dim3(grid), dim3(MX_NW * 64), MX_SMEM, stream, what);
    };
    switch (epi) {
        case LTXMI_EPI_NONE: return go(epi_t<LTXMI_EPI_NONE>{});
        case LTXMI_EPI_GELU_TANH: return go(epi_t<LTXMI_EPI_GELU_TANH>{});
        default: break;
    }
    if constexpr (!MXOUT) {
        if (epi == LTXMI_EPI_GATE_RESIDUAL) return go(epi_t<LTXMI_EPI_GATE_RESIDUAL>{});
        if (epi == EPI_RESIDUAL) return go(epi_t<EPI_RESIDUAL>{});
    }
    set_error("%s: bad epilogue %d", what, epi);
    return LTXMI_ERR_INVALID_ARG;
}

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_gemm_mx8(const ltxmi_gemm_mx8_args* a, void* stream) {
    const char* what = "ltxmi_gemm_mx8";
    LTXMI_REQUIRE(a && a->Aq && a->A_scales && a->Wq && a->W_scales, LTXMI_ERR_INVALID_ARG, "%s: NULL argument", what);
    LTXMI_REQUIRE((a->C != nullptr) != (a->Cq != nullptr), LTXMI_ERR_INVALID_ARG, "%s: exactly one of C and Cq must be set", what);
    LTXMI_REQUIRE(!a->Cq || a->C_scales, LTXMI_ERR_INVALID_ARG, "%s: Cq without C_scales", what);
    LTXMI_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, LTXMI_ERR_INVALID_ARG, "%s: non-positive size M=%d N=%d K=%d", what, a->M, a->N,
                  a->K);
    const bool epi_ok = a->epilogue == LTXMI_EPI_NONE || a->epilogue == LTXMI_EPI_GELU_TANH ||
                        (a->epilogue == LTXMI_EPI_GATE_RESIDUAL && !a->Cq);
    LTXMI_REQUIRE(epi_ok, LTXMI_ERR_INVALID_ARG, "%s: bad epilogue %d%s", what, a->epilogue, a->Cq ? " for the MX output" : "");
    const bool resid = a->epilogue == LTXMI_EPI_GATE_RESIDUAL;
    if (resid) {
        LTXMI_REQUIRE(a->residual && a->ldr >= a->N && a->ldr % 4 == 0, LTXMI_ERR_INVALID_ARG,
                      "%s: GATE_RESIDUAL needs a residual with ldr >= N, ldr %% 4 == 0", what);
        if (a->gate_table)
            LTXMI_REQUIRE(a->gate_temb && a->rows_per_group > 0 && a->gate_ld % 4 == 0, LTXMI_ERR_INVALID_ARG,
                          "%s: gate_table given without gate_temb / rows_per_group", what);
    }
    LTXMI_REQUIRE(a->K % MX_BK == 0, LTXMI_ERR_UNSUPPORTED, "%s: K=%d must be a multiple of 128", what, a->K);
    LTXMI_REQUIRE(a->N % LTXMI_MX_BLOCK == 0, LTXMI_ERR_UNSUPPORTED, "%s: N=%d must be a multiple of 32", what, a->N);
    const int kb = a->K / LTXMI_MX_BLOCK, nblk = a->N / LTXMI_MX_BLOCK;
    LTXMI_REQUIRE(a->lda % 16 == 0 && a->ldw % 16 == 0 && a->lda >= a->K && a->ldw >= a->K &&
                      (((uintptr_t)a->Aq | (uintptr_t)a->Wq) & 15) == 0,
                  LTXMI_ERR_UNSUPPORTED, "%s: Aq and Wq must be 16-byte aligned with lda, ldw %% 16 == 0 and >= K", what);
    LTXMI_REQUIRE((int64_t)MX_BM * a->lda < (1ll << 31) && (int64_t)MX_BN * a->ldw < (1ll << 31), LTXMI_ERR_UNSUPPORTED,
                  "%s: 256 rows of Aq / Wq must span less than 2^31 bytes", what);
    LTXMI_REQUIRE(a->lda_s % 4 == 0 && a->ldw_s % 4 == 0 && a->lda_s >= kb && a->ldw_s >= kb &&
                      (((uintptr_t)a->A_scales | (uintptr_t)a->W_scales) & 3) == 0,
                  LTXMI_ERR_UNSUPPORTED, "%s: the scale arrays must be 4-byte aligned with lda_s, ldw_s %% 4 == 0 and >= K / 32", what);
    LTXMI_REQUIRE((((uintptr_t)a->bias) & 7) == 0, LTXMI_ERR_UNSUPPORTED, "%s: bias must be 8-byte aligned", what);
    if (a->C)
        LTXMI_REQUIRE(a->ldc % 4 == 0 && a->ldc >= a->N && (((uintptr_t)a->C) & 7) == 0, LTXMI_ERR_UNSUPPORTED,
                      "%s: C must be 8-byte aligned with ldc %% 4 == 0 and >= N", what);
    else
        LTXMI_REQUIRE(a->ldcq % 4 == 0 && a->ldcq >= a->N && a->ldc_s >= nblk && (((uintptr_t)a->Cq) & 3) == 0, LTXMI_ERR_UNSUPPORTED,
                      "%s: Cq must be 4-byte aligned with ldcq %% 4 == 0 and >= N, ldc_s >= N / 32", what);
    // the stores go through 32-bit offsets into descriptors that end with the last element; a masked lane stores at 0xfffffff0
    // (+ at most 48), which has to lie outside every descriptor
    constexpr int64_t SPAN = (1ll << 32) - 256;
    LTXMI_REQUIRE(a->C ? (int64_t)a->M * a->ldc * 2 < SPAN : ((int64_t)a->M * a->ldcq < SPAN && (int64_t)a->M * a->ldc_s < SPAN),
                  LTXMI_ERR_UNSUPPORTED, "%s: the output (and its scales) must span less than 2^32 - 256 bytes", what);
    if (resid)
        LTXMI_REQUIRE((((uintptr_t)a->residual | (uintptr_t)a->gate_table | (a->gate_table ? (uintptr_t)a->gate_temb : (uintptr_t)0)) & 7) == 0,
                      LTXMI_ERR_UNSUPPORTED, "%s: residual, gate_table and gate_temb must be 8-byte aligned", what);
    Mx8Params p = {};
    p.A = (const uint8_t*)a->Aq; p.lda = a->lda; p.As = (const uint8_t*)a->A_scales; p.lda_s = a->lda_s;
    p.W = (const uint8_t*)a->Wq; p.ldw = a->ldw; p.Ws = (const uint8_t*)a->W_scales; p.ldw_s = a->ldw_s;
    p.bias = (const uint16_t*)a->bias;
    p.C = (uint16_t*)a->C; p.ldc = a->ldc;
    p.Cq = (uint8_t*)a->Cq; p.ldcq = a->ldcq; p.Cs = (uint8_t*)a->C_scales; p.ldc_s = a->ldc_s;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.R = (const uint16_t*)a->residual; p.ldr = a->ldr;
    p.gate_table = (const uint16_t*)a->gate_table; p.gate_temb = (const uint16_t*)a->gate_temb; p.gate_ld = a->gate_ld;
    p.rows_per_group = a->rows_per_group > 0 ? a->rows_per_group : 1;
    p.tiles_m = (a->M + MX_BM - 1) / MX_BM;
    p.tiles_n = (a->N + MX_BN - 1) / MX_BN;
    LTXMI_REQUIRE((int64_t)p.tiles_m * p.tiles_n < (1ll << 31), LTXMI_ERR_UNSUPPORTED, "%s: too many tiles", what);
    const int epi = (resid && !a->gate_table) ? EPI_RESIDUAL : a->epilogue;
    return a->Cq ? launch_mx8<true>(p, epi, (hipStream_t)stream, what) : launch_mx8<false>(p, epi, (hipStream_t)stream, what);
}
