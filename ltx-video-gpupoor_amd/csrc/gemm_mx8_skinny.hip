// gemm_mx8_skinny.hip -- ltxmi_gemm_mx8_skinny (include/ltxmi_mx_t5.h): the MX-FP8 GEMM of gemm_mx8_body.h for M <= 512 rows, the
// projections of the T5 encoder.  ltxmi_gemm_mx8's 256 x 256 tiles make 32 workgroups of M = 512, N = 4096; here an output tile
// is 128 x 64 or 64 x 64 (rows of activations x columns of weights), so that every T5 shape fills the 256 CUs, and each tile
// walks all of K alone: no split over K, no workgroup talks to another.
//
// What replaces the split is a ring of LDS stages filled by LDS-DMA, and more than one workgroup per CU.  A stage (one K-tile of
// 128 e4m3 bytes per row: the activation image, the weight image, one scale word per row) is 25 KB / 17 KB; the ring holds
// STAGES = 3 of them, so tiles kt + 1 and kt + 2 are in flight while tile kt is multiplied, and the LDS takes two workgroups of
// the 128 x 64 form (75 KB each) or three of the 64 x 64 form per CU.  Measured (profiles/t5_mx8.md): a ring of 4, one 128 x 64
// workgroup per CU, was 5 - 18 % slower on the wide outputs and no faster on the N = 4096 ones -- a K-tile costs a workgroup
// about 0.8 us whatever the depth, so a second resident workgroup buys more than a third tile in flight.  Per K-tile and wave:
// a COUNTED s_waitcnt vmcnt (the wave's pieces of tile kt have landed, those of the later tiles stay in flight) with lgkmcnt(0)
// (its reads of tile kt - 1 are done), one raw s_barrier -- a __syncthreads() would drain the DMAs -- then the refill of the slot
// tile kt - 1 left, then the reads and the MFMAs of tile kt.
//
// Numerics: the LDS image (128-byte rows, chunk c of row r at slot c ^ (r & 7)), the operand fragments (16-byte chunks h and
// h + 2 per k-step), the scale bytes and the C/D map are those of gemm_mx8_kernel.inc, the k-steps go in ascending order into
// one fp32 accumulator and the epilogue's additions are its additions: every output element sees exactly the sums ltxmi_gemm_mx8
// forms, and the result is bit-identical to it (tests/test_gpu_mxt_kernels.py).  Activations pass through LDS in whole 128-byte
// rows; 4 waves as 2 x 2, each 64 x 32 or 32 x 32 of the tile.
#include "gemm_mx8_body.h"
#include "../../include/ltxmi_mx_t5.h"

namespace ltxmi {

namespace skinny {

constexpr int BN = 64, NW = 4, STAGES = LTXMI_MXT_STAGES;
constexpr int SC_BYTES = NW * 64 * 4;       // a scale word per row, one 4-byte LDS-DMA lane each: every wave issues one (a counted
                                            // vmcnt wants the same number of DMAs from every wave), the spare lanes re-read a row
__host__ __device__ constexpr int stage_bytes(int BM) { return (BM + BN) * MX_BK + SC_BYTES; }
__host__ __device__ constexpr int smem_bytes(int BM) { return STAGES * stage_bytes(BM); }
static_assert(STAGES >= 3 && STAGES <= 6, "wait_for_tile() spells out the counts of a ring of 3 to 6 stages");
static_assert(smem_bytes(128) <= 160 * 1024 && 2 * smem_bytes(64) <= 160 * 1024, "at least one / two workgroups per CU");

// the wave's DMAs of tile kt have landed when at most `ahead` <= STAGES - 2 later tiles' (PIECES each) are outstanding; its LDS
// reads are done
template <int PIECES>
__device__ __forceinline__ void wait_for_tile(int ahead) {
    static_assert((STAGES - 2) * PIECES < 64, "vmcnt is a 6-bit count");
    if (STAGES >= 6 && ahead >= 4) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(4 * PIECES) : "memory");
    else if (STAGES >= 5 && ahead >= 3) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(3 * PIECES) : "memory");
    else if (STAGES >= 4 && ahead >= 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * PIECES) : "memory");
    else if (ahead >= 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PIECES) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

// RESID: C = R + acc (GATE_RESIDUAL without a gate table; R may alias C: a lane reads the elements it writes, before it writes)
template <int BM, bool RESID>
__global__ __launch_bounds__(NW * 64) void gemm_mx8_skinny_kernel(Mx8Params p) {
    constexpr int WM = BM / 2, WN = BN / 2;
    constexpr int MI = WM / 32;
    static_assert(WN == 32, "one weight fragment per wave and k-step");
    constexpr int A_INSTR = (BM / 8) / NW, B_INSTR = (BN / 8) / NW;
    constexpr int PIECES = A_INSTR + B_INSTR + 1;
    constexpr int A_BYTES = BM * MX_BK, B_BYTES = BN * MX_BK, STAGE = stage_bytes(BM);

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    // M-major: the (at most 8) workgroups that read one 64-row panel of W are neighbours, on one XCD where the grid allows
    const int tile = xcd_work_id();
    const int tm = tile % p.tiles_m, tn = tile / p.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- LDS-DMA sources, as gemm_mx8_kernel.inc: a wave-uniform tile origin plus a per-lane 32-bit byte offset.  Rows past M / N
    // re-read the last valid row; their results are never stored.
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
    // scale word r = wave * 64 + lane of a stage: the activation rows, then the weight rows, then spare words
    const uint8_t* sc_src;
    {
        const int r = wave * 64 + lane;
        sc_src = r < BM ? p.As + (int64_t)min(m0 + r, p.M - 1) * p.lda_s
                        : p.Ws + (int64_t)min(n0 + min(r - BM, BN - 1), p.N - 1) * p.ldw_s;
    }
    auto stage = [&](int buf, int kt) {
        char* sa = smem + buf * STAGE;
#pragma unroll
        for (int g = 0; g < A_INSTR; ++g) glds16(a_base + (a_src[g] + (uint32_t)(kt * MX_BK)), sa + (wave * A_INSTR + g) * 1024);
#pragma unroll
        for (int g = 0; g < B_INSTR; ++g)
            glds16(w_base + (b_src[g] + (uint32_t)(kt * MX_BK)), sa + A_BYTES + (wave * B_INSTR + g) * 1024);
        __builtin_amdgcn_global_load_lds((glb_void_ptr)(sc_src + kt * 4), (lds_void_ptr)(sa + A_BYTES + B_BYTES + wave * 256), 4, 0, 0);
    };

    // ---- fragment read offsets within a stage, k-step 0: lane l reads row l & 31, chunks h and h + 2 (k-step 1: ^ 64); rows 32
    // apart share row & 7, so fragment i is fragment 0 plus i * 4096
    const int frow = lane & 31, fh = lane >> 5;
    const int a_row0 = wm * WM + frow, b_row0 = wn * WN + frow;
    const int a_off = a_row0 * 128 + ((fh ^ (a_row0 & 7)) << 4);
    const int b_off = A_BYTES + b_row0 * 128 + ((fh ^ (b_row0 & 7)) << 4);
    const int a_sc = A_BYTES + B_BYTES + a_row0 * 4, b_sc = A_BYTES + B_BYTES + BM * 4 + b_row0 * 4;
    auto frag = [&](const char* st, int off) __attribute__((always_inline)) {
        const u32x4 lo = *(const u32x4*)(st + off), hi = *(const u32x4*)(st + (off ^ 32));
        return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    };

    f32x16 acc[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    const int nk = p.K / MX_BK;
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
        if (s < nk) stage(s, s);

    // a row's scale word of the K-tile holds its 4 blocks; k-step s, lane half h uses byte 2 s + h
    const int sh0 = 8 * fh, sh1 = 8 * fh + 16;
    int slot = 0;                                            // kt % STAGES
    for (int kt = 0; kt < nk; ++kt) {
        wait_for_tile<PIECES>(min(nk - 1 - kt, STAGES - 2));
        __builtin_amdgcn_s_barrier();
        // every wave's pieces of tile kt are in LDS and every wave is done with tile kt - 1: its slot takes tile kt + STAGES - 1
        if (kt + STAGES - 1 < nk) stage(slot == 0 ? STAGES - 1 : slot - 1, kt + STAGES - 1);
        const char* st = smem + slot * STAGE;
        const i32x8 wf0 = frag(st, b_off), wf1 = frag(st, b_off ^ 64);
        const uint32_t bsw = *(const uint32_t*)(st + b_sc);
        i32x8 af0[MI], af1[MI];
        uint32_t asw[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            af0[i] = frag(st, a_off + i * 4096);
            af1[i] = frag(st, (a_off ^ 64) + i * 4096);
            asw[i] = *(const uint32_t*)(st + a_sc + i * 128);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
            acc[i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf0, af0[i], acc[i], 0, 0, 0, (int)((bsw >> sh0) & 0xffu), 0,
                                                                     (int)((asw[i] >> sh0) & 0xffu));
#pragma unroll
        for (int i = 0; i < MI; ++i)
            acc[i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf1, af1[i], acc[i], 0, 0, 0, (int)((bsw >> sh1) & 0xffu), 0,
                                                                     (int)((asw[i] >> sh1) & 0xffu));
        slot = slot == STAGES - 1 ? 0 : slot + 1;
    }

    // ---- epilogue, the bf16 branch of gemm_mx8_kernel.inc.  acc[i][4 g + e]: row m = m0 + wm*WM + 32 i + (l & 31), column
    // n = n0 + wn*32 + 8 g + 4 h + e.  Every load is unconditional on a clamped address; masked lanes store at an offset outside
    // the descriptor, which the hardware drops.
    const int ecol = 4 * fh;
    __amdgpu_buffer_rsrc_t c_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(p.C, 0, (uint32_t)(((int64_t)(p.M - 1) * p.ldc + p.N) * 2), 0x00020000);
    const int nb = n0 + wn * WN;                             // N % 32 == 0: the 32 columns are in range together
    const bool n_ok = nb < p.N;
    const int nbc = n_ok ? nb : p.N - 32;
    u32x2 bias_v[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias_v[g] = p.bias ? *(const u32x2*)(p.bias + nbc + 8 * g + ecol) : u32x2{0u, 0u};
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int m = m0 + wm * WM + 32 * i + frow;
        const bool ok = n_ok && m < p.M;
        const int mc = m < p.M ? m : p.M - 1;
        float v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = acc[i][e];
        u32x2 rr_v[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (RESID) rr_v[g] = *(const u32x2*)(p.R + (int64_t)mc * p.ldr + nbc + 8 * g + ecol);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float* v4 = v + 4 * g;
            add_bf16x4(v4, bias_v[g]);
            if (RESID) add_bf16x4(v4, rr_v[g]);              // (bias is NULL here: (acc + 0) + r is acc + r however it is associated)
        }
        const uint32_t off = ok ? (uint32_t)(((int64_t)m * p.ldc + nb + ecol) * 2) : 0xfffffff0u;
#pragma unroll
        for (int g = 0; g < 4; ++g) __builtin_amdgcn_raw_buffer_store_b64(pack_bf16x4(v + 4 * g), c_rsrc, off, 16 * g, 0);
    }
}

// The checks and the plan: LTXMI_OK with p (its tile counts those of the form) and the form that runs, or the negative status.
static int plan(const ltxmi_gemm_mx8_args* a, int form, const char* what, Mx8Params& p, int& chosen) {
    if (const int rc = mx8_check_args(a, what, p)) return rc;
    LTXMI_REQUIRE(!a->Cq, LTXMI_ERR_UNSUPPORTED, "%s: bf16 output only (Cq set)", what);
    LTXMI_REQUIRE(a->epilogue == LTXMI_EPI_NONE || a->epilogue == LTXMI_EPI_GATE_RESIDUAL, LTXMI_ERR_UNSUPPORTED,
                  "%s: epilogue %d is not on this path (NONE or GATE_RESIDUAL)", what, a->epilogue);
    LTXMI_REQUIRE(!a->gate_table, LTXMI_ERR_UNSUPPORTED, "%s: a gate_table is not on this path", what);
    LTXMI_REQUIRE(!(a->epilogue == LTXMI_EPI_GATE_RESIDUAL && a->bias), LTXMI_ERR_UNSUPPORTED,
                  "%s: a bias together with GATE_RESIDUAL is not on this path", what);
    LTXMI_REQUIRE(a->M <= LTXMI_MXT_MAX_ROWS, LTXMI_ERR_UNSUPPORTED, "%s: M=%d is above the row limit %d (use ltxmi_gemm_mx8)", what,
                  a->M, LTXMI_MXT_MAX_ROWS);
    LTXMI_REQUIRE(form == LTXMI_MXT_FORM_AUTO || form == LTXMI_MXT_FORM_128X64 || form == LTXMI_MXT_FORM_64X64, LTXMI_ERR_UNSUPPORTED,
                  "%s: form %d names no tile form", what, form);
    const int tiles_n = (a->N + BN - 1) / BN;
    if (form == LTXMI_MXT_FORM_AUTO)
        form = (a->M > 256 && (int64_t)((a->M + 127) / 128) * tiles_n >= 256) ? LTXMI_MXT_FORM_128X64 : LTXMI_MXT_FORM_64X64;
    const int bm = form == LTXMI_MXT_FORM_128X64 ? 128 : 64;
    p.tiles_m = (a->M + bm - 1) / bm;
    p.tiles_n = tiles_n;
    chosen = form;
    return LTXMI_OK;
}

template <int BM>
static int launch(const Mx8Params& p, bool resid, hipStream_t stream, const char* what) {
    const dim3 grid(p.tiles_m * p.tiles_n), block(NW * 64);
    if (resid) return launch_with_lds<gemm_mx8_skinny_kernel<BM, true>>(p, grid, block, smem_bytes(BM), stream, what);
    return launch_with_lds<gemm_mx8_skinny_kernel<BM, false>>(p, grid, block, smem_bytes(BM), stream, what);
}

}  // namespace skinny

}  // namespace ltxmi

using namespace ltxmi;

extern "C" int ltxmi_gemm_mx8_skinny_form(const ltxmi_gemm_mx8_args* a, int32_t form) {
    Mx8Params p;
    int chosen = 0;
    if (const int rc = skinny::plan(a, form, "ltxmi_gemm_mx8_skinny", p, chosen)) return rc;
    return chosen;
}

extern "C" int ltxmi_gemm_mx8_skinny(const ltxmi_gemm_mx8_args* a, int32_t form, void* stream) {
    const char* what = "ltxmi_gemm_mx8_skinny";
    Mx8Params p;
    int chosen = 0;
    if (const int rc = skinny::plan(a, form, what, p, chosen)) return rc;
    const bool resid = a->epilogue == LTXMI_EPI_GATE_RESIDUAL;
    if (chosen == LTXMI_MXT_FORM_128X64) return skinny::launch<128>(p, resid, (hipStream_t)stream, what);
    return skinny::launch<64>(p, resid, (hipStream_t)stream, what);
}
