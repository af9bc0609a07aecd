// gemm_mx8_kernel.inc -- the statements of the MX-FP8 GEMM kernels, included INSIDE a __global__ function that has
//   p                     its Mx8Params (by value, as the kernel argument);
//   EPI, MXOUT, RSS       compile-time constants: the epilogue, MXOUT = write e4m3 + scales (Cq, Cs) instead of bf16 (C), RSS = also
//                         p.rss[m * p.rss_ld + n / 64], the sums of squares of the stored bf16 values over each 64-column block
//                         below p.rss_cols (bf16 output only).
// Text and not a __device__ function template: called as one (params by reference or by value, force-inlined) the body sees its
// arguments as a copy or through a pointer instead of as the kernel argument segment, and the register allocation of the gated
// instance moved (43 spilled VGPRs became 18 or 32 under a K loop scheduled differently); tests/test_mx8_kernel_resources.py pins it.
// TWIN: gemm_mx8_pair2.hip holds a second copy of the fragment maps, the register plan and the K-tile body below, with its
// sources addressed through buffer descriptors.  A fix to one of them belongs in the other too.
static_assert(!RSS || !MXOUT, "the row sums are those of the bf16 output");
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

// ---- epilogue: the text the two-pair kernel (gemm_mx8_pair2.hip) shares
#include "gemm_mx8_epilogue.inc"
