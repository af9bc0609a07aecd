// gemm_tile.h -- what the non-persistent tile kernels of gemm.hip (dense and implicit-GEMM convolution) and gemm_pair2.hip (two
// operand pairs) have in common: the parameter struct, the tile epilogue with the struct it reads, and the host glue that
// fills the one and picks the instance of the other.  The persistent kernel of gemm.hip has a loop and an epilogue of its own
// and shares only the struct and the host glue.
#pragma once
#include "epilogue.h"

namespace ltxmi {

struct GemmParams {
    const uint16_t* A; int64_t lda;
    const uint16_t* W; int64_t ldw;
    const uint16_t* bias; int bias_stride;   // never NULL: a zero page with stride 0 stands in for "no bias"
    uint16_t* C; int64_t ldc;
    int M, N, K;
    const uint16_t* R; int64_t ldr;
    const uint16_t* gate_table;
    const uint16_t* gate_temb;
    int64_t gate_ld;
    int rows_per_group;
    int tiles_m, tiles_n;
    // implicit-GEMM convolution (MODE == 1): A rows are gathered from x [B,T,H,W,Cin]
    int cB, cT, cH, cW, cCin;      // input grid
    int oT, oH, oW;                 // output grid (== input grid unless strided / extended in time)
    int sT, sHW;                    // strides (1 or 2)
    int tzero;                      // time padding with zeros (plain nn.Conv3d) instead of frame replication
    int tpad;            // frames replicated in front (2 causal, 1 otherwise)
    int pad_replicate;   // spatial padding mode
    // depth-to-space epilogue (EPI == EPI_D2S)
    const uint16_t* res; int res_ch;
    // EPI_SUMSQ: fp32 [M, sumsq_ld] partial row sums of squares of the bf16 outputs, one per 64-column block
    float* sumsq; int sumsq_cols; int64_t sumsq_ld;
    // A whose K axis is cut into blocks of a_kblk elements lying a_kblk_stride elements apart (0 = plain): the receive
    // buffer of the Ulysses return all-to-all, [P source ranks][rows][D / P], is consumed in place by to_out
    int a_kblk; int64_t a_kblk_stride;

    __device__ __forceinline__ int64_t a_koff_elems(int kk) const { // element offset of column kk inside a row of A
        if (a_kblk <= 0) return kk;
        const int blk = kk / a_kblk;
        return (int64_t)blk * a_kblk_stride + (kk - blk * a_kblk);
    }
    __device__ __forceinline__ int64_t a_koff(int kt) const { return a_koff_elems(kt * 64); }   // ... of k-tile kt
};

constexpr int BK = 64;

// ---- host glue (defined in gemm.hip, next to the zero page)
// what the dense call and the convolution have in common: operands, output, shape; everything else of *p stays as the caller's
// `GemmParams p = {}` left it.  A missing bias is the zero page with stride 0.
int gemm_params(GemmParams* p, const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, void* C, int64_t ldc, int M,
                int N, int K, const char* what);
// every field of a dense call (ltxmi_gemm_bf16, and the first pair of ltxmi_gemm_pair2_bf16) and the epilogue it runs: the
// public value, or EPI_SUMSQ / EPI_RESIDUAL
int gemm_dense_params(GemmParams* p, int* epi, const ltxmi_gemm_args* a, const char* what);

// run-time epilogue -> go(epi_t<E>{}), which launches that instance; the ONE list of the dense epilogues
template <class Go>
static int dispatch_epilogue(int epi, Go&& go, const char* what) {
    switch (epi) {
        case LTXMI_EPI_NONE: return go(epi_t<LTXMI_EPI_NONE>{});
        case EPI_SUMSQ: return go(epi_t<EPI_SUMSQ>{});
        case LTXMI_EPI_GELU_TANH: return go(epi_t<LTXMI_EPI_GELU_TANH>{});
        case LTXMI_EPI_SILU: return go(epi_t<LTXMI_EPI_SILU>{});
        case LTXMI_EPI_GATE_RESIDUAL: return go(epi_t<LTXMI_EPI_GATE_RESIDUAL>{});
        case EPI_RESIDUAL: return go(epi_t<EPI_RESIDUAL>{});
        default: set_error("%s: bad epilogue %d", what, epi); return LTXMI_ERR_INVALID_ARG;
    }
}

// ---- the tile epilogue.  acc[i][j][e]: row m = row0 + i*16 + erow, col n = col0 + j*16 + ecol + e, with the wave's sub-tile
// origin (row0, col0) = (m0 + wm*WM, n0 + wn*WN) and the lane's place (erow, ecol) = (lane & 15, (lane >> 4) * 4).
// Every load below is unconditional (masked lanes read a clamped address): a runtime-conditional
// load makes hipcc branch around it and wait vmcnt(0) per element -- 32 dependent L2 round trips.
//
// What it reads comes as a small struct BY VALUE, filled from the kernel's own parameter struct by epi_args().  Found with
// tools/codegen_diff.py --sequence against the code with the epilogue written out in each kernel:
//   * through a `const GemmParams&` the callee has to assume that its stores alias the struct and re-reads fields after every
//     store: every tile instance grew by 3-5 % in instructions (v_mul_lo_u32, v_mad_u64_u32, v_lshl_add_u64);
//   * the whole GemmParams by value left the K loops alone but fetched the kernel arguments of the residual epilogues in other
//     pieces, in front of the K loop, and the 256x256 instance measured 1.7 % slower on a K = 8192 shape; with the fields
//     picked out by the kernel everything up to the epilogue is the written-out code, instruction for instruction;
//   * the four ints are expressions of the KERNEL: formed in here from m0, wm, lane ..., hipcc simplifies them on their own
//     before inlining (their sub-expressions then have one use less in the kernel), and the fragment offsets in front of the
//     K loop and the piece offsets inside it moved in the two-pair kernels and in 11 instances of gemm.hip.
struct EpiArgs {
    const uint16_t* bias; int bias_stride;
    uint16_t* C; int64_t ldc;
    int M, N;
    const uint16_t* R; int64_t ldr;
    const uint16_t* gate_table;
    const uint16_t* gate_temb;
    int64_t gate_ld;
    int rows_per_group;
    float* sumsq; int sumsq_cols; int64_t sumsq_ld;
    int cT, cH, cW; const uint16_t* res; int res_ch;         // EPI_D2S only
};
__device__ __forceinline__ EpiArgs epi_args(const GemmParams& p) {
    return {p.bias, p.bias_stride, p.C, p.ldc, p.M, p.N, p.R, p.ldr, p.gate_table, p.gate_temb, p.gate_ld, p.rows_per_group,
            p.sumsq, p.sumsq_cols, p.sumsq_ld, p.cT, p.cH, p.cW, p.res, p.res_ch};
}

// EPI_RESIDUAL is acc + bias + residual.  Written as two adds and left to -ffast-math, hipcc associated it per instance: bias +
// residual first in the 128-row tile kernels, acc + bias first in the 256-row ones and in the persistent kernel -- in gemm.hip
// and gemm_pair2.hip alike, so that a two-pair call gave the bits of the plain call the dispatcher picks for the same shape.
// It is now written down, per tile form, as it was (one bf16 ulp in a few outputs per million hangs on it); a new tile form
// has to say which it takes.  So `algo = 128` and `algo = 256` differ by that ulp under EPI_RESIDUAL, as they always did.
constexpr bool residual_joins_bias_first(int BM) { return BM == 128; }

// BIAS_SELECT (the two-pair kernels): the bias read through the zero page is also selected against zero where bias_stride is 0,
// as those kernels always did.  Same bits.  Without the select hipcc lays the masked store blocks of the two-pair epilogue out
// of line -- the common case, every lane in range, then takes a branch there and one back per 16-column fragment, each block
// behind its own s_waitcnt vmcnt(0) (+31 instructions) -- and the 256x256 GELU instance measured 0.4 to 1.3 % slower at M = 4992 in five runs of five
// (profiles/shared_parts_ab.md).  The instances of gemm.hip never had the select and are laid out as they were.
template <int EPI, bool RESIDUAL_JOINS_BIAS_FIRST, bool BIAS_SELECT = false, int MI, int NI>
__device__ __forceinline__ void tile_epilogue(const EpiArgs p, const f32x4 (&acc)[MI][NI], int row0, int col0, int erow, int ecol) {
    constexpr bool GATED = (EPI == LTXMI_EPI_GATE_RESIDUAL);
    constexpr bool RESID = (EPI == LTXMI_EPI_GATE_RESIDUAL || EPI == EPI_RESIDUAL);
    u32x2 bias_v[NI], gt_v[NI];
    int ncl[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int n = col0 + j * 16 + ecol;
        ncl[j] = n < p.N ? n : p.N - 4;
        bias_v[j] = *(const u32x2*)(p.bias + ncl[j] * p.bias_stride);
        if (BIAS_SELECT) bias_v[j] = p.bias_stride ? bias_v[j] : u32x2{0u, 0u};
        if (GATED) gt_v[j] = *(const u32x2*)(p.gate_table + ncl[j]);
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int m = row0 + i * 16 + erow;
        const bool m_ok = m < p.M;
        const int mc = m_ok ? m : p.M - 1;
        const uint16_t* gate_row = GATED ? p.gate_temb + (int64_t)(mc / p.rows_per_group) * p.gate_ld : nullptr;
        float ss[NI / 4 > 0 ? NI / 4 : 1];                       // EPI_SUMSQ: one partial per 64 columns (4 fragments)
#pragma unroll
        for (int q = 0; q < (NI / 4 > 0 ? NI / 4 : 1); ++q) ss[q] = 0.f;
        u32x2 ge_v[NI], rr_v[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            if (GATED) ge_v[j] = *(const u32x2*)(gate_row + ncl[j]);
            if (RESID) rr_v[j] = *(const u32x2*)(p.R + (int64_t)mc * p.ldr + ncl[j]);
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int n = col0 + j * 16 + ecol;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (EPI == EPI_RESIDUAL) add2_bf16x4<RESIDUAL_JOINS_BIAS_FIRST>(v, bias_v[j], rr_v[j]);      // (see above)
            else add_bf16x4(v, bias_v[j]);
            if (EPI == LTXMI_EPI_GELU_TANH) {
                // the packed form of the persistent kernel: under this epilogue every GEMM kernel produces the same bits for a
                // given row (the accumulation order over K is the same in all of them), whatever M made the dispatcher choose
                gelu_tanh_pk(v[0], v[1]);
                gelu_tanh_pk(v[2], v[3]);
            } else if (EPI == LTXMI_EPI_SILU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
            }
            if (GATED) {
                mul_sum_bf16x4(v, gt_v[j], ge_v[j]);
                add_bf16x4(v, rr_v[j]);
            }
            if (!(m_ok && n < p.N)) continue;
            u32x2 o;
            if constexpr (EPI == EPI_D2S) {
                // weight rows are packed (p1 p2 p3)-major: n = pp * C' + c'
                const int Cp = p.N >> 3;
                const int pp = n / Cp, cp = n - pp * Cp;
                const int x_ = m % p.cW, r1 = m / p.cW, y_ = r1 % p.cH, r2 = r1 / p.cH;
                const int t_ = r2 % p.cT, b_ = r2 / p.cT;
                const int to = 2 * t_ + (pp >> 2) - 1;
                if (to < 0) continue;                       // first upsampled frame is dropped
                const int yo = 2 * y_ + ((pp >> 1) & 1), xo = 2 * x_ + (pp & 1);
                if (p.res) {
                    // x_in = repeat(pixel_shuffle(x)): channel c' <- x[(c' mod (Cres/8)) * 8 + pp]
                    const uint16_t* rrow = p.res + (int64_t)m * p.res_ch + pp;
                    const int cm = p.res_ch >> 3;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += bf2f(rrow[((cp + e) % cm) * 8]);
                }
                o = pack_bf16x4(v);
                const int64_t opos = (((int64_t)b_ * (2 * p.cT - 1) + to) * (2 * p.cH) + yo) * (2 * p.cW) + xo;
                *(u32x2*)(p.C + opos * Cp + cp) = o;
            } else {
                o = pack_bf16x4(v);
                *(u32x2*)(p.C + (int64_t)m * p.ldc + n) = o;
                if (EPI == EPI_SUMSQ)
                    ss[j / 4] = sumsq4(ss[j / 4], o);
            }
        }
        if (EPI == EPI_SUMSQ) {
            static_assert(EPI != EPI_SUMSQ || NI % 4 == 0, "sum-of-squares partials are per 64 columns");
#pragma unroll
            for (int q = 0; q < NI / 4; ++q) {
                float s = ss[q];
                s += __shfl_xor(s, 16, 64);
                s += __shfl_xor(s, 32, 64);
                const int nb = col0 + q * 64;            // first column of this 64-column block
                if (ecol == 0 && m_ok && nb < p.sumsq_cols) p.sumsq[(int64_t)m * p.sumsq_ld + (nb >> 6)] = s;
            }
        }
    }
}

}  // namespace ltxmi
