// gemm_mx8_epilogue.inc -- the epilogue statements of the MX-FP8 GEMM kernels, included behind their K loops: by
// gemm_mx8_kernel.inc (one operand pair) and by gemm_mx8_pair2.hip (two).  It reads p, EPI, MXOUT, RSS, GATED, RESID, the tile
// origin m0, n0, the wave's place wm, wn, WM, WN, MI, NI, the lane's frow, fh and the accumulators acc[MI][NI].
// ---- epilogue.  acc[i][j][4 g + e]: row m = m0 + wm*WM + 32 i + (l & 31), column n = n0 + wn*WN + 32 j + 8 g + 4 h + e.
// Every load is unconditional on a clamped address (gemm_tile.h says why).
const int ecol = 4 * fh;
// the outputs through buffer descriptors that end with the last element (sizes below 2^32 bytes: checked on the host)
const auto rsrc = [](void* base, int64_t bytes) { return __builtin_amdgcn_make_buffer_rsrc(base, 0, (uint32_t)bytes, 0x00020000); };
__amdgpu_buffer_rsrc_t c_rsrc = rsrc(p.C, MXOUT ? 0 : ((int64_t)(p.M - 1) * p.ldc + p.N) * 2);
__amdgpu_buffer_rsrc_t cq_rsrc = rsrc(p.Cq, MXOUT ? (int64_t)(p.M - 1) * p.ldcq + p.N : 0);
__amdgpu_buffer_rsrc_t cs_rsrc = rsrc(p.Cs, MXOUT ? (int64_t)(p.M - 1) * p.ldc_s + p.N / 32 : 0);
// RSS: the wave's 128 x 64 sub-tile is one 64-column block per row; row 32 i + frow spans acc[i][0..1][0..15] of the lanes
// l and l ^ 32
static_assert(!RSS || WN == 64, "one row-sum block per wave");
float ss[MI];
#pragma unroll
for (int i = 0; i < MI; ++i) ss[i] = 0.f;
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
            if constexpr (RSS) {
#pragma unroll
                for (int g = 0; g < 4; ++g) ss[i] = sumsq4(ss[i], pack_bf16x4(v + 4 * g));
            }
        }
    }
}
if constexpr (RSS) {
    // a block below rss_cols <= N lies inside N with all its 64 columns (rss_cols % 64 == 0); masked lanes store outside
    // the descriptor as above
    const auto& r = mx8_rss(p);
    const int nb = n0 + wn * WN;
    __amdgpu_buffer_rsrc_t ss_rsrc = rsrc(r.rss, ((int64_t)(p.M - 1) * r.rss_ld + (r.rss_cols >> 6)) * 4);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int m = m0 + wm * WM + 32 * i + frow;
        const float s = ss[i] + __shfl_xor(ss[i], 32, 64);
        const bool ok = nb < r.rss_cols && m < p.M && fh == 0;
        const uint32_t off = ok ? (uint32_t)(((int64_t)m * r.rss_ld + (nb >> 6)) * 4) : 0xfffffff0u;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(s), ss_rsrc, off, 0, 0);
    }
}
