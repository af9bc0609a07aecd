// conv.h -- what the convolution's files share: the plan of a call (conv_plan.hip makes it, gemm.hip and conv_direct.hip launch
// it), the direct kernels' parameter block, their two geometries, and the parts of the (chunk, tap) stream that the eight-wave
// and the four-wave kernel share with their generated code unchanged (what had to stay written out, and why).
#pragma once
#include "common.h"

namespace ltxmi {

// ltxmi_conv3d_ndhwc_bf16 (conv_plan.hip): how one call runs, worked out once from its arguments by conv3d_plan; the launch acts
// on it and ltxmi_conv3d_workspace_bytes / ltxmi_conv3d_fuses_post_norm return its fields.  CONV_REFUSED: algo asks for the
// direct convolution, which does not take the shape.
enum ConvRoute : int { CONV_GEMM128, CONV_GEMM256, CONV_DIRECT8, CONV_DIRECT4, CONV_REFUSED };
struct ConvPlan {
    int kt, sT, sHW, tpad;              // kernel frames, time / space strides, frames of padding in front
    int oT, oH, oW; int64_t M;          // output grid, M = B oT oH oW positions
    ConvRoute route;                    // the implicit GEMM (gemm.hip) with 128- / 256-wide tiles, the eight- / four-wave direct form
    int epi;                            // 0 plain, 1 + add, 2 depth-to-space; four-wave form also 3 .. 5 = the same + post_norm,
                                        // 6 = fp32 partial sums of a channel split (the finalising pass applies the epilogue)
    int swap, ksplit, tiles_t, tiles_8, tiles_16, tiles_n;    // direct forms: see conv3d_plan
    int64_t grid, split_bytes;          // workgroups of ONE channel range; workspace the split needs (0: no split pays)
    bool fuses_post_norm;               // post_norm = 1 would be applied in the epilogue
};
int conv3d_gemm_tile(int64_t M, int Cout);     // gemm.hip: the implicit GEMM's tile (128 or 256) for M positions x Cout
int launch_conv3d_gemm(const ltxmi_conv3d_args* a, const ConvPlan& pl, hipStream_t stream);       // gemm.hip
int launch_conv3d_direct(const ltxmi_conv3d_args* a, const ConvPlan& pl, hipStream_t stream);     // conv_direct.hip

// ltxmi_conv3d_args.pad_replicate: the spatial padding mode (nn.Conv3d padding_mode with padding 1)
enum ConvPad : int { CONV_PAD_ZEROS = 0, CONV_PAD_REPLICATE = 1, CONV_PAD_REFLECT = 2 };

// Where coordinate i of an axis of extent L (H or W; each on its own, so a corner mirrors on both) is read from: the source
// index, always in [0, L - 1], and whether the element is zero padding instead.  Only i = -1 and i = L are padding (reflect:
// -1 reads 1 and L reads L - 2, the edge is not repeated; the entry check refuses L < 2); tiles and M-rows overhang the image
// further, into positions whose outputs are never stored, and there a mirror 2 L - 2 - i would leave the buffer (L = 2, i = 9:
// -7): every i beyond L reads what i = L reads, whatever the mode.
// The mirror is the clamp moved one step back inside: + 1 in the lanes below 0, - 1 in the lanes from L on.  Written as an add
// with carry and a subtract with borrow whose carry-in is the lane mask of the compare, it works on the clamped value in place.
// The implicit GEMM's gather (gemm.hip, in the K loop of a kernel that lives at 256 registers) has none to spare: as selects or
// as arithmetic on i (2 clamp(i) - i) every C++ form of it cost the 256-wide instances one to seven more spilled registers.
struct ConvSrc { int i; bool zero; };
__device__ __forceinline__ ConvSrc conv_pad_src(int i, int L, int mode) {
    const bool lo = i < 0, hi = i >= L, mirror = mode == CONV_PAD_REFLECT && L > 1;
    int s = lo ? 0 : (hi ? L - 1 : i);
    const uint64_t up = __builtin_amdgcn_ballot_w64(lo && mirror), down = __builtin_amdgcn_ballot_w64(hi && mirror);
    uint64_t carry_out;                                              // (never read)
    asm("v_addc_co_u32_e64 %0, %1, %0, 0, %2" : "+v"(s), "=s"(carry_out) : "s"(up));
    asm("v_subb_co_u32_e64 %0, %1, %0, 0, %2" : "+v"(s), "=s"(carry_out) : "s"(down));
    return ConvSrc{s, (lo | hi) && mode == CONV_PAD_ZEROS};
}

// the direct forms' output tile: 2 (t) x 8 x 16 positions x 128 output channels
constexpr int CONV_TT = 2, CONV_TY = 8, CONV_TX = 16;

struct ConvDirectP {
    const uint16_t* x; const uint16_t* w; const uint16_t* bias; uint16_t* y; const uint16_t* add;
    const uint16_t* res; int res_ch;            // depth-to-space residual (x itself) or NULL
    int B, T, H, W, Cin, Cout;
    int tpad, pad_replicate, tzero;
    int tiles_t, tiles_y, tiles_x, tiles_n;
    const float* post_scale; const float* post_shift; float post_eps;      // EPI >= 3 only
    uint16_t* y2;                                                          // EPI 4 / 5: the activated second output
    // four-wave form only.  swap_hw: the tile's 16-position rows run along H and its 8 rows along W (W = 24 is 1.5 tiles of 16,
    // H = 16 exactly one: 21 tiles instead of 28 at the 1024-channel stage).  ksplit > 1: the input channels are cut into ksplit
    // ranges, one workgroup each (grid x ksplit), whose fp32 partial sums go to `part` [ksplit][B T H W][Cout] (EPI 6, no bias);
    // conv_split_finalize_kernel adds them up and applies the epilogue
    int swap_hw, ksplit; float* part;
};

// ---- the two geometries (conv_direct.hip describes them): the LDS image of a tile -- halo rows in 1-KB pieces, three weight
// stages, row table, control table -- and the piece numbers that bound the three windows in which the halo streams
template <int WAVES_, int ROW_B_, int PLANE_STRIDE_>
struct ConvGeo {
    static constexpr int WAVES = WAVES_, ROW_B = ROW_B_, CHUNK = ROW_B / 2, PLANE_STRIDE = PLANE_STRIDE_, PIECE_ROWS = 1024 / ROW_B;
    static constexpr int HT = CONV_TT + 2, HY = CONV_TY + 2, HX = CONV_TX + 2, PLANE_ROWS = HY * HX, WSTAGES = 3;
    static constexpr int HALO_ROWS = HT * PLANE_STRIDE, HALO_BYTES = HALO_ROWS * ROW_B, W_BYTES = 128 * ROW_B;
    static constexpr int ROWTAB_OFF = HALO_BYTES + WSTAGES * W_BYTES, CTLTAB_OFF = ROWTAB_OFF + HALO_ROWS * 4;
    static constexpr int SMEM = CTLTAB_OFF + WAVES * 27 * 8, Q_END = HALO_ROWS / PIECE_ROWS;
};
// eight waves, 64-channel chunks: 720 rows x 128 B (pieces end rows 0 .. 175 | .. 359 | .. 719)
struct ConvGeo8 : ConvGeo<8, 128, 180> {
    static constexpr bool KSPLIT = false;
    static constexpr int Q_PLANE0 = 22, Q_PLANE1 = 45;
};
// four waves, 32-channel chunks: planes padded to 192 rows (whole 16-row pieces) x 64 B; also the split over the input channels
struct ConvGeo4 : ConvGeo<4, 64, 192> {
    static constexpr bool KSPLIT = true;
    static constexpr int Q_PLANE0 = PLANE_STRIDE / 16, Q_PLANE1 = 2 * Q_PLANE0;      // 12, 24 (of 48)
    __device__ static __forceinline__ int swz(int c, int r) { return c ^ (((r >> 2) & 1) << 1); }    // slot of source chunk c in LDS row r
};

// ---- tile: blockIdx.x -> (n block fastest, then x, y, t, b [, channel range]): the n blocks of a position tile are neighbours
struct ConvTile { int b, ks, t0, y0, x0, n0; };    // y0: the tile's 8-row direction, x0: its 16-position one
template <class G>
__device__ __forceinline__ ConvTile conv_tile(int id, int tiles_n, int tiles_x, int tiles_y, int tiles_t, int B) {
    ConvTile t;
    const int nb = id % tiles_n; id /= tiles_n;
    const int tx = id % tiles_x; id /= tiles_x;
    const int ty = id % tiles_y; id /= tiles_y;
    const int tt = id % tiles_t; id /= tiles_t;
    t.b = G::KSPLIT ? id % B : id;
    t.ks = G::KSPLIT ? id / B : 0;                      // channel range of this workgroup (0 unless ksplit > 1)
    t.t0 = tt * CONV_TT; t.y0 = ty * CONV_TY; t.x0 = tx * CONV_TX; t.n0 = nb * 128;
    return t;
}

// ---- control table: what a tap of the (chunk, tap) stream does besides its MFMAs -- all wave-uniform, all a function of (tap,
// chunk).  Scalar instructions are NOT free beside MFMAs here: both waves of a SIMD pair run the same code at the same time, and a
// wave that issues a scalar instruction issues no MFMA (tools/ubench/conv_loop.hip: a bare loop of the eight-wave tap's 2 x 32
// MFMAs runs at 1032 cycles per tap; with the fragment reads, their address arithmetic and the barrier 1196; with ~140 dependent
// scalar instructions behind block 2 it takes 1780).  So the control of the 27 taps is worked out ONCE per tile into a table
// in LDS (two packed words per (wave, tap)); a tap reads the entry of the tap after the next with one hidden ds_read_b64 at
// its end, and the tap in between unpacks it behind an MFMA block: ~20 scalar instructions per tap instead of the ~85
// that recomputing it from (tap, chunk) took (measured on the way: recomputed at the top of the tap -5 %, behind block 2
// +2.0..2.7 % over round 2's kernel, behind block 0 / 1 / 3 -3.5 / -2.2 / -2.0 %: profiles/r03_conv_stream.log).
struct ConvCtl {
    int w_soff, w_stage;     // weights two taps ahead in the stream: scalar byte offset (< 0: nothing to issue), stage
    int h_q, h_soff;         // this tap's halo piece (-1: none) and its chunk's byte offset
    int n_off, n_stage;      // next tap: halo row offset of its (dt, dy, dx), weight stage
    int n_q;                 // next tap's piece slot in the row table (clamped; whether there is a piece: its own h_q)
};
// word 0: byte offset of tap + 2's weights inside a weight row, relative to its chunk; bit 31: that tap belongs to the NEXT chunk
// word 1: n_off [0,9) | w_stage [9,11) | n_stage [11,13) | halo piece [13,21) (0xff: none) | piece of the chunk itself [21] | n_q [22,29)
// the entry (d0, d1) at stream position (tap, chunk at channel c0) of a channel range that ends at c_end
template <class G>
__device__ __forceinline__ ConvCtl conv_unpack_ctl(uint32_t d0, uint32_t d1, int c0, int c_end) {
    ConvCtl k;
    const int c_next = c0 + G::CHUNK < c_end ? c0 + G::CHUNK : -1;
    const int c2 = (int)d0 < 0 ? c_next : c0;
    k.w_soff = c2 >= 0 ? (int)(d0 & 0x7fffffffu) + c2 * 2 : -1;
    k.n_off = (int)(d1 & 0x1ffu);
    k.w_stage = (int)((d1 >> 9) & 3u);
    k.n_stage = (int)((d1 >> 11) & 3u);
    const int hq = (int)((d1 >> 13) & 0xffu);
    const int c = ((d1 >> 21) & 1u) ? c0 : c_next;
    k.h_q = ((hq != 0xff) & (c >= 0)) ? hq : -1;
    k.h_soff = c * 2;
    k.n_q = (int)((d1 >> 22) & 0x7fu);
    return k;
}
// The two hidden reads at a tap's end: the control entry of the tap after the next and the row-table entry of the next tap's
// piece.  Issued from inline asm and waited for by hand: as a C++ load hipcc put s_waitcnt lgkmcnt(0) in front of it (at the end
// of every tap, behind the fragment reads just issued).  An LDS read hipcc does not know about only makes its own counted waits
// more conservative: LDS operations complete in order.
__device__ __forceinline__ void conv_read_ctl(u32x2& cw_nx, uint32_t ctltab_lds, int tap) {      // ctltab_lds: this wave's 27 entries
    const uint32_t a = ctltab_lds + (uint32_t)(tap * 8);
    asm volatile("ds_read_b64 %0, %1" : "=v"(cw_nx) : "v"(a) : "memory");
}
template <class G>
__device__ __forceinline__ void conv_read_hoff(uint32_t& hoff_nx, uint32_t rowtab_lds, int q) {  // rowtab_lds: + this lane's row of a piece
    const uint32_t a = rowtab_lds + (uint32_t)(q * (G::PIECE_ROWS * 4));
    asm volatile("ds_read_b32 %0, %1" : "=v"(hoff_nx) : "v"(a) : "memory");
}

}  // namespace ltxmi
