// What the GEMM kernels share, device side only: which operands batch z addresses, which tile a workgroup id maps to, which K
// tiles a split walks, and the accumulator-order store of a wave's tiles without row scales (gemm_f32.hip: the fp32 tile
// kernel, the GEMV and the few-row kernel; gemm_bf16x3.hip).  The f16x2 kernels take the tile map and the K range from here
// (gemm_f16x2_tile.h holds what only they share); the bf16x3 arithmetic itself is in device_math.h, beside the chunkwise
// mLSTM cell that sums in the same order.  The launch policy (split-K, XCD split, the reduce) is host code in gemm_f32.hip.
//
// Functions where the compiler gives the kernels the code they had, macros where it does not (each says what moved): the
// kernels are compared instruction for instruction with scripts/gemm_isa_compare.py (profiles/gemm_rest_isa.txt).
#pragma once
#include "common.h"
#include "device_math.h"

namespace lram {

// Two-level batching (GemmArgs): z = z1 * nb2 + z2, pointer = base + z1 * s?1 + z2 * s?2.  Declares the kernel's A, WNAME, C,
// R and bias for batch Z of its GemmArgs g.  Table form (TAB true: the launch carries operand tables): z2 picks unrelated
// base pointers from g.a_tab / WTAB / g.c_tab instead of a stride -- several projections as ONE launch (the four sLSTM gates);
// bias and residual have no tables.  WBASE / WTAB: the kernel's own W operand as const TW* (fp32 rows; bf16 planes, whose
// table holds them as uint16_t).  HB / HR: the launch has a bias / a residual (template arguments, or tested at run time).
// A MACRO: a function that takes TAB and WBASE as arguments reads them from the kernel arguments ahead of the z1 / z2
// division, and the compiler schedules the prologue around that order -- the few-row kernel <4, 16> went from 170 to 172 VGPRs
// with other compares in its K loop, and every bf16x3 instance moved.
#define LRAM_GEMM_BATCH_OPERANDS_TAB(Z, HB, HR, TW, WNAME, WBASE, TAB, WTAB)                                         \
  const int z = (Z);                                                                                                 \
  const int z1 = z / g.nb2, z2 = z - z1 * g.nb2;                                                                     \
  const bool tab = (TAB);                                                                                            \
  const float* A = tab ? g.a_tab[z2] + z1 * g.sA1 : g.a + z1 * g.sA1 + z2 * g.sA2;                                   \
  const TW* WNAME = tab ? reinterpret_cast<const TW*>((WTAB)[z2]) + z1 * g.sW1 : (WBASE) + z1 * g.sW1 + z2 * g.sW2;  \
  float* C = tab ? g.c_tab[z2] + z1 * g.sC1 : g.c + z1 * g.sC1 + z2 * g.sC2;                                         \
  const float* R = (HR) ? g.residual + z1 * g.sC1 + z2 * g.sC2 : nullptr;                                            \
  const float* bias = (HB) ? g.bias + z1 * g.sBias1 + z2 * g.sBias2 : nullptr;
// Plain form: fp32 W rows, strides only.
#define LRAM_GEMM_BATCH_OPERANDS(Z, HB, HR) LRAM_GEMM_BATCH_OPERANDS_TAB(Z, HB, HR, float, W, g.w, false, g.w_tab)

// One-dimensional XCD-aware tile order: row-major over the grid of nwg tiles, tiles_n per row, each XCD a contiguous run of it
// (xcd_contiguous_id, device_math.h), so that neighbouring N tiles of one M tile (same A rows) hit the same L2.
// (nwg is an argument: with tiles_m in its place and the product taken here, the callers' prologues came out reordered)
__device__ __forceinline__ void gemm_tile_1d(int bid, int nwg, int tiles_n, int& tm, int& tn) {
  bid = xcd_contiguous_id(bid, nwg);
  tm = bid / tiles_n;
  tn = bid - tm * tiles_n;
}
// The tile a workgroup id maps to under the launcher's split (gemm_choose_xcd_split: the f16x2 kernels.  The launchers of the
// fp32 / bf16x3 kernels never choose one; those kernels call gemm_tile_1d themselves -- two scalar branches less).
__device__ __forceinline__ void gemm_tile_of(const GemmArgs& g, int bid, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int nwg = tiles_m * tiles_n;
  if (g.panel_w > 0) {
    const int x = bid & 7, q = nwg >> 3, r = nwg & 7;
    const int pos = x * q + min(x, r) + (bid >> 3);           // XCD x owns walk positions [x q + min(x, r), ...)
    const int per_panel = tiles_m * g.panel_w;
    const int p = pos / per_panel, rem = pos - p * per_panel;
    const int w = min(g.panel_w, tiles_n - p * g.panel_w);
    const int row = rem / w;
    tm = (p & 1) ? tiles_m - 1 - row : row;
    tn = p * g.panel_w + rem - row * w;
    return;
  }
  if (g.xcd_gm > 0) {
    const int x = bid & 7, idx = bid >> 3;                    // XCD, position in that XCD's stream of workgroups
    const int bm_t = tiles_m / g.xcd_gm, bn_t = tiles_n / g.xcd_gn;   // tiles per band
    const int xm = x / g.xcd_gn, xn = x - xm * g.xcd_gn;
    tm = xm * bm_t + idx / bn_t;                              // M outer, N inner: the band's N tiles of one M tile run together
    tn = xn * bn_t + idx % bn_t;
    return;
  }
  gemm_tile_1d(bid, nwg, tiles_n, tm, tn);
}

// K tiles [kt0, nk) of this workgroup out of the launch's nk_all: all of them, or with split-K the share of split blockIdx.z
// (the last split may be short, or empty for the kernels whose nk_all rounds K down).
__device__ __forceinline__ void gemm_k_range(const GemmArgs& g, int nk_all, int& kt0, int& nk) {
  kt0 = g.split_k > 1 ? blockIdx.z * g.k_tiles_per_split : 0;
  nk = g.split_k > 1 ? min(nk_all, kt0 + g.k_tiles_per_split) : nk_all;
}

// Accumulator-order store of a wave's TI x 2 tiles of 32 x 32 (C/D layout of the MFMA: a lane holds column lane & 31 of the
// rows acc_row(r, lane >> 5), r = 0..15), no row scales: with split-K the raw partial sums into this split's slab [M][N] (bias
// and residual are applied by the reduce) and the kernel returns; else acc + bias, + residual, with ACT silu from column
// g.act_silu_from on, into C.  WM = rows per wave.
// A MACRO, expanded at the end of the kernel template (it names the kernel's g, acc, C, R, bias, HAS_BIAS, HAS_RES, m0, n0,
// wm, wn, li, lh): gemm_f16x2_tile.h records what this construct cost the f16x2p kernels as a function template.  The row is
// acc_row(r, lh) SPELLED OUT, summed left to right with the tile's base: with the call in its place the same sum associates
// otherwise and every bf16x3 instance got another epilogue (five of eleven other SGPR counts).
#define LRAM_GEMM_STORE_ACC_TILES(TI, WM, ACT)                                                \
  if (g.split_k > 1) {                                                                        \
    float* S_ = g.splitk_ws + (int64_t)blockIdx.z * g.m * g.n;                                \
    _Pragma("unroll") for (int i = 0; i < (TI); ++i)                                          \
      _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                         \
        const int col = n0 + 64 * wn + 32 * j + li;                                           \
        if (col >= g.n) continue;                                                             \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                      \
          const int row = m0 + (WM) * wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;          \
          if (row < g.m) S_[(int64_t)row * g.n + col] = acc[i][j][r];                         \
        }                                                                                     \
      }                                                                                       \
    return;                                                                                   \
  }                                                                                           \
  _Pragma("unroll") for (int i = 0; i < (TI); ++i)                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                           \
      const int col = n0 + 64 * wn + 32 * j + li;                                             \
      if (col >= g.n) continue;                                                               \
      const float bv = HAS_BIAS ? bias[col] : 0.f;                                            \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                        \
        const int row = m0 + (WM) * wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;            \
        if (row < g.m) {                                                                      \
          float v = acc[i][j][r] + bv;                                                        \
          if (HAS_RES) v += R[(int64_t)row * g.ldc + col];                                    \
          if ((ACT) && g.act_silu_from >= 0 && col >= g.act_silu_from) v = silu_hw(v);        \
          C[(int64_t)row * g.ldc + col] = v;                                                  \
        }                                                                                     \
      }                                                                                       \
    }

}  // namespace lram
