// What the three f16x2 tile kernels share (gemm_f16x2.hip: A split while it is staged; gemm_f16x2p.hip: both operands pre-split;
// gemm_f16x2_8p.hip: 256 x 256 tiles, 8 phases): the product triple, the LDS chunk swizzle and the two epilogue forms.  The
// kernels are bit-identical by contract (tests/test_gpu_parity.py) -- the arithmetic lives here once, the schedules stay theirs.
#pragma once
#include "gemm_tile.h"   // what they share with the other GEMM kernels: gemm_tile_of, gemm_k_range

namespace lram {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// One 16-deep MFMA step of a wave's TI x 2 accumulator tiles: af / bf = [tile][plane (hi, lo)] fragments.  The order -- per
// tile lo*hi, hi*lo, hi*hi, smallest terms first -- is part of the result: every kernel sums in it.
template <int TI>
__device__ __forceinline__ void f16x2_products(f32x16 (&acc)[TI][2], const f16x8 (&af)[TI][2], const f16x8 (&bf)[2][2]) {
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][1], bf[j][0], acc[i][j], 0, 0, 0);  // lo * hi
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][0], bf[j][1], acc[i][j], 0, 0, 0);  // hi * lo
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][0], bf[j][0], acc[i][j], 0, 0, 0);  // hi * hi
    }
}

// LDS image of an operand plane tile: un-padded rows of 32 f16 = four 16-byte chunks.  A ds_read_b128 fragment read of rows
// r, r + 4, r + 8, r + 12 would hit the same banks, so the chunk at linear position c of row `row` holds logical chunk
// c ^ f16x2_chunk_swizzle(row).  An involution: whoever fills the tile (the lane's source address of the LDS-DMA, or the
// ds_write of the two-stage on-the-fly kernel) and the fragment read apply the same XOR (cdna_hip_programming.md section 5.4
// rule 21).  `row` may be the row inside any 32-row-aligned piece of the tile: only bits 2-3 count.
__device__ __forceinline__ int f16x2_chunk_swizzle(int row) { return (row >> 2) & 3; }
// f16 offset inside its LDS row of the fragment a lane (half lh = lane >> 5) reads for 16-deep step ks of a 32-deep K tile:
// the lane holds k = 16 ks + 8 lh + 0..7 of both operands, i.e. logical chunk 2 ks + lh.  sw = f16x2_chunk_swizzle of the
// lane's row, taken ONCE ahead of the K loop by the caller (with the row itself as the argument, the swizzle was re-derived
// inside the two-stage loop of gemm_f16x2.hip: three to four more instructions per K tile).
__device__ __forceinline__ int f16x2_frag_offset(int ks, int lh, int sw) { return ((2 * ks + lh) ^ sw) << 3; }

// Accumulator-order store of one 32 x 32 tile (C/D layout of the MFMA: a lane holds column `col` (< g.n: the caller drops the
// others) of rows row0 + (r & 3) + 8 * (r >> 2), r = 0..15, row0 including its 4 * (lane >> 5)).  Per element
// acc * (wi * ainv[r]) + bias, + residual, silu from column g.act_silu_from on; S != nullptr: the raw un-scaled sums into
// this split's slab [M][N] instead (bias / residual are applied by the reduce).
// (per tile one base pointer; the 16 rows are compile-time multiples of the row pitch from it -- the per-element 64-bit
// row * pitch products, bounds checks and libm SiLU of the first form were ~60 instructions per stored value, as many in the
// epilogue as in the whole K loop)
// A MACRO, expanded inside the kernel template (it names the kernel's g, S, HAS_BIAS, HAS_RES): as a __forceinline__ function
// template -- arguments by value, by reference or as scalars alike -- hipcc kept the 16 row predicates and row offsets of a
// tile row live in scalar registers across the calls: every instance of gemm_f16x2p.hip and gemm_f16x2_8p.hip went to 106
// SGPRs with spills into VGPR lanes (200-300 v_readlane per kernel) and one more VGPR.  ACC: the tile's f32x16; AINV: float[16].
#define LRAM_F16X2_STORE_ACC_TILE(ACC, AINV, WI, ROW0, COL)                                               \
  {                                                                                                       \
    const int row0_ = (ROW0), col_ = (COL);                                                               \
    const float wi_ = (WI);                                                                               \
    const float bv_ = HAS_BIAS ? g.bias[col_] : 0.f;                                                      \
    const bool act_ = g.act_silu_from >= 0 && col_ >= g.act_silu_from;                                    \
    const bool rows_in_ = row0_ + 27 < g.m; /* (uniform but for tiles on the lower edge) */               \
    if (S != nullptr) {                                                                                   \
      float* sp_ = S + (int64_t)row0_ * g.n + col_;                                                       \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                 \
        const int ro_ = (r_ & 3) + 8 * (r_ >> 2);                                                         \
        if (rows_in_ || row0_ + ro_ < g.m) sp_[(int64_t)ro_ * g.n] = (ACC)[r_] * (wi_ * (AINV)[r_]);      \
      }                                                                                                   \
    } else {                                                                                              \
      float* cp_ = g.c + (int64_t)row0_ * g.ldc + col_;                                                   \
      const float* rp_ = HAS_RES ? g.residual + (int64_t)row0_ * g.ldc + col_ : nullptr;                  \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                 \
        const int ro_ = (r_ & 3) + 8 * (r_ >> 2);                                                         \
        if (rows_in_ || row0_ + ro_ < g.m) {                                                              \
          float v_ = (ACC)[r_] * (wi_ * (AINV)[r_]) + bv_;                                                \
          if (HAS_RES) v_ += rp_[(int64_t)ro_ * g.ldc];                                                   \
          if (act_) v_ = silu_hw(v_);                                                                     \
          cp_[(int64_t)ro_ * g.ldc] = v_;                                                                 \
        }                                                                                                 \
      }                                                                                                   \
    }                                                                                                     \
  }

// The float4 step of the LDS-turned epilogue (the staging loops around it differ per kernel and stay there): t = four
// consecutive columns gcol.. of row grow as the accumulators left them, un-scaled, + bias, + residual, silu, one dwordx4
// store to outp (row pitch ld_out: C, or with `slab` the split's slab, which takes neither residual nor activation --
// the caller passes bv4 = 0 and act_from = -1 then, as it does bv4 = 0 without a bias: the sum is written as before, so
// this piece has no HAS_BIAS).  Same arithmetic per element as f16x2_store_acc_tile.
template <bool HAS_RES>
__device__ __forceinline__ void f16x2_finish4(const GemmArgs& g, float* outp, int64_t ld_out, bool slab, int act_from, const float4 t,
                                              const float4 wi4, float ai, const float4 bv4, int grow, int gcol) {
  float4 v;
  v.x = t.x * (wi4.x * ai) + bv4.x, v.y = t.y * (wi4.y * ai) + bv4.y;
  v.z = t.z * (wi4.z * ai) + bv4.z, v.w = t.w * (wi4.w * ai) + bv4.w;
  if (HAS_RES && !slab) {
    const float4 rr = *reinterpret_cast<const float4*>(g.residual + (int64_t)grow * g.ldc + gcol);
    v.x += rr.x, v.y += rr.y, v.z += rr.z, v.w += rr.w;
  }
  if (act_from >= 0) {
    if (gcol + 0 >= act_from) v.x = silu_hw(v.x);
    if (gcol + 1 >= act_from) v.y = silu_hw(v.y);
    if (gcol + 2 >= act_from) v.z = silu_hw(v.z);
    if (gcol + 3 >= act_from) v.w = silu_hw(v.w);
  }
  *reinterpret_cast<float4*>(outp + (int64_t)grow * ld_out + gcol) = v;
}

}  // namespace lram
