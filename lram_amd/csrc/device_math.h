// Device-side scalar helpers shared by the recurrent kernels.  The formulas follow the order of
// operations of the PyTorch CPU ops the oracle uses, so that states stay within a few ulp of it.
#pragma once
#include <hip/hip_runtime.h>

namespace lram {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// torch.argmax order of (value, index) candidates: NaN is the maximum, the first index wins among equal values (NaNs
// included), +-Inf compare as ordinary values.  Starting from (-inf, INT_MAX) every element of a non-empty row is taken
// or loses to one that was, so the winner is always a real index.  (Action head: action_head.h.)
__device__ __forceinline__ bool argmax_beats(float v, int i, float best, int bi) {
  const bool v_nan = v != v, best_nan = best != best;
  if (v_nan) return !best_nan || i < bi;
  return !best_nan && (v > best || (v == best && i < bi));
}

// MinMaxTokenizer.inv_tokenize (src/tokenizers_custom/minmax_tokenizer.py:31-47) on a bin index t >= 0: float(t) * bin_width is
// rounded to fp32 BEFORE min_val is added -- two roundings, as the reference's two tensor operations.  The compiler contracts
// a * b + c into one FMA by default (and __fmul_rn / __fadd_rn are plain operators to it), which is 1 ulp off on more than half
// of the tokens wherever the bin width is no power of two; contraction is switched off for this function alone.
__device__ __forceinline__ float inv_tokenize_bin(int t, float bin_width, float tok_min) {
#pragma clang fp contract(off)
  const float scaled = (float)t * bin_width;
  return scaled + tok_min;
}
// Its inverse, MinMaxTokenizer.tokenize (minmax_tokenizer.py:14-29), of a finite x: the bin trunc((x - min) / bin_width) clamped to
// 0 .. channels - 1 -- fp32 subtract, IEEE fp32 division.
__device__ __forceinline__ int tokenize_bin(float x, float bin_width, float tok_min, int channels) {
  const float q = __fdiv_rn(__fsub_rn(x, tok_min), bin_width);
  return q <= 0.f ? 0 : (q >= (float)(channels - 1) ? channels - 1 : (int)q);
}

// torch.nn.functional.logsigmoid: min(x, 0) - log1p(exp(-|x|))
__device__ __forceinline__ float log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// torch silu: x * sigmoid(x)
__device__ __forceinline__ float silu_f(float x) { return x / (1.f + expf(-x)); }

// torch softplus (beta 1, threshold 20)
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

// The same two on the hardware transcendentals (v_exp_f32 / v_log_f32 / v_rcp_f32, 1 ulp each; results within ~3 ulp of the libm
// forms above), for kernels that evaluate them per (channel, token): the libm softplus is a 145-instruction double-float log1p and
// was 39 % of the Mamba state-update kernel's instruction stream.
__device__ __forceinline__ float silu_hw(float x) {
  return x * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
// softplus(x) = max(x, 0) + log1p(e), e = exp(-|x|); log1p(e) = log(u) * e / (u - 1) with u = fl(1 + e) cancels the rounding of
// 1 + e (for u == 1 the result is e itself); above the reference's threshold 20 the second term is below half an ulp of x
__device__ __forceinline__ float softplus_hw(float x) {
  const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(x));
  const float u = 1.f + e, d = u - 1.f;
  const float t = (__builtin_amdgcn_logf(u) * 0.69314718055994531f) * (e * __builtin_amdgcn_rcpf(d));
  return fmaxf(x, 0.f) + (d == 0.f ? e : t);
}

// exact (erf) GELU, torch.nn.functional.gelu default
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// The hold rule of the stored-context path (lram_prefill_append / lram_score_append): env b takes no token in this launch, so the
// launch writes no byte of its recurrent state and ignores its reset flag.  HOLD is a compile-time switch: the instances every
// other call launches (HOLD = false) contain nothing of it.  The flag is read through a pointer select (`other` = any readable
// address of the launch), never under a branch on `hold`: no state request of the workgroup waits for it.
template <bool HOLD>
__device__ __forceinline__ bool env_held(const uint8_t* hold, int64_t b, const void* other) {
  if (!HOLD) return false;
  const uint8_t* hp = hold != nullptr ? hold + b : reinterpret_cast<const uint8_t*>(other);
  const uint8_t hb = *hp;
  return hold != nullptr && hb != 0;
}

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float dot4(const float4& x, const float4& y) { return x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w; }

// Zeroing by a bit mask (keep = all ones or 0), not a branch or a multiply: no control flow on the flag that decides it -- the
// compiler otherwise waits for that flag before it issues anything else -- and no NaN * 0.
__device__ __forceinline__ float masked(float v, unsigned keep) { return __uint_as_float(__float_as_uint(v) & keep); }
__device__ __forceinline__ float4 masked4(const float4& v, unsigned keep) {
  return make_float4(masked(v.x, keep), masked(v.y, keep), masked(v.z, keep), masked(v.w, keep));
}

// ---- matrix-core accumulators ----
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
// row of the 32x32 MFMA accumulator held in register r by a lane of half lh
__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// Hardware hands consecutive workgroup ids to the 8 XCDs in turn (ids b, b + 8, ... share an L2): the position this id takes
// when every XCD is to own a contiguous run of a launch's nwg work items instead (grids that 8 divides; else the id itself).
__device__ __forceinline__ int xcd_contiguous_id(int bid, int nwg) {
  return (nwg & 7) == 0 ? (bid & 7) * (nwg >> 3) + (bid >> 3) : bid;
}

// ---- bf16x3: fp32-accurate products on the bf16 matrix cores (gemm_bf16x3.hip, the chunkwise cell of mlstm_chunk.hip) ----
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
// Exact 3-way bf16 split of an fp32 value, x = hi + mid + lo (8 + 8 + 8 significand bits; the residuals x - hi and
// x - hi - mid are exact in fp32).
__device__ __forceinline__ void split3(float x, __bf16& hi, __bf16& mid, __bf16& lo) {
  hi = (__bf16)x;
  const float r1 = x - (float)hi;
  mid = (__bf16)r1;
  lo = (__bf16)(r1 - (float)mid);
}
// ... of N values into three vectors V = bf16xN (a vector element does not bind to a reference)
template <typename V, int N>
__device__ __forceinline__ void split3v(const float (&x)[N], V& hi, V& mid, V& lo) {
#pragma unroll
  for (int e = 0; e < N; ++e) {
    __bf16 h, m, l;
    split3(x[e], h, m, l);
    hi[e] = h, mid[e] = m, lo[e] = l;
  }
}
// acc += a * b over one 16-deep step, a = a[0] + a[1] + a[2] (hi, mid, lo), b likewise: the six largest piece products --
// lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi, smallest terms first; the dropped mid*lo, lo*mid, lo*lo are <= 2^-24
// relative.  The order is part of the result: every caller sums in it.
__device__ __forceinline__ void bf16x3_products(f32x16& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}

// ---- row maxima for the f16x2 GEMM (gemm_f16x2.hip) ----
// power-of-two scale that puts a row whose largest magnitude is `mx` into [2^14, 2^15); 1 for an all-zero row
__device__ __forceinline__ float pow2_scale(float mx) {
  if (!(mx > 0.f)) return 1.f;
  int e = (int)((__float_as_uint(mx) >> 23) & 0xffu);  // biased exponent (0: subnormal)
  if (e == 0) e = 1;
  int se = 268 - e;                                    // biased exponent of 2^(14 - (e - 127))
  se = se > 254 ? 254 : (se < 1 ? 1 : se);
  return __uint_as_float((unsigned)se << 23);
}
// The operand format of the f16x2 GEMMs: the exact 2-way f16 split of an (already row-scaled) fp32 value, v = hi + lo up to
// the bits below lo -- hi = rn16(v), lo = rn16(v - hi); the residual v - hi is exact in fp32.
__device__ __forceinline__ void split2(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)(v - (float)hi);
}
// ... of s * v (gemm_f16x2p.hip's A operand): p points at the element in the hi plane, the lo plane is `plane` elements on.
// s is the row's power-of-two scale (pow2_scale of its largest magnitude).
__device__ __forceinline__ void split2_store4(const float4& v, float s, _Float16* p, int64_t plane) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const float xs[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
  h4 hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    _Float16 h, l;   // (a vector element does not bind to a reference)
    split2(xs[e], h, l);
    hi[e] = h, lo[e] = l;
  }
  *reinterpret_cast<h4*>(p) = hi;
  *reinterpret_cast<h4*>(p + plane) = lo;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// The wave's sum as a wave-uniform value, on the DPP cross-lane paths (no LDS crossbar round trips): quad permutes and row
// mirrors leave every lane of a 16-lane row with the row's sum, the two row broadcasts assemble the four rows in row 3, and
// lane 63 is read back into a scalar register.  Fixed summation order (deterministic).
__device__ __forceinline__ float wave_sum_bcast(float x) {
#define LRAM_DPP_ADD(ctrl) x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), ctrl, 0xf, 0xf, false))
  LRAM_DPP_ADD(0xB1);   // quad_perm [1, 0, 3, 2]
  LRAM_DPP_ADD(0x4E);   // quad_perm [2, 3, 0, 1]
  LRAM_DPP_ADD(0x141);  // row_half_mirror
  LRAM_DPP_ADD(0x140);  // row_mirror
  LRAM_DPP_ADD(0x142);  // row_bcast15: rows 1, 3 (and 2) take the sum of the row before
  LRAM_DPP_ADD(0x143);  // row_bcast31: row 3 takes rows 0 + 1
#undef LRAM_DPP_ADD
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

// The wave's maximum of NON-NEGATIVE values, in lane 63 only, on the DPP cross-lane paths (two quad permutes, two row mirrors, two
// row broadcasts) instead of six ds_bpermute round trips through the LDS crossbar: for kernels that take a maximum per (row,
// channel block) inside their inner loop.  Non-negative floats order like their bit patterns, so the maximum is taken on unsigned
// integers with 0 for lanes a step has no source for -- the form hipcc folds into one v_max_u32_dpp per step.
__device__ __forceinline__ float wave_max_nonneg_lane63(float x) {
  unsigned v = __builtin_bit_cast(unsigned, x);
#define LRAM_DPP_MAX(ctrl) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xf, 0xf, false))
  LRAM_DPP_MAX(0xB1);   // quad_perm [1, 0, 3, 2]
  LRAM_DPP_MAX(0x4E);   // quad_perm [2, 3, 0, 1]
  LRAM_DPP_MAX(0x141);  // row_half_mirror
  LRAM_DPP_MAX(0x140);  // row_mirror: every lane of a 16-lane row holds the row's maximum
  LRAM_DPP_MAX(0x142);  // row_bcast15: row r takes row r - 1's
  LRAM_DPP_MAX(0x143);  // row_bcast31: rows 2, 3 take row 1's (= rows 0, 1)
#undef LRAM_DPP_MAX
  return __builtin_bit_cast(float, v);
}

}  // namespace lram
