// Action head, sampling mode: one token per (env, action dim) drawn from the head's logits on the device.
//
// Reference function replaced: sample_from_logits(logits, temperature, top_k, top_p)
// (src/algos/models/model_utils.py:7-32), applied row by row as DiscreteDecisionMamba.get_action_pred does
// (src/algos/decision_mamba.py:118-120; the xLSTM agent hands it the [act_dim, n_vocab] block,
// src/algos/discrete_decision_transformer_sb3.py:63-64).  Per row of n logits:
//   1. top_p > 0: q = torch.quantile(row, top_p) in float64 (order statistics floor / ceil(top_p * (n - 1)), ATen's lerp);
//      unless q equals the row maximum, every logit <= q is dropped.  A quantile of the logit VALUES, not nucleus sampling.
//   2. top_k > 0: only the k largest of what is left stay; ties at the k-th place: lowest index first.
//   3. weights exp(temperature * (logit - max)): the reference MULTIPLIES by `temperature`, and so does this.
//   4. token = first kept index, in vocabulary order, whose cumulative probability exceeds the uniform u in [0, 1);
//      u is word 0 of Philox4x32-10 with key (seed lo, seed hi) and counter (slot lo, action dim, draw lo, draw hi).
// A row that holds a NaN, whose maximum is +-inf, or of which nothing is left, takes the argmax rule (argmax_beats);
// the reference raises there.  Arithmetic: fp64 from the quantile on (a row is 5 values per lane; the selection is a
// bitwise binary search on the order-preserving integer image of the floats, 32 rounds of PER compares + ballot per
// order statistic, linear in n).
#include "common.h"
#include "device_math.h"

namespace lram {
namespace {

__device__ __forceinline__ uint32_t order_key(float v) {  // a < b  <=>  order_key(a) < order_key(b)   (no NaN, -0 canonicalised)
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): word 0 of the block, as a double in [0, 1)
__device__ __forceinline__ double philox_uniform(uint64_t seed, uint64_t slot, uint32_t dim, uint64_t draw) {
  uint32_t c0 = (uint32_t)slot, c1 = dim, c2 = (uint32_t)draw, c3 = (uint32_t)(draw >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return (double)c0 * 2.3283064365386963e-10;  // 2^-32
}

template <int PER>
__device__ __forceinline__ int wave_count_lt(const uint32_t (&key)[PER], uint32_t x) {
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) cnt += __popcll(__ballot(key[j] < x));
  return cnt;
}

// The r-th smallest (0-based) of the wave's 64 * PER keys: the largest x with |{key < x}| <= r, built bit by bit.
template <int PER>
__device__ __forceinline__ uint32_t wave_select(const uint32_t (&key)[PER], int r) {
  uint32_t res = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = res | (1u << bit);
    if (wave_count_lt<PER>(key, cand) <= r) res = cand;
  }
  return res;
}

// One wave, one row, staged in LDS (`row`, n floats); lane l holds the PER consecutive entries from l * PER on, so that
// vocabulary order is (lane, j) order.  Returns the token (wave-uniform).
template <int PER>
__device__ __forceinline__ int sample_row(const float* row, int n, double temperature, int top_k, double top_p, double u,
                                          int lane) {
  float v[PER];
  uint32_t key[PER];
  bool nan_here = false;
  float vmax = -INFINITY;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = lane * PER + j;
    v[j] = i < n ? row[i] + 0.f : -INFINITY;  // (-0 -> +0: one key per value)
    nan_here |= v[j] != v[j];
    vmax = fmaxf(vmax, v[j]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
  bool plain = __any(nan_here) || vmax == INFINITY || vmax == -INFINITY;
  int token = 0x7fffffff;
  if (!plain) {
    uint32_t keep = 0;  // bit j: entry j of this lane is in the support
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const bool valid = lane * PER + j < n;
      key[j] = valid ? order_key(v[j]) : 0xffffffffu;  // padding sorts last
      keep |= (valid ? 1u : 0u) << j;
    }
    if (top_p > 0.0) {
      const double rank = top_p * (double)(n - 1);
      const int lo = (int)floor(rank), hi = (int)ceil(rank);
      const double wgt = rank - (double)lo;
      const uint32_t klo = wave_select<PER>(key, lo);
      uint32_t khi = klo;
      if (hi > lo && wave_count_lt<PER>(key, klo + 1u) <= hi) {  // order statistic `hi` is the next larger value
        uint32_t mn = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < PER; ++j) mn = key[j] > klo ? min(mn, key[j]) : mn;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, off, 64));
        khi = mn;
      }
      const double a = (double)key_value(klo), b = (double)key_value(khi);
      const double q = wgt < 0.5 ? a + wgt * (b - a) : b - (b - a) * (1.0 - wgt);  // at::lerp
      if (q != (double)vmax) {
#pragma unroll
        for (int j = 0; j < PER; ++j)
          if (!((double)v[j] > q)) keep &= ~(1u << j);
      }
    }
    if (top_k > 0) {
      int kept = 0;
#pragma unroll
      for (int j = 0; j < PER; ++j) kept += __popcll(__ballot((keep >> j) & 1u));
      if (kept > top_k) {
#pragma unroll
        for (int j = 0; j < PER; ++j) key[j] = ((keep >> j) & 1u) ? key[j] : 0u;  // dropped entries and padding sort first
        const uint32_t kth = wave_select<PER>(key, 64 * PER - top_k);           // the k-th largest: a kept key, as kept > k
        const int above = 64 * PER - wave_count_lt<PER>(key, kth + 1u);           // (kth < 0xffffffff: no NaN in the row)
        const int room = top_k - above;                                           // ties at the k-th place that stay
        int ties = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) ties += key[j] == kth ? 1 : 0;
        int before = ties;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int t = __shfl_up(before, off, 64);
          if (lane >= off) before += t;
        }
        before -= ties;  // ties on lower lanes = at lower indices
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          if (key[j] == kth) {
            if (before >= room) keep &= ~(1u << j);
            ++before;
          } else if (key[j] < kth) {
            keep &= ~(1u << j);
          }
        }
      }
    }
    double w[PER], loc = 0.0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      w[j] = ((keep >> j) & 1u) ? exp(temperature * ((double)v[j] - (double)vmax)) : 0.0;
      loc += w[j];
    }
    double inc = loc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double t = __shfl_up(inc, off, 64);
      if (lane >= off) inc += t;
    }
    const double total = __shfl(inc, 63, 64);
    if (total > 0.0 && total < (double)INFINITY) {
      const double target = u * total;
      double run = __shfl_up(inc, 1, 64);
      if (lane == 0) run = 0.0;
      int first = 0x7fffffff, last = -1;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        run += w[j];
        if (w[j] > 0.0) {
          last = lane * PER + j;
          if (first == 0x7fffffff && run > target) first = last;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
      if (first == 0x7fffffff) {  // rounding at the top end of the CDF: the last token of the support
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) last = max(last, __shfl_xor(last, off, 64));
        first = last;
      }
      token = first;
    } else {
      plain = true;  // nothing left (a quantile that is NaN): the argmax rule
    }
  }
  if (plain) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
      const float x = row[i];
      if (argmax_beats(x, i, best, bi)) best = x, bi = i;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (argmax_beats(ov, oi, best, bi)) best = ov, bi = oi;
    }
    token = bi;
  }
  return token;
}

// A wave's row: global -> its LDS strip, coalesced.  Every wave of the workgroup reaches the barrier behind it.
template <int PER>
__device__ __forceinline__ void stage_row(float* strip, const float* src, int n, int lane, bool active) {
  if (active) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = lane + 64 * j;
      if (i < n) strip[i] = src[i];
    }
  }
  __syncthreads();
}

// The sampling counterpart of action_argmax_kernel (misc_kernels.hip), same grid: one wave per (env, action dim), four
// per workgroup.  sp.draw is read, never written, here: sample_advance_kernel bumps it once per env-step behind every head
// launch of that step.
template <int PER>
__global__ __launch_bounds__(256) void action_sample_kernel(const float* logits, float* actions, int32_t* tokens, int B,
                                                            int act_dim, int n_vocab, int n_discrete, int action_channels,
                                                            float tok_min, float tok_max, int discrete, int col_begin,
                                                            int col_end, SampleArgs sp, const uint8_t* slot_flags,
                                                            const uint8_t* slot_act) {
  __shared__ float stage[4][64 * PER];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int item = blockIdx.x * 4 + wv;
  const int ndim = (discrete && slot_flags == nullptr) ? 1 : act_dim;
  const int b = item / ndim, j = item - b * ndim;
  bool active = item < B * ndim && j >= col_begin && j < col_end;
  bool fill = false;
  if (active && slot_flags != nullptr) {  // slot table: head mode and dims in use of the wave's env slot (wave-uniform)
    discrete = slot_flags[b] & 1;
    fill = j >= (int)slot_act[b];
    active = !fill;
  }
  const int n = discrete ? n_discrete : n_vocab;
  stage_row<PER>(stage[wv], logits + (int64_t)b * act_dim * n_vocab + (int64_t)j * n_vocab, n, lane, active);
  if (fill && lane == 0) {  // a column the slot does not use: the fill values, on every call
    if (tokens != nullptr) tokens[(int64_t)b * act_dim + j] = -1;
    actions[(int64_t)b * act_dim + j] = 0.f;
  }
  if (!active) return;
  const double u = philox_uniform(sp.seed, sp.slot0 + (uint64_t)b, (uint32_t)j, *sp.draw);
  const int tok = sample_row<PER>(stage[wv], n, sp.temperature, sp.top_k, sp.top_p, u, lane);
  if (lane == 0) {
    if (tokens != nullptr) tokens[(int64_t)b * act_dim + j] = tok;
    float out;
    if (discrete) {
      out = (float)tok;
    } else {  // inv_tokenize, as action_argmax_kernel
      int t = tok - n_discrete;
      t = t < 0 ? 0 : t;
      const float bin_width = (tok_max - tok_min) / (float)action_channels;
      out = (float)t * bin_width + tok_min;
    }
    actions[(int64_t)b * act_dim + j] = out;
  }
}

__global__ void sample_advance_kernel(uint64_t* draw) {
  if (threadIdx.x == 0 && blockIdx.x == 0) draw[0] = draw[0] + 1;
}

// Test / evidence entry: the same row code on caller logits (row r at logits + r * ld) and caller uniforms.
template <int PER>
__global__ __launch_bounds__(256) void sample_tokens_kernel(const float* logits, int64_t rows, int n, int64_t ld,
                                                            double temperature, int top_k, double top_p,
                                                            const double* uniform, int32_t* tokens) {
  __shared__ float stage[4][64 * PER];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wv;
  const bool active = r < rows;
  stage_row<PER>(stage[wv], logits + (active ? r : 0) * ld, n, lane, active);
  if (!active) return;
  const int tok = sample_row<PER>(stage[wv], n, temperature, top_k, top_p, uniform[r], lane);
  if (lane == 0) tokens[r] = tok;
}

__global__ __launch_bounds__(256) void sample_uniforms_kernel(uint64_t seed, uint64_t slot_base, int64_t n_slots,
                                                              int act_dim, uint64_t draw, double* out) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n_slots * act_dim) return;
  const int64_t s = gid / act_dim;
  out[gid] = philox_uniform(seed, slot_base + (uint64_t)s, (uint32_t)(gid - s * act_dim), draw);
}

}  // namespace

void launch_action_sample(const float* logits, float* actions, int32_t* tokens, int B, int act_dim, int n_vocab,
                          int n_discrete, int action_channels, float tok_min, float tok_max, int discrete, int col_begin,
                          int col_end, const SampleArgs& sp, hipStream_t stream, const uint8_t* slot_flags,
                          const uint8_t* slot_act) {
  LRAM_REQUIRE((slot_flags == nullptr) == (slot_act == nullptr), "action sampling: the slot table's two arrays go together");
  const bool per_slot = slot_flags != nullptr;
  // with a slot table the rows of one launch differ in length: PER comes from the largest, n_vocab (the engine has checked
  // top_k against n_discrete where the table holds a discrete slot)
  const int n = (discrete && !per_slot) ? n_discrete : n_vocab;
  LRAM_REQUIRE(n >= 1 && n <= kSampleMaxRow, "action sampling: a row holds 1 .. 512 logits");
  LRAM_REQUIRE(sp.top_k <= n, "action sampling: top_k exceeds the number of logits of the head in use");
  LRAM_REQUIRE(sp.draw != nullptr, "action sampling: no draw counter");
  const int items = B * ((discrete && !per_slot) ? 1 : act_dim);
  const dim3 grid((items + 3) / 4), block(256);
  if (col_end < 0) col_end = act_dim;
#define LRAM_SAMPLE_LAUNCH(PER)                                                                                      \
  hipLaunchKernelGGL(action_sample_kernel<PER>, grid, block, 0, stream, logits, actions, tokens, B, act_dim, n_vocab, \
                     n_discrete, action_channels, tok_min, tok_max, discrete, col_begin, col_end, sp, slot_flags, slot_act)
  if (n <= 64)
    LRAM_SAMPLE_LAUNCH(1);
  else if (n <= 320)
    LRAM_SAMPLE_LAUNCH(5);
  else
    LRAM_SAMPLE_LAUNCH(8);
#undef LRAM_SAMPLE_LAUNCH
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_sample_advance(uint64_t* draw, hipStream_t stream) {
  hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(64), 0, stream, draw);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_sample_tokens(const float* logits, int64_t rows, int n, int64_t ld, double temperature, int top_k, double top_p,
                          const double* uniform, int32_t* tokens, hipStream_t stream) {
  LRAM_REQUIRE(n >= 1 && n <= kSampleMaxRow, "sample tokens: a row holds 1 .. 512 logits");
  LRAM_REQUIRE(rows >= 1 && rows <= ((int64_t)1 << 32), "sample tokens: rows must be in 1 .. 2^32");
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define LRAM_SAMPLE_LAUNCH(PER)                                                                                \
  hipLaunchKernelGGL(sample_tokens_kernel<PER>, grid, block, 0, stream, logits, rows, n, ld, temperature, top_k, \
                     top_p, uniform, tokens)
  if (n <= 64)
    LRAM_SAMPLE_LAUNCH(1);
  else if (n <= 320)
    LRAM_SAMPLE_LAUNCH(5);
  else
    LRAM_SAMPLE_LAUNCH(8);
#undef LRAM_SAMPLE_LAUNCH
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_sample_uniforms(uint64_t seed, uint64_t slot_base, int64_t n_slots, int act_dim, uint64_t draw, double* out,
                            hipStream_t stream) {
  const int64_t n = n_slots * act_dim;
  LRAM_REQUIRE(n_slots >= 1 && act_dim >= 1 && n <= ((int64_t)1 << 38), "sample uniforms: bad shape");
  hipLaunchKernelGGL(sample_uniforms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed, slot_base,
                     n_slots, act_dim, draw, out);
  LRAM_HIP_CHECK(hipGetLastError());
}

}  // namespace lram
