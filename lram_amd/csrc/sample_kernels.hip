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
// Per-slot settings (lram_set_sampling_slots): action_sample_slots_kernel reads {temperature, top_p, top_k, mode} of the
// wave's env slot from a device table instead of the launch's scalars; mode 0 = greedy, the argmax rule at once.
// logp_row (action_logp_kernel, sample_rows_kernel): the log-probability of a GIVEN token under the same support and
// weights -- t * (x_tok - max) - log(sum over the support of exp(t * (x - max))), fp64, one fp32 rounding at the store.
// The greedy head (action_argmax_kernel) lives here too: the sampling head's twin on the same grid.  The rules every head kernel
// applies to its row -- which columns are in use, the argmax, the de-tokenisation, the staging -- are action_head.h's.
#include "action_head.h"

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

// A value that is the same on every lane of the wave, moved to scalar registers (the compiler cannot see that a table
// entry indexed by the wave's row is wave-uniform).
__device__ __forceinline__ int uniform_i32(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ double uniform_f64(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)uniform_i32((int)(uint32_t)b), hi = (uint32_t)uniform_i32((int)(uint32_t)(b >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
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
// vocabulary order is (lane, j) order.  The row code comes in parts that the draw (sample_row) and the log-probability of a
// given token (logp_row) share: the support (steps 1 and 2), its weights (step 3), the argmax rule.
//
// with_row_support: v = the lane's entries, vmax = the row maximum, bit j of keep = entry j of this lane is in the support;
// body(v, vmax, keep) runs on them and returns true if nothing is left for it.  Returns true (wave-uniform) where the row
// takes the argmax rule instead: greedy (a per-slot setting), a NaN in the row, a maximum of +-inf, or nothing left.
// (The body runs INSIDE the branch that computed the support: ballots and shuffles pin the control flow, so a second branch
// on the same condition would not be merged with the first.)
// MASK (w = the env slot's allowed set, `words` words): the row is its sub-row -- a disallowed entry is padding like one from
// n on (v = -inf, the last key, never kept: invisible, a NaN included), and the quantile ranks the m allowed values.
template <int PER, bool MASK = false, class Body>
__device__ __forceinline__ bool with_row_support(const float* row, int n, int top_k, double top_p, int lane, bool greedy,
                                                 Body&& body, const uint32_t* w = nullptr, int words = 0) {
  float v[PER];
  float vmax = -INFINITY;
  uint32_t key[PER];
  bool nan_here = false;
  uint32_t allow = (1u << PER) - 1u;
  if constexpr (MASK) allow = mask_lane_bits<PER>(w, words, lane);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = lane * PER + j;
    if constexpr (MASK)
      v[j] = (i < n && ((allow >> j) & 1u)) ? row[i] + 0.f : -INFINITY;
    else
      v[j] = i < n ? row[i] + 0.f : -INFINITY;  // (-0 -> +0: one key per value)
    nan_here |= v[j] != v[j];
    vmax = fmaxf(vmax, v[j]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
  bool plain = greedy || __any(nan_here) || vmax == INFINITY || vmax == -INFINITY;
  if (!plain) {
    uint32_t keep = 0;  // bit j: entry j of this lane is in the support
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const bool valid = lane * PER + j < n && (!MASK || ((allow >> j) & 1u));
    key[j] = valid ? order_key(v[j]) : 0xffffffffu;  // padding sorts last
    keep |= (valid ? 1u : 0u) << j;
  }
  if (top_p > 0.0) {
    int m = n;  // the values the quantile ranks: the sub-row's (wave-uniform; >= 1 here: its maximum is finite)
    if constexpr (MASK) m = mask_count(w, words, n, lane);
    const double rank = top_p * (double)(m - 1);
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
    if (body(v, vmax, keep)) plain = true;
  }
  return plain;
}

// w[j] = exp(temperature * (v[j] - vmax)) on the support, 0 elsewhere.  Returns the lane's sum.
template <int PER>
__device__ __forceinline__ double row_weights(const float (&v)[PER], float vmax, uint32_t keep, double temperature,
                                              double (&w)[PER]) {
  double loc = 0.0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    w[j] = ((keep >> j) & 1u) ? exp(temperature * ((double)v[j] - (double)vmax)) : 0.0;
    loc += w[j];
  }
  return loc;
}
// The inclusive scan of the lanes' sums, in lane (= vocabulary) order; lane 63 holds the row's total.  Outside (0, inf)
// nothing is left (a quantile that is NaN) and the row takes the argmax rule.
__device__ __forceinline__ double wave_scan_f64(double inc, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  return inc;
}

// The draw.  Returns the token (wave-uniform); greedy (a per-slot setting, wave-uniform): the argmax rule at once.
template <int PER, bool MASK = false>
__device__ __forceinline__ int sample_row(const float* row, int n, double temperature, int top_k, double top_p, double u,
                                          int lane, bool greedy = false, const uint32_t* w = nullptr, int words = 0) {
  int token = 0x7fffffff;
  const bool plain = with_row_support<PER, MASK>(row, n, top_k, top_p, lane, greedy, [&](const float (&v)[PER], float vmax, uint32_t keep) {
    double w[PER];
    const double inc = wave_scan_f64(row_weights<PER>(v, vmax, keep, temperature, w), lane);
    const double total = __shfl(inc, 63, 64);
    if (!(total > 0.0 && total < (double)INFINITY)) return true;  // nothing left (a quantile that is NaN): the argmax rule
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
    return false;
  }, w, words);
  if constexpr (MASK) {
    if (plain) token = row_argmax_masked(row, n, lane, w);
  } else {
    if (plain) token = row_argmax(row, n, lane);
  }
  return token;
}

// log of the probability with which sample_row returns `tok` (wave-uniform) from this row under these settings:
// t * (x_tok - max) - log(sum over the support of exp(t * (x - max))), fp64 throughout; the caller rounds once to fp32.
// Outside 0 .. n - 1 or outside the support: -inf.  A row on the argmax rule: 0 at the argmax token, -inf elsewhere.
template <int PER, bool MASK = false>
__device__ __forceinline__ double logp_row(const float* row, int n, double temperature, int top_k, double top_p, int tok,
                                           int lane, bool greedy, const uint32_t* w = nullptr, int words = 0) {
  double lp = -(double)INFINITY;
  const bool plain = with_row_support<PER, MASK>(row, n, top_k, top_p, lane, greedy, [&](const float (&v)[PER], float vmax, uint32_t keep) {
    double w[PER], z = -(double)INFINITY;
    const double loc = row_weights<PER>(v, vmax, keep, temperature, w);
#pragma unroll
    for (int j = 0; j < PER; ++j)   // (ahead of the scan: the weights are not kept across it; w = 0: never drawn)
      if (lane * PER + j == tok && w[j] > 0.0) z = temperature * ((double)v[j] - (double)vmax);
    const double total = __shfl(wave_scan_f64(loc, lane), 63, 64);   // the draw's own total, bit for bit
    if (!(total > 0.0 && total < (double)INFINITY)) return true;
    if (tok >= 0 && tok < n) {
      z = __shfl(z, tok / PER, 64);  // from the lane that holds the token
      lp = z - log(total);           // (the support holds the maximum: total >= 1; a support of one entry gives 0 - log(1))
    }
    return false;
  }, w, words);
  if constexpr (MASK) {
    if (plain) lp = tok == row_argmax_masked(row, n, lane, w) ? 0.0 : -(double)INFINITY;
  } else {
    if (plain) lp = tok == row_argmax(row, n, lane) ? 0.0 : -(double)INFINITY;
  }
  return lp;
}

// The grid of an env-step's head (argmax and sampling): one wave per (env, action dim), four per workgroup -- over all act_dim
// columns, or over column 0 alone on a discrete call without a slot table (columns j >= 1 are then left alone).  `live`: the
// wave has a column, and it lies in col_begin .. col_end - 1 (repeated-forward mode: pass p writes action dim p, the last pass
// every dim from its own on, engine_step.hip::action_head).
__host__ __device__ __forceinline__ int step_columns(const HeadGeom& g, const HeadSlots& s, int discrete) {
  return (discrete && s.flags == nullptr) ? 1 : g.act_dim;
}
struct StepItem {
  int b, j;
  bool live;
};
__device__ __forceinline__ StepItem step_item(int B, const HeadGeom& g, const HeadSlots& s, int discrete, int col_begin,
                                              int col_end) {
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6), ndim = step_columns(g, s, discrete);
  StepItem it;
  it.b = item / ndim, it.j = item - it.b * ndim;
  it.live = item < B * ndim && it.j >= col_begin && it.j < col_end;
  return it;
}
// lane 0: the column's token (where asked for) and its action
__device__ __forceinline__ void store_action(int64_t o, int tok, int discrete, const HeadGeom& g, int32_t* tokens, float* actions) {
  if (tokens != nullptr) tokens[o] = tok;
  if (actions != nullptr) actions[o] = detokenise(tok, discrete, g);
}

// The greedy head: first index of the row's maximum (torch.argmax rule), then inv_tokenize.  Nothing is staged: the row is
// walked once in global memory, and a wave without work returns at once.
template <bool MASK>
__device__ __forceinline__ void action_argmax_body(const float* logits, float* actions, int32_t* tokens, int B, const HeadGeom& g,
                                                   const HeadSlots& s, int discrete, int col_begin, int col_end,
                                                   const HeadMask& mask) {
  const int lane = threadIdx.x & 63;
  const StepItem it = step_item(B, g, s, discrete, col_begin, col_end);
  if (!it.live) return;
  const HeadCol col = head_column(g, s, discrete, it.b, it.j);
  const int64_t o = (int64_t)it.b * g.act_dim + it.j;
  if (col.fill) {
    if (lane == 0) store_fill(o, tokens, actions, nullptr);
    return;
  }
  int tok;
  if constexpr (MASK)
    tok = row_argmax_masked(logits + o * g.n_vocab, col.n, lane, mask_words(mask, it.b));
  else
    tok = row_argmax(logits + o * g.n_vocab, col.n, lane);
  if (lane == 0) store_action(o, tok, col.discrete, g, tokens, actions);
}
__global__ __launch_bounds__(256) void action_argmax_kernel(const float* logits, float* actions, int32_t* tokens, int B,
                                                            HeadGeom g, HeadSlots s, int discrete, int col_begin, int col_end) {
  action_argmax_body<false>(logits, actions, tokens, B, g, s, discrete, col_begin, col_end, HeadMask{});
}
// Its twin under allowed sets (mask.bits starts at the launch's first env slot): the walk over the sub-row.
__global__ __launch_bounds__(256) void action_argmax_masked_kernel(const float* logits, float* actions, int32_t* tokens, int B,
                                                                   HeadGeom g, HeadSlots s, int discrete, int col_begin,
                                                                   int col_end, HeadMask mask) {
  action_argmax_body<true>(logits, actions, tokens, B, g, s, discrete, col_begin, col_end, mask);
}

// Its sampling counterpart, same grid.  sp.draw is read, never written, here: sample_advance_kernel bumps it once per env-step
// behind every head launch of that step.
// SLOTS: the settings come from the per-slot table (lram_set_sampling_slots; `slots` starts at the launch's first env slot)
// instead of sp's scalars -- a compile-time split, so that the launch without a table is the code it was before the table.
// MASK: the env slot's allowed set (mask.bits starts at the launch's first env slot, like `slots`); the masked kernel reads the
// settings from the table where one is given and from sp's scalars otherwise (one instance per PER: it is not the hot launch).
template <int PER, bool SLOTS, bool MASK = false>
__device__ __forceinline__ void action_sample_body(float (&stage)[4][64 * PER], const float* logits, float* actions,
                                                   int32_t* tokens, int B, const HeadGeom& g, const HeadSlots& s, int discrete,
                                                   int col_begin, int col_end, const SampleArgs& sp, const SampleSlot* slots,
                                                   const HeadMask& mask = {}) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const StepItem it = step_item(B, g, s, discrete, col_begin, col_end);
  const int b = it.b, j = it.j;
  HeadCol col{discrete};
  if (it.live) col = head_column(g, s, discrete, b, j);
  const bool active = it.live && !col.fill;
  const int64_t o = (int64_t)b * g.act_dim + j;
  stage_row<PER>(stage[wv], logits + o * g.n_vocab, col.n, lane, active);
  if (col.fill && lane == 0) store_fill(o, tokens, actions, nullptr);
  if (!active) return;
  const double u = philox_uniform(sp.seed, sp.slot0 + (uint64_t)b, (uint32_t)j, *sp.draw);
  int tok;
  if constexpr (MASK) {
    double t = sp.temperature, p = sp.top_p;
    int k = sp.top_k;
    bool greedy = false;
    if (slots != nullptr) {
      const SampleSlot st = slots[b];
      t = st.temperature, p = st.top_p, k = st.top_k, greedy = st.mode == 0;
    }
    tok = sample_row<PER, true>(stage[wv], col.n, uniform_f64(t), uniform_i32(k), uniform_f64(p), u, lane,
                                uniform_i32(greedy) != 0, mask_words(mask, b), mask.words);
  } else if constexpr (SLOTS) {  // the env slot's own settings (wave-uniform, like the slot table's entry)
    const SampleSlot st = slots[b];
    tok = sample_row<PER>(stage[wv], col.n, st.temperature, st.top_k, st.top_p, u, lane, st.mode == 0);
  } else {
    tok = sample_row<PER>(stage[wv], col.n, sp.temperature, sp.top_k, sp.top_p, u, lane);
  }
  if (lane == 0) store_action(o, tok, col.discrete, g, tokens, actions);
}

template <int PER>
__global__ __launch_bounds__(256) void action_sample_kernel(const float* logits, float* actions, int32_t* tokens, int B,
                                                            HeadGeom g, HeadSlots s, int discrete, int col_begin, int col_end,
                                                            SampleArgs sp) {
  __shared__ float stage[4][64 * PER];
  action_sample_body<PER, false>(stage, logits, actions, tokens, B, g, s, discrete, col_begin, col_end, sp, nullptr);
}

template <int PER>
__global__ __launch_bounds__(256) void action_sample_slots_kernel(const float* logits, float* actions, int32_t* tokens, int B,
                                                                  HeadGeom g, HeadSlots s, int discrete, int col_begin,
                                                                  int col_end, SampleArgs sp, const SampleSlot* slots) {
  __shared__ float stage[4][64 * PER];
  action_sample_body<PER, true>(stage, logits, actions, tokens, B, g, s, discrete, col_begin, col_end, sp, slots);
}

template <int PER>
__global__ __launch_bounds__(256) void action_sample_masked_kernel(const float* logits, float* actions, int32_t* tokens, int B,
                                                                   HeadGeom g, HeadSlots s, int discrete, int col_begin,
                                                                   int col_end, SampleArgs sp, const SampleSlot* slots,
                                                                   HeadMask mask) {
  __shared__ float stage[4][64 * PER];
  action_sample_body<PER, false, true>(stage, logits, actions, tokens, B, g, s, discrete, col_begin, col_end, sp, slots, mask);
}

// log-probabilities of given tokens under the distribution the head above draws from: always act_dim columns per env (as
// action_score_kernel), same rows, same settings -- sp's scalars, or the per-slot table where `slots` is given.
// Columns the head does not use and token -1 get the fill value 0.
template <int PER, bool MASK>
__device__ __forceinline__ void action_logp_body(float (&stage)[4][64 * PER], const float* logits, const int32_t* tokens,
                                                 float* logp, int B, const HeadGeom& g, const HeadSlots& s, int discrete,
                                                 const SampleArgs& sp, const SampleSlot* slots, const HeadMask& mask) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int item = blockIdx.x * 4 + wv;
  const int b = item / g.act_dim, j = item - b * g.act_dim;
  const bool in_grid = item < B * g.act_dim;
  const int64_t o = (int64_t)b * g.act_dim + j;
  HeadCol col{discrete};
  int tok = -1;
  if (in_grid) {  // (every condition below is the same for the whole wave)
    col = head_column(g, s, discrete, b, j);
    tok = tokens[o];
    col.fill = col.fill || tok == -1;
  }
  const bool active = in_grid && !col.fill;
  stage_row<PER>(stage[wv], logits + o * g.n_vocab, col.n, lane, active);
  if (col.fill && lane == 0) store_fill(o, nullptr, nullptr, logp);
  if (!active) return;
  double temperature = sp.temperature, top_p = sp.top_p;
  int top_k = sp.top_k;
  bool greedy = false;
  if (slots != nullptr) {
    const SampleSlot st = slots[b];
    temperature = st.temperature, top_p = st.top_p, top_k = st.top_k, greedy = st.mode == 0;
  }
  double lp;
  if constexpr (MASK)
    lp = logp_row<PER, true>(stage[wv], col.n, uniform_f64(temperature), uniform_i32(top_k), uniform_f64(top_p),
                             uniform_i32(tok), lane, uniform_i32(greedy) != 0, mask_words(mask, b), mask.words);
  else
    lp = logp_row<PER>(stage[wv], col.n, uniform_f64(temperature), uniform_i32(top_k), uniform_f64(top_p),
                       uniform_i32(tok), lane, uniform_i32(greedy) != 0);
  if (lane == 0) logp[o] = (float)lp;
}
template <int PER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void action_logp_kernel(
    const float* logits, const int32_t* tokens, float* logp, int B, HeadGeom g, HeadSlots s, int discrete, SampleArgs sp,
    const SampleSlot* slots) {
  __shared__ float stage[4][64 * PER];
  action_logp_body<PER, false>(stage, logits, tokens, logp, B, g, s, discrete, sp, slots, HeadMask{});
}
template <int PER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void action_logp_masked_kernel(
    const float* logits, const int32_t* tokens, float* logp, int B, HeadGeom g, HeadSlots s, int discrete, SampleArgs sp,
    const SampleSlot* slots, HeadMask mask) {
  __shared__ float stage[4][64 * PER];
  action_logp_body<PER, true>(stage, logits, tokens, logp, B, g, s, discrete, sp, slots, mask);
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

// Test / evidence entry with per-row settings (device arrays of length rows): draws (uniform -> tokens_out) and / or
// log-probabilities of given tokens (tokens_in -> logp_out; token -1: the fill value 0) through the row code of the head.
template <int PER, bool MASK>
__device__ __forceinline__ void sample_rows_body(float (&stage)[4][64 * PER], const float* logits, int64_t rows, int n, int64_t ld,
                                                 const uint8_t* mode, const double* temperature, const int32_t* top_k,
                                                 const double* top_p, const double* uniform, const int32_t* tokens_in,
                                                 int32_t* tokens_out, float* logp_out, const HeadMask& mask) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wv;
  const bool active = r < rows;
  stage_row<PER>(stage[wv], logits + (active ? r : 0) * ld, n, lane, active);
  if (!active) return;
  double t = temperature[r], p = top_p[r];
  int k = top_k[r];
  bool greedy = mode[r] == 0;
  const uint32_t* w = nullptr;
  if constexpr (MASK) {  // row r's own set; the row's settings are wave-uniform: scalar registers, as in action_logp_kernel
    w = mask_words(mask, r);
    t = uniform_f64(t), p = uniform_f64(p), k = uniform_i32(k), greedy = uniform_i32(greedy) != 0;
  }
  if (tokens_out != nullptr) {
    const int tok = sample_row<PER, MASK>(stage[wv], n, t, k, p, uniform[r], lane, greedy, w, mask.words);
    if (lane == 0) tokens_out[r] = tok;
  }
  if (logp_out != nullptr) {
    const int tok = tokens_in[r];
    const double lp = tok == -1 ? 0.0 : logp_row<PER, MASK>(stage[wv], n, t, k, p, tok, lane, greedy, w, mask.words);
    if (lane == 0) logp_out[r] = (float)lp;
  }
}
template <int PER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void sample_rows_kernel(const float* logits, int64_t rows, int n, int64_t ld,
                                                          const uint8_t* mode, const double* temperature, const int32_t* top_k,
                                                          const double* top_p, const double* uniform, const int32_t* tokens_in,
                                                          int32_t* tokens_out, float* logp_out) {
  __shared__ float stage[4][64 * PER];
  sample_rows_body<PER, false>(stage, logits, rows, n, ld, mode, temperature, top_k, top_p, uniform, tokens_in, tokens_out, logp_out,
                               HeadMask{});
}
template <int PER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void sample_rows_masked_kernel(
    const float* logits, int64_t rows, int n, int64_t ld, const uint8_t* mode, const double* temperature, const int32_t* top_k,
    const double* top_p, const double* uniform, const int32_t* tokens_in, int32_t* tokens_out, float* logp_out, HeadMask mask) {
  __shared__ float stage[4][64 * PER];
  sample_rows_body<PER, true>(stage, logits, rows, n, ld, mode, temperature, top_k, top_p, uniform, tokens_in, tokens_out, logp_out,
                              mask);
}

__global__ __launch_bounds__(256) void sample_uniforms_kernel(uint64_t seed, uint64_t slot_base, int64_t n_slots,
                                                              int act_dim, uint64_t draw, double* out) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n_slots * act_dim) return;
  const int64_t s = gid / act_dim;
  out[gid] = philox_uniform(seed, slot_base + (uint64_t)s, (uint32_t)(gid - s * act_dim), draw);
}

}  // namespace

void launch_action_argmax(const float* logits, float* actions, int32_t* tokens, int B, const HeadGeom& g, const HeadSlots& s,
                          int discrete, int col_begin, int col_end, hipStream_t stream, const HeadMask& mask) {
  LRAM_REQUIRE((s.flags == nullptr) == (s.act == nullptr), "action head: the slot table's two arrays go together");
  LRAM_REQUIRE(mask.bits == nullptr || mask.words == (g.n_vocab + 31) / 32, "action head: the mask holds ceil(n_vocab / 32) words per slot");
  // with a slot table: one wave per (env, action dim) over all act_dim columns, the head mode is read per env slot
  const int items = B * step_columns(g, s, discrete);
  if (mask.bits != nullptr)
    hipLaunchKernelGGL(action_argmax_masked_kernel, dim3((items + 3) / 4), dim3(256), 0, stream, logits, actions, tokens, B, g, s,
                       discrete, col_begin, col_end, mask);
  else
    hipLaunchKernelGGL(action_argmax_kernel, dim3((items + 3) / 4), dim3(256), 0, stream, logits, actions, tokens, B, g, s,
                       discrete, col_begin, col_end);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_action_sample(const float* logits, float* actions, int32_t* tokens, int B, const HeadGeom& g, const HeadSlots& s,
                          int discrete, int col_begin, int col_end, const SampleArgs& sp, const SampleSlot* slots,
                          hipStream_t stream, const HeadMask& mask) {
  LRAM_REQUIRE((s.flags == nullptr) == (s.act == nullptr), "action sampling: the slot table's two arrays go together");
  const bool per_slot = s.flags != nullptr;
  // with a slot table the rows of one launch differ in length: PER comes from the largest, n_vocab (the engine has checked
  // top_k against n_discrete where the table holds a discrete slot)
  const int n = (discrete && !per_slot) ? g.n_discrete : g.n_vocab;
  LRAM_REQUIRE(n >= 1 && n <= kSampleMaxRow, "action sampling: a row holds 1 .. 512 logits");
  // (per-slot settings: the engine has checked every sampling slot's top_k against the head that slot gets)
  LRAM_REQUIRE(slots != nullptr || sp.top_k <= n, "action sampling: top_k exceeds the number of logits of the head in use");
  LRAM_REQUIRE(sp.draw != nullptr, "action sampling: no draw counter");
  const int items = B * step_columns(g, s, discrete);
  const dim3 grid((items + 3) / 4), block(256);
  LRAM_REQUIRE(mask.bits == nullptr || mask.words == (g.n_vocab + 31) / 32,
               "action sampling: the mask holds ceil(n_vocab / 32) words per slot");
  with_per(n, [&](auto per) {
    if (mask.bits != nullptr)
      hipLaunchKernelGGL(action_sample_masked_kernel<decltype(per)::value>, grid, block, 0, stream, logits, actions, tokens, B, g, s,
                         discrete, col_begin, col_end, sp, slots, mask);
    else if (slots == nullptr)
      hipLaunchKernelGGL(action_sample_kernel<decltype(per)::value>, grid, block, 0, stream, logits, actions, tokens, B, g, s, discrete,
                         col_begin, col_end, sp);
    else
      hipLaunchKernelGGL(action_sample_slots_kernel<decltype(per)::value>, grid, block, 0, stream, logits, actions, tokens, B, g, s, discrete,
                         col_begin, col_end, sp, slots);
  });
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_action_logp(const float* logits, const int32_t* tokens, float* logp, int B, const HeadGeom& g, const HeadSlots& s,
                        int discrete, const SampleArgs& sp, const SampleSlot* slots, hipStream_t stream, const HeadMask& mask) {
  LRAM_REQUIRE((s.flags == nullptr) == (s.act == nullptr), "action logp: the slot table's two arrays go together");
  LRAM_REQUIRE(logits && tokens && logp && B >= 1 && g.act_dim >= 1, "action logp: bad arguments");
  const int n = (discrete && s.flags == nullptr) ? g.n_discrete : g.n_vocab;
  LRAM_REQUIRE(n >= 1 && n <= kSampleMaxRow && g.n_discrete <= g.n_vocab, "action logp: a row holds 1 .. 512 logits");
  LRAM_REQUIRE(slots != nullptr || sp.top_k <= n, "action logp: top_k exceeds the number of logits of the head in use");
  const dim3 grid((B * g.act_dim + 3) / 4), block(256);
  LRAM_REQUIRE(mask.bits == nullptr || mask.words == (g.n_vocab + 31) / 32, "action logp: the mask holds ceil(n_vocab / 32) words per slot");
  with_per(n, [&](auto per) {
    if (mask.bits != nullptr)
      hipLaunchKernelGGL(action_logp_masked_kernel<decltype(per)::value>, grid, block, 0, stream, logits, tokens, logp, B, g, s,
                         discrete, sp, slots, mask);
    else
      hipLaunchKernelGGL(action_logp_kernel<decltype(per)::value>, grid, block, 0, stream, logits, tokens, logp, B, g, s, discrete, sp, slots);
  });
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
  with_per(n, [&](auto per) {
    hipLaunchKernelGGL(sample_tokens_kernel<decltype(per)::value>, grid, block, 0, stream, logits, rows, n, ld, temperature, top_k, top_p,
                       uniform, tokens);
  });
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_sample_rows(const float* logits, int64_t rows, int n, int64_t ld, const uint8_t* mode, const double* temperature,
                        const int32_t* top_k, const double* top_p, const double* uniform, const int32_t* tokens_in,
                        int32_t* tokens_out, float* logp_out, hipStream_t stream, const HeadMask& mask) {
  LRAM_REQUIRE(n >= 1 && n <= kSampleMaxRow, "sample rows: a row holds 1 .. 512 logits");
  LRAM_REQUIRE(rows >= 1 && rows <= ((int64_t)1 << 32), "sample rows: rows must be in 1 .. 2^32");
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  LRAM_REQUIRE(mask.bits == nullptr || mask.words == (n + 31) / 32, "sample rows: the mask holds ceil(n / 32) words per row");
  with_per(n, [&](auto per) {
    if (mask.bits != nullptr)
      hipLaunchKernelGGL(sample_rows_masked_kernel<decltype(per)::value>, grid, block, 0, stream, logits, rows, n, ld, mode, temperature,
                         top_k, top_p, uniform, tokens_in, tokens_out, logp_out, mask);
    else
      hipLaunchKernelGGL(sample_rows_kernel<decltype(per)::value>, grid, block, 0, stream, logits, rows, n, ld, mode, temperature, top_k, top_p,
                         uniform, tokens_in, tokens_out, logp_out);
  });
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
