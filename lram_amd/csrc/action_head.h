// The action head's row rules, once: what a wave does with its (env, action dim) is the same in the argmax, sampling, logp and
// score kernels (sample_kernels.hip, score_kernels.hip), so a row gives the same token and action from whichever of them reads it.
//
// Reference functions replaced: torch.argmax + MinMaxTokenizer.inv_tokenize (src/algos/models/multi_domain_discrete_dt_model.py:83-94,
// src/tokenizers_custom/minmax_tokenizer.py:31-47).
#pragma once
#include <type_traits>

#include "common.h"
#include "device_math.h"

namespace lram {

// The column rule.  A wave's column (env, action dim j) under the call's head mode `discrete`, or with a slot table
// (LRAM_HEAD_PER_SLOT) under the env slot's own: n = the number of logits it selects from, fill = a column the head does not use
// (j >= act_dim[slot]; j >= 1 of a discrete call), which holds the fill values on every call.  Wave-uniform (the wave's row
// decides); no barrier, no LDS: a kernel may return on it.
struct HeadCol {
  int discrete;
  int n = 0;
  bool fill = false;
};
__device__ __forceinline__ HeadCol head_column(const HeadGeom& g, const HeadSlots& s, int discrete, int64_t env, int j) {
  HeadCol c{discrete};
  if (s.flags != nullptr) {
    c.discrete = s.flags[env] & 1;
    c.fill = j >= (int)s.act[env];
  } else {
    c.fill = discrete && j >= 1;
  }
  c.n = c.discrete ? g.n_discrete : g.n_vocab;
  return c;
}

// The fill values of output element o: token -1, action 0, logp 0, each where the pointer is given.
__device__ __forceinline__ void store_fill(int64_t o, int32_t* tokens, float* actions, float* logp) {
  if (tokens != nullptr) tokens[o] = -1;
  if (actions != nullptr) actions[o] = 0.f;
  if (logp != nullptr) logp[o] = 0.f;
}

// The wave argmax by argmax_beats, from (best, bi) = (-inf, INT_MAX): argmax_take per element of the lane's walk, wave_argmax
// across the lanes (every lane ends with the row's winner; `vmax`, where given, becomes the wave's maximum of it on the same
// shuffle steps, so that a kernel that needs both pays the cross-lane latency once).
__device__ __forceinline__ void argmax_take(float x, int i, float& best, int& bi, bool in_range = true) {
  const bool take = in_range && argmax_beats(x, i, best, bi);  // (two selects: a branch here costs the walk its speed)
  best = take ? x : best;
  bi = take ? i : bi;
}
__device__ __forceinline__ void wave_argmax(float& best, int& bi, float* vmax = nullptr) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    argmax_take(ov, oi, best, bi);
    if (vmax != nullptr) *vmax = fmaxf(*vmax, __shfl_xor(*vmax, off, 64));
  }
}
__device__ __forceinline__ int row_argmax(const float* row, int n, int lane) {
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = lane; i < n; i += 64) argmax_take(row[i], i, best, bi);
  wave_argmax(best, bi);
  return bi;
}

// The allowed-set rule (lram_set_action_mask).  A column works on the SUB-ROW x[i], i in S within [0, n), in vocabulary order,
// where S is its env slot's allowed set: a disallowed entry is not there, whatever it holds.  `w` = the slot's words.
// Every kernel takes the rule as a compile-time MASK: the instances without it are the code they were.
// (every lane of a wave has the wave's env: the slot's pointer is moved to scalar registers, its words are scalar loads)
__device__ __forceinline__ const uint32_t* mask_words(const HeadMask& m, int64_t env) {
  const uint64_t p = reinterpret_cast<uint64_t>(m.bits + env * m.words);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(p >> 32));
  return reinterpret_cast<const uint32_t*>(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ bool mask_allows(const uint32_t* w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }
// The argmax rule over the sub-row (one word read per element: the walk is lane-strided).  With a non-empty sub-row it ends
// on a real index of it: argmax_beats from (-inf, INT_MAX) takes the first entry it sees, NaN and -inf included.
__device__ __forceinline__ int row_argmax_masked(const float* row, int n, int lane, const uint32_t* w) {
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = lane; i < n; i += 64) argmax_take(row[i], i, best, bi, mask_allows(w, i));
  wave_argmax(best, bi);
  return bi;
}
// Staged rows (n <= 512: at most 16 words): lane l holds the PER (<= 8) consecutive entries from l * PER on, so its bits
// come from at most two adjacent words.  Bit j of the result = entry l * PER + j is allowed; entries from 32 * words on are
// not (the word behind a slot's last word is never read: behind the last slot's it is past the allocation).
template <int PER>
__device__ __forceinline__ uint32_t mask_lane_bits(const uint32_t* w, int words, int lane) {
  static_assert(PER >= 1 && PER <= 8, "a lane's entries span at most two words");
  const int first = lane * PER, k = first >> 5;
  if (k >= words) return 0u;
  const uint64_t lo = w[k], hi = k + 1 < words ? w[k + 1] : 0u;
  return (uint32_t)(((hi << 32) | lo) >> (first & 31)) & ((1u << PER) - 1u);
}
// m = |S within [0, n)|, wave-uniform: lanes 0 .. words - 1 count their word cut at n, then a wave sum (words <= 64).
__device__ __forceinline__ int mask_count(const uint32_t* w, int words, int n, int lane) {
  int cnt = 0;
  if (lane < words && lane * 32 < n) {
    const int left = n - lane * 32;  // >= 1
    const uint32_t cut = left >= 32 ? 0xffffffffu : (1u << left) - 1u;
    cnt = __popc(w[lane] & cut);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  return cnt;
}

// The action of a token: the token itself on a discrete column, otherwise inv_tokenize of its bin.
__device__ __forceinline__ float head_bin_width(const HeadGeom& g) { return (g.tok_max - g.tok_min) / (float)g.action_channels; }
__device__ __forceinline__ float detokenise(int tok, int discrete, const HeadGeom& g) {
  if (discrete) return (float)tok;
  int t = tok - g.n_discrete;
  t = t < 0 ? 0 : t;
  return inv_tokenize_bin(t, head_bin_width(g), g.tok_min);  // two roundings, as the reference: no FMA
}

// A wave's row: global -> its LDS strip, coalesced, read once -- and, where `copy` is given, on to copy[copy_at + i] (the pointer
// stays the launch's own, so that the test for it is a scalar branch).  Every wave of the workgroup reaches the barrier behind it.
template <int PER>
__device__ __forceinline__ void stage_row(float* strip, const float* src, int n, int lane, bool active, float* copy = nullptr,
                                          int64_t copy_at = 0) {
  if (active) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = lane + 64 * j;
      if (i < n) {
        const float x = src[i];
        strip[i] = x;
        if (copy != nullptr) copy[copy_at + i] = x;
      }
    }
  }
  __syncthreads();
}

// Host: f(std::integral_constant<int, PER>) with the PER (floats per lane of a staged row) of rows of n <= kSampleMaxRow logits.
template <class F>
void with_per(int n, F&& f) {
  if (n <= 64)
    f(std::integral_constant<int, 1>{});
  else if (n <= 320)
    f(std::integral_constant<int, 5>{});
  else
    f(std::integral_constant<int, 8>{});
}

}  // namespace lram
