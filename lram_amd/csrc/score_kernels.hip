// Action head, scoring mode: per (row, action dim) the greedy token, the de-tokenised greedy action and the log-probability
// of a GIVEN target token under the row's logits -- what grading a stored trajectory needs at every timestep.
//
// Reference computation replaced: the cross-entropy of the recorded actions under the no-cache forward's action logits
// (src/algos/universal_decision_transformer_sb3.py:398-434: tokenize_actions of the float targets, CE over act_dim x n_vocab),
// with the targets tokenised as MinMaxTokenizer.tokenize does (src/tokenizers_custom/minmax_tokenizer.py:14-29) and
// `temperature` multiplying the logits as sample_from_logits does (src/algos/models/model_utils.py:7-32).
//
// One wave per (row, action dim), four per workgroup, as action_argmax_kernel and action_sample_kernel (sample_kernels.hip).
// The row is read from global memory ONCE, coalesced, into the wave's LDS strip (and on the way, if asked, copied to the caller's
// logits tensor); everything else walks the strip:
//   greedy token   first index of the maximum over the selectable range, then its action: the rules of action_head.h, which the
//                  argmax and sampling kernels apply too -- a row gives the same token and action on all of them
//   target token   an int32 token, or a float action tokenised here: trunc((x - min) / bin_width) clamped to
//                  0 .. action_channels - 1, plus n_discrete -- fp32 subtract, IEEE fp32 division; discrete rows: (int)x
//   logp           t * x[target] - logsumexp(t * x) over the normalisation range; maximum, sum and log in fp64, one fp32
//                  rounding at the store.  over = 0: all n_vocab logits (the reference's CE); over = 1: the selectable range
//                  (n_discrete on discrete rows, n_vocab otherwise: what the sampling head draws from)
// A target outside the normalisation range or a non-finite float target: -inf.  A NaN in the range: NaN.  A -inf logit at the
// target: -inf.  Rows with valid[row] == 0, columns j >= act_dim[slot] of a slot table and columns j >= 1 of a discrete call
// write logp 0, token -1, action 0 and nothing else (wave-uniform branch).  Rows wider than 512 logits are not staged: they
// are walked in global memory (the second walk is served by the cache).
#include "action_head.h"

namespace lram {
namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// t * x - zmax with the product rounded to fp64 BEFORE the subtraction.  Fused into one fma the product would keep its
// exact low bits, the row's maximum would not cancel against zmax = t * max x, and a one-logit row would score -7e-17, not 0.
__device__ __forceinline__ double scaled_minus(double t, float x, double zmax) {
#pragma clang fp contract(off)
  const double z = t * (double)x;
  return z - zmax;
}

// The wave's item: (row r of the launch, action dim j); its env and the row `orow` of the outputs, targets and `valid`.
struct ScoreItem {
  bool in_grid;
  int64_t r, env, orow;
  int j;
  bool pad;   // a padded timestep of a per-env-length call: the fill values, nothing read
};

__device__ __forceinline__ ScoreItem score_item(const ScoreArgs& a) {
  ScoreItem it;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  it.in_grid = item < a.rows * a.geom.act_dim;
  it.r = it.in_grid ? item / a.geom.act_dim : 0;
  it.j = it.in_grid ? (int)(item - it.r * a.geom.act_dim) : 0;
  const int64_t g = a.row0 + it.r;
  it.env = g / a.inner;
  it.orow = it.env * a.outer + a.off + (g - it.env * a.inner);
  it.pad = false;
  return it;
}

// The same with the contexts END-aligned inside the call (ScoreArgs::start): row g is call-timestep t of its env; its outputs go
// to the left-aligned row t - start[env], those of a padded timestep (t < start[env]) as fill values to row n_env + t.  Over the
// call-timesteps 0 .. outer - 1 of an env this is a bijection onto its rows.
__device__ __forceinline__ ScoreItem score_item_ragged(const ScoreArgs& a) {
  ScoreItem it = score_item(a);
  const int64_t t = it.orow - it.env * a.outer;
  const int64_t s = it.in_grid ? (int64_t)a.start[it.env] : 0;
  it.pad = it.in_grid && t < s;
  it.orow = it.env * a.outer + (it.pad ? (a.outer - s) + t : t - s);
  return it;
}

// PER floats per lane in the wave's LDS strip; PER = 0: no strip, the row stays in global memory.
// MASK (`mask`, the env's allowed set): the greedy token is the argmax of the sub-row; with over = 1 the maximum, the NaN flag and
// the sum run over the sub-row too and a target outside it scores -inf; with over = 0 the normalisation is what it is without a mask.
template <int PER, bool MASK>
__device__ __forceinline__ void score_row(const ScoreArgs& a, const ScoreItem& it, float (*stage)[64 * (PER > 0 ? PER : 1)],
                                          const HeadMask& mask = {}) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const HeadGeom& g = a.geom;
  const int64_t o = it.orow * g.act_dim + it.j;
  HeadCol col{a.discrete};
  if (it.in_grid) {  // (every condition below is the same for the whole wave)
    if (it.pad || (a.valid != nullptr && a.valid[it.orow] == 0))
      col.fill = true;
    else
      col = head_column(g, a.slots, a.discrete, it.env, it.j);
  }
  const bool active = it.in_grid && !col.fill;
  const int nsel = col.n;                                    // the greedy token's range
  const int nnorm = a.over ? nsel : g.n_vocab;               // the softmax's range (>= nsel)
  const int nread = (a.logits_out != nullptr || !a.over) ? g.n_vocab : nsel;
  const float* row = a.logits + it.r * a.ld + (int64_t)it.j * g.n_vocab;
  if constexpr (PER > 0) {
    stage_row<PER>(stage[wv], row, nread, lane, active, a.logits_out, o * g.n_vocab);
    row = stage[wv];
  } else {
    if (active && a.logits_out != nullptr)
      for (int i = lane; i < nread; i += 64) a.logits_out[o * g.n_vocab + i] = row[i];
  }
  if (col.fill && lane == 0) store_fill(o, a.tokens, a.actions, a.logp);
  if (!active) return;

  // one walk: the greedy token over the selectable range, the maximum and the NaN flag over the normalisation range
  float best = -INFINITY, vmax = -INFINITY;
  int bi = 0x7fffffff;
  bool nan_here = false;
  const uint32_t* w = nullptr;
  if constexpr (MASK) w = mask_words(mask, it.env);
  const bool sub = MASK && a.over;  // the normalisation runs over the sub-row (wave-uniform)
  for (int i = lane; i < nnorm; i += 64) {
    const float x = row[i];
    if constexpr (MASK) {
      const bool in = i < nsel && mask_allows(w, i), cnt = in || !sub;
      nan_here |= cnt && x != x;
      vmax = cnt ? fmaxf(vmax, x) : vmax;
      argmax_take(x, i, best, bi, in);
    } else {
      nan_here |= x != x;
      vmax = fmaxf(vmax, x);
      argmax_take(x, i, best, bi, i < nsel);
    }
  }
  wave_argmax(best, bi, &vmax);
  const bool has_nan = __any(nan_here);
  if (lane == 0) {
    if (a.tokens != nullptr) a.tokens[o] = bi;
    if (a.actions != nullptr) a.actions[o] = detokenise(bi, col.discrete, g);
  }
  if (a.logp == nullptr) return;

  // the target token (the same value on every lane)
  int tgt = -1;
  if (a.target_tokens != nullptr) {
    tgt = a.target_tokens[o];
  } else {
    const float x = a.target_actions[o];
    if (x - x == 0.f)  // finite
      tgt = col.discrete ? (int)x : tokenize_bin(x, head_bin_width(g), g.tok_min, g.action_channels) + g.n_discrete;
  }
  // (t > 0 and rounding is monotone: the maximum of t * x is t * max x)
  const double zmax = a.temperature * (double)vmax;
  double sum = 0.0;
  if constexpr (MASK) {
    for (int i = lane; i < nnorm; i += 64)
      if (!sub || mask_allows(w, i)) sum += exp(scaled_minus(a.temperature, row[i], zmax));
  } else {
    for (int i = lane; i < nnorm; i += 64) sum += exp(scaled_minus(a.temperature, row[i], zmax));
  }
  sum = wave_sum_f64(sum);
  if (lane == 0) {
    float lp;
    bool outside = tgt < 0 || tgt >= nnorm;
    if constexpr (MASK) outside = outside || (sub && !mask_allows(w, tgt));   // (read behind the range test: tgt is in 0 .. nnorm - 1)
    if (outside)
      lp = -INFINITY;
    else if (has_nan)
      lp = __builtin_nanf("");
    else
      lp = (float)(scaled_minus(a.temperature, row[tgt], zmax) - log(sum));
    a.logp[o] = lp;
  }
}

template <int PER>
__global__ __launch_bounds__(256) void action_score_kernel(ScoreArgs a) {
  __shared__ float stage[4][64 * (PER > 0 ? PER : 1)];
  score_row<PER, false>(a, score_item(a), stage);
}
// Its twin under allowed sets: a compile-time split, the kernel above is the code it was and takes the arguments it took.
template <int PER>
__global__ __launch_bounds__(256) void action_score_masked_kernel(ScoreArgs a, HeadMask mask) {
  __shared__ float stage[4][64 * (PER > 0 ? PER : 1)];
  score_row<PER, true>(a, score_item(a), stage, mask);
}

// Ragged score sink (lram_score_ragged): the row code above, the rows placed by score_item_ragged.
template <int PER>
__global__ __launch_bounds__(256) void action_score_ragged_kernel(ScoreArgs a) {
  __shared__ float stage[4][64 * (PER > 0 ? PER : 1)];
  score_row<PER, false>(a, score_item_ragged(a), stage);
}
template <int PER>
__global__ __launch_bounds__(256) void action_score_ragged_masked_kernel(ScoreArgs a, HeadMask mask) {
  __shared__ float stage[4][64 * (PER > 0 ? PER : 1)];
  score_row<PER, true>(a, score_item_ragged(a), stage, mask);
}

}  // namespace

void launch_action_score(const ScoreArgs& a, hipStream_t stream, const HeadMask& mask) {
  LRAM_REQUIRE(a.logits != nullptr && a.rows >= 1 && a.inner >= 1, "action score: bad rows");
  const HeadGeom& g = a.geom;
  LRAM_REQUIRE(g.act_dim >= 1 && g.n_vocab >= 1 && g.n_discrete >= 0 && g.n_discrete <= g.n_vocab && g.action_channels >= 1,
               "action score: bad head dimensions");
  LRAM_REQUIRE(!(a.discrete == 1 && a.slots.flags == nullptr && g.n_discrete < 1), "action score: a discrete head needs n_discrete >= 1");
  LRAM_REQUIRE(a.ld >= (int64_t)g.act_dim * g.n_vocab, "action score: ld must be >= act_dim * n_vocab");
  LRAM_REQUIRE((a.slots.flags == nullptr) == (a.slots.act == nullptr), "action score: the slot table's two arrays go together");
  LRAM_REQUIRE(a.over == 0 || a.over == 1, "action score: over must be 0 (the whole vocabulary) or 1 (the selectable range)");
  LRAM_REQUIRE(a.temperature > 0.0 && a.temperature < (double)INFINITY, "action score: temperature must be finite and > 0");
  LRAM_REQUIRE(a.target_actions == nullptr || a.target_tokens == nullptr,
               "action score: both target_actions and target_tokens are given (at most one)");
  LRAM_REQUIRE(a.logp == nullptr || a.target_actions != nullptr || a.target_tokens != nullptr,
               "action score: logp needs a target (target_actions or target_tokens)");
  LRAM_REQUIRE(a.actions != nullptr || a.tokens != nullptr || a.logp != nullptr || a.logits_out != nullptr,
               "action score: no output is given");
  const int64_t items = a.rows * a.geom.act_dim;
  LRAM_REQUIRE(items <= ((int64_t)1 << 32), "action score: rows * act_dim must be <= 2^32");
  const dim3 grid((unsigned)((items + 3) / 4)), block(256);
  LRAM_REQUIRE(mask.bits == nullptr || mask.words == (g.n_vocab + 31) / 32,
               "action score: the mask holds ceil(n_vocab / 32) words per env");
  auto launch = [&](auto per) {
    constexpr int P = decltype(per)::value;
    if (mask.bits != nullptr) {
      if (a.start != nullptr)
        hipLaunchKernelGGL(action_score_ragged_masked_kernel<P>, grid, block, 0, stream, a, mask);
      else
        hipLaunchKernelGGL(action_score_masked_kernel<P>, grid, block, 0, stream, a, mask);
    } else if (a.start != nullptr) {
      hipLaunchKernelGGL(action_score_ragged_kernel<P>, grid, block, 0, stream, a);
    } else {
      hipLaunchKernelGGL(action_score_kernel<P>, grid, block, 0, stream, a);
    }
  };
  if (a.geom.n_vocab > kSampleMaxRow)
    launch(std::integral_constant<int, 0>{});  // not staged: walked in global memory
  else
    with_per(a.geom.n_vocab, launch);
  LRAM_HIP_CHECK(hipGetLastError());
}

}  // namespace lram
