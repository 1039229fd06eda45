// Stored contexts of per-env length (lram_prefill_ragged / lram_score_ragged, and their append forms): the kernels that stand
// between the caller's left-aligned [B, L, ...] tensors and a call whose contexts are END-aligned -- env b's context of n_b
// timesteps occupies the call-timesteps start[b] = L - n_b .. L - 1.  No recurrent kernel knows about lengths: these kernels feed
// them zero tokens ahead of an env's context, build the per-chunk flags that restart an env at its first timestep (and, for the
// append entries, hold it until then), and put the head's outputs back at the left-aligned rows (the score sink's row arithmetic
// lives beside its dense twin, score_kernels.hip).
//
// Reference computation replaced: the padding + attention_mask handling of batches of unequal trajectories in the no-cache
// forward (src/algos/universal_decision_transformer_sb3.py:398-434) and the per-env context windows of the evaluation loop
// (src/algos/decision_transformer_sb3.py:628-666), here for a recurrent state.
//
// All four kernels move a few bytes per (env, timestep): one thread per 4 channels (float4) or per output element; the only
// branch, t < start[b], is taken per (env, timestep) row.
#include "common.h"

namespace lram {
namespace {

// embed_chunk_kernel (misc_kernels.hip) with a start per env: token rows 3j .. 3j + 2 of env b hold call-timestep t = t0 + j.
// From start[b] on they come from row t - start[b] of the env's own emb / rtg / rew; before it all three rows are zeros, so the
// padding is finite by construction (embed_ln turns a zero row into its bias) whatever the caller's buffers hold there.
__global__ __launch_bounds__(256) void embed_chunk_ragged_kernel(float* x, const float* emb, int64_t emb_stride, const float* rtg,
                                                                 const float* rew, int64_t in_stride, const int32_t* start, int t0,
                                                                 const float* w_rtg, const float* b_rtg, const float* w_rew,
                                                                 const float* b_rew, int B, int steps, int T, int D) {
  const int d4 = D >> 2;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)B * steps * d4) return;
  const int d = (int)(gid % d4) << 2;
  const int64_t bj = gid / d4;
  const int j = (int)(bj % steps), b = (int)(bj / steps);
  float* row = x + ((int64_t)b * T + 3 * j) * D + d;
  const int src = t0 + j - start[b];   // row of the env's own context; negative: padding
  if (src < 0) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(row) = z;
    *reinterpret_cast<float4*>(row + D) = z;
    *reinterpret_cast<float4*>(row + 2 * D) = z;
    return;
  }
  *reinterpret_cast<float4*>(row) = *reinterpret_cast<const float4*>(emb + (int64_t)b * emb_stride + (int64_t)src * D + d);
  const float g = rtg[b * in_stride + src], r = rew[b * in_stride + src];
  const float4 wg = *reinterpret_cast<const float4*>(w_rtg + d), bg = *reinterpret_cast<const float4*>(b_rtg + d);
  const float4 wr = *reinterpret_cast<const float4*>(w_rew + d), br = *reinterpret_cast<const float4*>(b_rew + d);
  *reinterpret_cast<float4*>(row + D) = make_float4(g * wg.x + bg.x, g * wg.y + bg.y, g * wg.z + bg.z, g * wg.w + bg.w);
  *reinterpret_cast<float4*>(row + 2 * D) = make_float4(r * wr.x + br.x, r * wr.y + br.y, r * wr.z + br.z, r * wr.w + br.w);
}

// The two flag rows of every chunk c, for every env b (s = start[b]).  mask[c][b]: the env restarts from an empty state at the
// chunk's start, which is its own first timestep -- where the caller's mask says so, and with `replace` (lram_prefill_ragged /
// lram_score_ragged) also wherever its context is shorter than the call.  hold[c][b]: the env has not started by the chunk; the
// append entries pass the row to the state kernels, which then write nothing of the env (device_math.h: env_held), s == L (no
// context) in every chunk.  A held env is never reset in the same chunk.
__global__ __launch_bounds__(256) void context_flags_kernel(uint8_t* hold, uint8_t* mask, const int32_t* start,
                                                            const int32_t* chunk_start, const uint8_t* reset, int replace,
                                                            int n_chunks, int B, int L) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)n_chunks * B) return;
  const int c = (int)(gid / B), b = (int)(gid - (int64_t)c * B);
  const int s = start[b], cs = chunk_start[c];
  hold[gid] = s > cs ? 1 : 0;
  mask[gid] = (s == cs && s < L && ((replace && s > 0) || (reset != nullptr && reset[b] != 0))) ? 1 : 0;
}

__global__ __launch_bounds__(256) void score_fill_ragged_kernel(float* actions, int32_t* tokens, float* logp, const int32_t* start,
                                                                int B, int L, int steps, int act_dim) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)B * steps * act_dim) return;
  const int j = (int)(gid % act_dim);
  const int64_t bt = gid / act_dim;
  const int t = (int)(bt % steps), b = (int)(bt / steps);
  const int row = L - start[b] + t;   // t < steps <= start[b]: inside the env's padded rows
  if (row < 0 || row >= L) return;
  const int64_t o = ((int64_t)b * L + row) * act_dim + j;
  if (logp != nullptr) logp[o] = 0.f;
  if (tokens != nullptr) tokens[o] = -1;
  if (actions != nullptr) actions[o] = 0.f;
}

__global__ __launch_bounds__(256) void action_fill_kept_kernel(float* actions, int32_t* tokens, const int32_t* start, int B, int L,
                                                               int act_dim) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= B * act_dim) return;
  if (start[gid / act_dim] < L) return;
  if (actions != nullptr) actions[gid] = 0.f;
  if (tokens != nullptr) tokens[gid] = -1;
}

}  // namespace

void launch_embed_chunk_ragged(float* x, const float* emb, int64_t emb_stride, const float* rtg, const float* rew, int64_t in_stride,
                               const int32_t* start, int t0, const float* w_rtg, const float* b_rtg, const float* w_rew,
                               const float* b_rew, int B, int steps, int T, int D, hipStream_t stream) {
  LRAM_REQUIRE(T >= 3 * steps && D % 4 == 0, "ragged embed: 3 token rows per timestep, d_model a multiple of 4");
  LRAM_REQUIRE(start != nullptr && t0 >= 0 && B >= 1 && steps >= 1, "ragged embed: bad argument");
  LRAM_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(emb)) & 15) == 0 && emb_stride % 4 == 0,
               "ragged embed: token rows and state embeddings must be 16-byte aligned");
  const int64_t n = (int64_t)B * steps * (D >> 2);
  hipLaunchKernelGGL(embed_chunk_ragged_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, emb, emb_stride, rtg,
                     rew, in_stride, start, t0, w_rtg, b_rtg, w_rew, b_rew, B, steps, T, D);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_context_flags(uint8_t* hold, uint8_t* mask, const int32_t* start, const int32_t* chunk_start, const uint8_t* reset,
                          bool replace, int n_chunks, int B, int L, hipStream_t stream) {
  LRAM_REQUIRE(hold && mask && start && chunk_start && n_chunks >= 1 && B >= 1 && L >= 1, "context flags: bad argument");
  const int64_t n = (int64_t)n_chunks * B;
  hipLaunchKernelGGL(context_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, hold, mask, start, chunk_start,
                     reset, replace ? 1 : 0, n_chunks, B, L);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_score_fill_ragged(float* actions, int32_t* tokens, float* logp, const int32_t* start, int B, int L, int steps,
                              int act_dim, hipStream_t stream) {
  if (steps <= 0 || (actions == nullptr && tokens == nullptr && logp == nullptr)) return;
  LRAM_REQUIRE(start != nullptr && steps <= L && B >= 1 && act_dim >= 1, "ragged score fill: bad argument");
  const int64_t n = (int64_t)B * steps * act_dim;
  hipLaunchKernelGGL(score_fill_ragged_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, actions, tokens, logp,
                     start, B, L, steps, act_dim);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_action_fill_kept(float* actions, int32_t* tokens, const int32_t* start, int B, int L, int act_dim, hipStream_t stream) {
  if (actions == nullptr && tokens == nullptr) return;
  LRAM_REQUIRE(start != nullptr && B >= 1 && act_dim >= 1, "kept action rows: bad argument");
  const int n = B * act_dim;
  hipLaunchKernelGGL(action_fill_kept_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, actions, tokens, start, B, L,
                     act_dim);
  LRAM_HIP_CHECK(hipGetLastError());
}

}  // namespace lram
