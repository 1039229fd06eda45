// Context-window inference (lram_step_window): the kernels that keep every env slot's ring of its last K timesteps and lay the
// windows out for the stored-context entries.  A ring entry is the state-token embedding (d_model floats, before embed_ln), the
// return-to-go and the reward of one timestep.  Every env pushes exactly one entry per call, so ONE head index serves the batch:
// the entry of age a (0 = newest) of any env sits at ring position (newest - a) mod K.  How many of them count is per env: n_b.
//
// Reference computation replaced: the per-env python lists of the cache-off evaluation loop and their slicing
// (src/callbacks/evaluation.py:130-251: append with reward 0, patch of the last reward, discount_cumsum of a finished episode,
// pruning to the last episodes; src/algos/decision_transformer_sb3.py:621-691: predict's [-context_len:] and pad_inputs).
//
// All three kernels move bytes: window_push_rows and window_gather one thread per 4 channels (float4), window_update one thread
// per env (a relabel walks at most K entries of its own env sequentially -- the stated order of the suffix sum).  The only
// branches are per env (update) or per (env, timestep) row (gather).  No entry at an age >= n_b is ever read.
#include "common.h"

namespace lram {
namespace {

// Per env b, in this order: the reward patch of the newest entry, the relabel of the newest m_b entries' rtg with the suffix sum
// of their rewards (s = r_newest, then s = r_j + s towards older entries, fp32), then the scalars of the pushed entry at `head`.
// `newest` is the position of the newest existing entry, (head - 1) mod K.  patch[b] / relabel[b] come from the host, which
// knows every n_b: relabel[b] <= n_b, patch[b] != 0 only where n_b > 0 and the env is not reset.
__global__ __launch_bounds__(256) void window_update_kernel(float* ring_rtg, float* ring_rew, const float* prev_reward,
                                                            const float* rtg, const int32_t* patch, const int32_t* relabel,
                                                            int head, int newest, int B, int K) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float* g = ring_rtg + (int64_t)b * K;
  float* r = ring_rew + (int64_t)b * K;
  if (patch[b] != 0) r[newest] = prev_reward[b];
  const int m = min(relabel[b], K);
  float s = 0.f;
  for (int a = 0, p = newest; a < m; ++a) {
    s = a == 0 ? r[p] : r[p] + s;
    g[p] = s;
    p = p == 0 ? K - 1 : p - 1;
  }
  g[head] = rtg[b];
  r[head] = 0.f;
}

// The pushed embeddings: row b of emb [B, D] -> ring position `head` of env b.
__global__ __launch_bounds__(256) void window_push_rows_kernel(float* ring_emb, const float* emb, int head, int B, int K, int d4) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)B * d4) return;
  const int c = (int)(gid % d4);
  const int64_t b = gid / d4;
  reinterpret_cast<float4*>(ring_emb)[(b * K + head) * d4 + c] = reinterpret_cast<const float4*>(emb)[gid];
}

// The windows, oldest to newest, into [B, K, D] / [B, K] / [B, K]: env b's n_b = count[b] entries occupy rows [K - n_b, K) (end-aligned)
// or rows [0, n_b) (`left`: what the entries of per-env length read).  The other rows take the pad entry (pad_emb, rtg 0, reward 0)
// or, without one, zeros.  `newest`: ring position of the newest entry.  Each output is nullable.
__global__ __launch_bounds__(256) void window_gather_kernel(float* out_emb, float* out_rtg, float* out_rew, const float* ring_emb,
                                                            const float* ring_rtg, const float* ring_rew, const int32_t* count,
                                                            const float* pad_emb, int left, int newest, int B, int K, int d4) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)B * K * d4) return;
  const int c = (int)(gid % d4);
  const int64_t row = gid / d4;
  const int t = (int)(row % K);
  const int64_t b = row / K;
  const int n = min(count[b], K);
  const int age = left ? n - 1 - t : K - 1 - t;   // of the entry that belongs at row t; outside 0 .. n - 1: no entry
  const bool real = age >= 0 && age < n;
  int p = newest - age;
  if (p < 0) p += K;
  if (out_emb != nullptr) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (real)
      v = reinterpret_cast<const float4*>(ring_emb)[(b * K + p) * d4 + c];
    else if (pad_emb != nullptr)
      v = reinterpret_cast<const float4*>(pad_emb)[c];
    reinterpret_cast<float4*>(out_emb)[gid] = v;
  }
  if (c == 0) {
    if (out_rtg != nullptr) out_rtg[row] = real ? ring_rtg[b * K + p] : 0.f;
    if (out_rew != nullptr) out_rew[row] = real ? ring_rew[b * K + p] : 0.f;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void launch_window_update(float* ring_rtg, float* ring_rew, const float* prev_reward, const float* rtg, const int32_t* patch,
                          const int32_t* relabel, int head, int B, int K, hipStream_t stream) {
  LRAM_REQUIRE(ring_rtg && ring_rew && prev_reward && rtg && patch && relabel, "window update: null pointer");
  LRAM_REQUIRE(B >= 1 && K >= 1 && head >= 0 && head < K, "window update: bad argument");
  hipLaunchKernelGGL(window_update_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, ring_rtg, ring_rew, prev_reward,
                     rtg, patch, relabel, head, (head + K - 1) % K, B, K);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_window_push_rows(float* ring_emb, const float* emb, int head, int B, int K, int D, hipStream_t stream) {
  LRAM_REQUIRE(ring_emb && emb && B >= 1 && K >= 1 && head >= 0 && head < K && D >= 4 && D % 4 == 0, "window push: bad argument");
  LRAM_REQUIRE(aligned16(ring_emb) && aligned16(emb), "window push: the embeddings must be 16-byte aligned");
  const int64_t n = (int64_t)B * (D >> 2);
  hipLaunchKernelGGL(window_push_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ring_emb, emb, head, B, K, D >> 2);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_window_gather(float* out_emb, float* out_rtg, float* out_rew, const float* ring_emb, const float* ring_rtg,
                          const float* ring_rew, const int32_t* count, const float* pad_emb, bool left, int newest, int B, int K,
                          int D, hipStream_t stream) {
  if (out_emb == nullptr && out_rtg == nullptr && out_rew == nullptr) return;
  LRAM_REQUIRE(ring_emb && ring_rtg && ring_rew && count, "window gather: null pointer");
  LRAM_REQUIRE(B >= 1 && K >= 1 && newest >= 0 && newest < K && D >= 4 && D % 4 == 0, "window gather: bad argument");
  LRAM_REQUIRE(aligned16(out_emb) && aligned16(ring_emb) && aligned16(pad_emb), "window gather: the embeddings must be 16-byte aligned");
  const int64_t n = (int64_t)B * K * (D >> 2);
  LRAM_REQUIRE((n + 255) / 256 <= 0x7fffffff, "window gather: too many rows");
  hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out_emb, out_rtg, out_rew,
                     ring_emb, ring_rtg, ring_rew, count, pad_emb, left ? 1 : 0, newest, B, K, D >> 2);
  LRAM_HIP_CHECK(hipGetLastError());
}

}  // namespace lram
