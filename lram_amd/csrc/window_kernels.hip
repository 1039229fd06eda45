// Context-window inference (lram_step_window): the kernels that keep every env slot's ring of its last K timesteps, lay the
// windows out for the stored-context entries and move whole windows between slots and records.  A ring entry is the state-token
// embedding (d_model floats, before embed_ln), the return-to-go and the reward of one timestep.  Every slot has its OWN ring
// position: pos[b] is where slot b's newest entry sits, and its entry of age a (0 = newest) sits at (pos[b] - a) mod K.  Only the
// slots a call runs push, so a parked slot's ring, position and count stay as they are.  How many entries count is per slot:
// n_b.  The host knows every position and every count and uploads both with the call; nothing is read back.
//
// Reference computation replaced: the per-env python lists of the cache-off evaluation loop and their slicing
// (src/callbacks/evaluation.py:130-251: append with reward 0, patch of the last reward, discount_cumsum of a finished episode,
// pruning to the last episodes; src/algos/decision_transformer_sb3.py:621-691: predict's [-context_len:] and pad_inputs).
//
// All kernels move bytes.  The step's three: window_push_rows and window_gather one thread per 4 channels (float4), window_update
// one thread per env (a relabel walks at most K entries of its own env sequentially -- the stated order of the suffix sum).  The
// only branches are per env (update) or per (env, timestep) row (gather).  No entry at an age >= n_b is ever read.  The movers:
// window_move copies or exchanges the raw ring rows of slot pairs (float4; the positions and counts travel on the host),
// window_save / window_load one thread per float of a position-free record (a record's pitch, K (d_model + 2) + 1 floats, is
// odd or even as K is: no float4).
#include "common.h"

namespace lram {
namespace {

// Per env b of the call's R rows, in this order: the reward patch of the newest entry, the relabel of the newest m_b entries' rtg
// with the suffix sum of their rewards (s = r_newest, then s = r_j + s towards older entries, fp32), then the scalars of the
// pushed entry.  pos[b] is where this call pushes (the newest entry once it has); the newest EXISTING entry sits one before it.
// patch[b] / relabel[b] come from the host, which knows every n_b: relabel[b] <= n_b, patch[b] != 0 only where n_b > 0 and the
// env is not reset.
__global__ __launch_bounds__(256) void window_update_kernel(float* ring_rtg, float* ring_rew, const float* prev_reward,
                                                            const float* rtg, const int32_t* patch, const int32_t* relabel,
                                                            const int32_t* pos, int R, int K) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= R) return;
  float* g = ring_rtg + (int64_t)b * K;
  float* r = ring_rew + (int64_t)b * K;
  const int head = pos[b], newest = head == 0 ? K - 1 : head - 1;
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

// The pushed embeddings: row b of emb [R, D] -> ring position pos[b] of env b.
__global__ __launch_bounds__(256) void window_push_rows_kernel(float* ring_emb, const float* emb, const int32_t* pos, int R, int K,
                                                               int d4) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)R * d4) return;
  const int c = (int)(gid % d4);
  const int64_t b = gid / d4;
  reinterpret_cast<float4*>(ring_emb)[(b * K + pos[b]) * d4 + c] = reinterpret_cast<const float4*>(emb)[gid];
}

// The windows, oldest to newest, into [R, K, D] / [R, K] / [R, K]: env b's n_b = count[b] entries occupy rows [K - n_b, K) (end-aligned)
// or rows [0, n_b) (`left`: what the entries of per-env length read).  The other rows take the pad entry (pad_emb, rtg 0, reward 0)
// or, without one, zeros.  pos[b]: ring position of env b's newest entry.  Each output is nullable.
__global__ __launch_bounds__(256) void window_gather_kernel(float* out_emb, float* out_rtg, float* out_rew, const float* ring_emb,
                                                            const float* ring_rtg, const float* ring_rew, const int32_t* count,
                                                            const int32_t* pos, const float* pad_emb, int left, int R, int K, int d4) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)R * K * d4) return;
  const int c = (int)(gid % d4);
  const int64_t row = gid / d4;
  const int t = (int)(row % K);
  const int64_t b = row / K;
  const int n = min(count[b], K);
  const int age = left ? n - 1 - t : K - 1 - t;   // of the entry that belongs at row t; outside 0 .. n - 1: no entry
  const bool real = age >= 0 && age < n;
  int p = pos[b] - age;
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

// Pair i of the lists: the K ring rows of slot dst[i] take those of slot src[i] as they lie (the position travels on the host);
// kSwap: and the other way round.  One thread per float4 of the embeddings; the first K threads of a pair also move the scalars.
// The host's list rules keep every destination apart from every other slot of the call.
template <bool kSwap>
__global__ __launch_bounds__(256) void window_move_kernel(float* ring_emb, float* ring_rtg, float* ring_rew, const int32_t* src,
                                                          const int32_t* dst, int n, int K, int d4) {
  const int64_t per = (int64_t)K * d4;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)n * per) return;
  const int i = (int)(gid / per);
  const int64_t j = gid % per;
  const int64_t a = src[i], b = dst[i];
  float4* e4 = reinterpret_cast<float4*>(ring_emb);
  const float4 va = e4[a * per + j];
  if (kSwap) e4[a * per + j] = e4[b * per + j];
  e4[b * per + j] = va;
  if (j < K) {
    const float ga = ring_rtg[a * K + j], ra = ring_rew[a * K + j];
    if (kSwap) ring_rtg[a * K + j] = ring_rtg[b * K + j], ring_rew[a * K + j] = ring_rew[b * K + j];
    ring_rtg[b * K + j] = ga, ring_rew[b * K + j] = ra;
  }
}

// Record i = the window of slot slots[i] as window_gather lays it out end-aligned without a pad entry -- [K, D] embeddings, [K]
// rtg, [K] rewards, zeros ahead of n_b -- and n_b as one trailing float.  One thread per float of the records.
__global__ __launch_bounds__(256) void window_save_kernel(float* records, const float* ring_emb, const float* ring_rtg,
                                                          const float* ring_rew, const int32_t* count, const int32_t* pos,
                                                          const int32_t* slots, int n, int K, int D) {
  const int64_t rec = (int64_t)K * (D + 2) + 1;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)n * rec) return;
  const int64_t j = gid % rec, b = slots[gid / rec];
  const int nb = min(count[b], K);
  if (j == rec - 1) {
    records[gid] = (float)nb;
    return;
  }
  const int64_t KD = (int64_t)K * D;
  const int t = j < KD ? (int)(j / D) : (int)((j - KD) % K);
  const int age = K - 1 - t;
  float v = 0.f;
  if (age < nb) {
    int p = pos[b] - age;
    if (p < 0) p += K;
    if (j < KD)
      v = ring_emb[(b * K + p) * D + j % D];
    else
      v = (j < KD + K ? ring_rtg : ring_rew)[b * K + p];
  }
  records[gid] = v;
}

// The inverse: record row t -> ring position t of slot slots[i], so the newest entry lands at K - 1 (the host sets the position
// and takes the count).  The trailing count is not the ring's to keep.
__global__ __launch_bounds__(256) void window_load_kernel(float* ring_emb, float* ring_rtg, float* ring_rew, const float* records,
                                                          const int32_t* slots, int n, int K, int D) {
  const int64_t rec = (int64_t)K * (D + 2) + 1;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)n * rec) return;
  const int64_t j = gid % rec, b = slots[gid / rec];
  if (j == rec - 1) return;
  const int64_t KD = (int64_t)K * D;
  if (j < KD)
    ring_emb[b * KD + j] = records[gid];
  else if (j < KD + K)
    ring_rtg[b * K + (j - KD)] = records[gid];
  else
    ring_rew[b * K + (j - KD - K)] = records[gid];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

unsigned blocks_of(int64_t n, const char* what) {
  LRAM_REQUIRE((n + 255) / 256 <= 0x7fffffff, std::string(what) + ": too many rows");
  return (unsigned)((n + 255) / 256);
}

}  // namespace

void launch_window_update(float* ring_rtg, float* ring_rew, const float* prev_reward, const float* rtg, const int32_t* patch,
                          const int32_t* relabel, const int32_t* pos, int R, int K, hipStream_t stream) {
  LRAM_REQUIRE(ring_rtg && ring_rew && prev_reward && rtg && patch && relabel && pos, "window update: null pointer");
  LRAM_REQUIRE(R >= 1 && K >= 1, "window update: bad argument");
  hipLaunchKernelGGL(window_update_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, stream, ring_rtg, ring_rew, prev_reward,
                     rtg, patch, relabel, pos, R, K);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_window_push_rows(float* ring_emb, const float* emb, const int32_t* pos, int R, int K, int D, hipStream_t stream) {
  LRAM_REQUIRE(ring_emb && emb && pos && R >= 1 && K >= 1 && D >= 4 && D % 4 == 0, "window push: bad argument");
  LRAM_REQUIRE(aligned16(ring_emb) && aligned16(emb), "window push: the embeddings must be 16-byte aligned");
  const int64_t n = (int64_t)R * (D >> 2);
  hipLaunchKernelGGL(window_push_rows_kernel, dim3(blocks_of(n, "window push")), dim3(256), 0, stream, ring_emb, emb, pos, R, K, D >> 2);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_window_gather(float* out_emb, float* out_rtg, float* out_rew, const float* ring_emb, const float* ring_rtg,
                          const float* ring_rew, const int32_t* count, const int32_t* pos, const float* pad_emb, bool left, int R,
                          int K, int D, hipStream_t stream) {
  if (out_emb == nullptr && out_rtg == nullptr && out_rew == nullptr) return;
  LRAM_REQUIRE(ring_emb && ring_rtg && ring_rew && count && pos, "window gather: null pointer");
  LRAM_REQUIRE(R >= 1 && K >= 1 && D >= 4 && D % 4 == 0, "window gather: bad argument");
  LRAM_REQUIRE(aligned16(out_emb) && aligned16(ring_emb) && aligned16(pad_emb), "window gather: the embeddings must be 16-byte aligned");
  const int64_t n = (int64_t)R * K * (D >> 2);
  hipLaunchKernelGGL(window_gather_kernel, dim3(blocks_of(n, "window gather")), dim3(256), 0, stream, out_emb, out_rtg, out_rew,
                     ring_emb, ring_rtg, ring_rew, count, pos, pad_emb, left ? 1 : 0, R, K, D >> 2);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_window_move(float* ring_emb, float* ring_rtg, float* ring_rew, const int32_t* src, const int32_t* dst, int n, bool swap,
                        int K, int D, hipStream_t stream) {
  LRAM_REQUIRE(ring_emb && ring_rtg && ring_rew && src && dst, "window move: null pointer");
  LRAM_REQUIRE(n >= 1 && K >= 1 && D >= 4 && D % 4 == 0 && aligned16(ring_emb), "window move: bad argument");
  const int64_t total = (int64_t)n * K * (D >> 2);
  const dim3 grid(blocks_of(total, "window move"));
  if (swap)
    hipLaunchKernelGGL(window_move_kernel<true>, grid, dim3(256), 0, stream, ring_emb, ring_rtg, ring_rew, src, dst, n, K, D >> 2);
  else
    hipLaunchKernelGGL(window_move_kernel<false>, grid, dim3(256), 0, stream, ring_emb, ring_rtg, ring_rew, src, dst, n, K, D >> 2);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_window_save(float* records, const float* ring_emb, const float* ring_rtg, const float* ring_rew, const int32_t* count,
                        const int32_t* pos, const int32_t* slots, int n, int K, int D, hipStream_t stream) {
  LRAM_REQUIRE(records && ring_emb && ring_rtg && ring_rew && count && pos && slots, "window save: null pointer");
  LRAM_REQUIRE(n >= 1 && K >= 1 && D >= 1, "window save: bad argument");
  const int64_t total = (int64_t)n * ((int64_t)K * (D + 2) + 1);
  hipLaunchKernelGGL(window_save_kernel, dim3(blocks_of(total, "window save")), dim3(256), 0, stream, records, ring_emb, ring_rtg,
                     ring_rew, count, pos, slots, n, K, D);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_window_load(float* ring_emb, float* ring_rtg, float* ring_rew, const float* records, const int32_t* slots, int n, int K,
                        int D, hipStream_t stream) {
  LRAM_REQUIRE(records && ring_emb && ring_rtg && ring_rew && slots, "window load: null pointer");
  LRAM_REQUIRE(n >= 1 && K >= 1 && D >= 1, "window load: bad argument");
  const int64_t total = (int64_t)n * ((int64_t)K * (D + 2) + 1);
  hipLaunchKernelGGL(window_load_kernel, dim3(blocks_of(total, "window load")), dim3(256), 0, stream, ring_emb, ring_rtg, ring_rew,
                     records, slots, n, K, D);
  LRAM_HIP_CHECK(hipGetLastError());
}

}  // namespace lram
