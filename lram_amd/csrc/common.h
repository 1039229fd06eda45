// Shared declarations of the engine's HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <type_traits>

namespace lram {

// True the first time a call site sees the current HIP device: per-device one-time setup such as raising a kernel's
// dynamic-LDS limit (hipFuncSetAttribute applies to the current device only).  `mask` is the call site's static.
inline bool first_use_on_device(uint64_t& mask) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if (mask & bit) return false;
  mask |= bit;
  return true;
}

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define LRAM_HIP_CHECK(expr)                                                                         \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                            \
      throw ::lram::Error(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" + __FILE__ + \
                          ":" + std::to_string(__LINE__) + ")");                                     \
  } while (0)

#define LRAM_REQUIRE(cond, msg)                                   \
  do {                                                            \
    if (!(cond)) throw ::lram::Error(std::string("lram: ") + msg); \
  } while (0)

constexpr int kMaxTokens = 12;  // tokens per launch of the fused recurrent kernels: 3 per env-step, up to 4
                                // timesteps (12 tokens) per state pass when a stored context is prefilled
constexpr int kChunkMaxTokens = 64;  // tokens per state pass of the chunkwise (matrix-core) mLSTM prefill kernels

// Measurement knobs of the projection launchers (LRAM_GEMM_TILE / LRAM_F16P_STAGES / LRAM_GEMM_PANEL / LRAM_SPLITK_TILES).  They
// travel with the launch (GemmArgs::knobs): an engine reads them once, at lram_create, into lram_engine::gemm_knobs and
// host::gemm() copies them into every launch; a standalone test / micro-benchmark entry (lram_gemm_*) reads the environment
// when it is called -- that is how the bit-identity tests walk through tiles, stages and tile orders.  No launcher reads the
// environment, and a launch whose args were never given knobs runs with these defaults.
struct GemmKnobs {
  int tile = 0;          // 64 / 128: force the workgroup tile height of the f16x2 kernels; 256: the 8-phase 256 x 256 kernel; -1: never it
  int stages = 0;        // 1 / 2: force the LDS stage count of the pre-split kernel
  int panel = 0;         // > 0: force the column-panel tile order with that width
  int splitk_tiles = 56; // outputs with fewer 128 x 128 tiles than this are split along K
};

// ---------------------------------------------------------------------------------------------
// GEMM  C[M,N] = A[M,K] * W[N,K]^T  (fp32 in, fp32 MFMA accumulate), optional bias / residual.
// Two-level batching: z = z1 * nb2 + z2 ; pointer = base + z1 * s?1 + z2 * s?2.
// ---------------------------------------------------------------------------------------------
struct GemmArgs {
  const float* a = nullptr;
  const float* w = nullptr;
  float* c = nullptr;
  const float* bias = nullptr;  // [N] (per batch: bias + z1*sBias1 + z2*sBias2)
  const float* residual = nullptr;  // same layout as c (may alias c)
  int64_t lda = 0, ldw = 0, ldc = 0;
  int m = 0, n = 0, k = 0;
  int nb1 = 1, nb2 = 1;
  int64_t sA1 = 0, sA2 = 0, sW1 = 0, sW2 = 0, sC1 = 0, sC2 = 0, sBias1 = 0, sBias2 = 0;
  // optional: W pre-split into three bf16 planes (hi, mid, lo), each laid out like w, `w3_plane` elements apart
  const uint16_t* w3 = nullptr;
  int64_t w3_plane = 0;
  // optional (bf16x3 kernel, fp32 A, no batch, no split-K): A[r][k] is multiplied by gate[r * ldg + k] while it is staged
  // (the mLSTM output gate: gate holds silu(z), written by proj_up's epilogue via act_silu_from)
  const float* gate = nullptr;
  int64_t ldg = 0;
  // optional (bf16x3 kernel, no split-K): output columns >= act_silu_from are stored as silu(value); -1 = none
  int act_silu_from = -1;
  // optional (f16x2 kernel): W pre-split into two f16 planes (hi, lo) of the row-scaled weight, `w2_plane` elements apart,
  // K-TILE-MAJOR: element (n, k) of a plane lives at (k / 32) * w2_kt + n * 32 + k % 32, w2_kt = 32 x the rows of the whole
  // weight (K padded to a multiple of 32) -- the 128 rows x 32 columns a workgroup stages per K tile are ONE contiguous 8 KB run
  // instead of 128 pieces of 64 bytes at the row pitch (half cache lines: 1.4 x slower to deliver, scripts/tile_delivery.cpp);
  // with the exact inverse of each weight row's power-of-two scale; a_amax[r] = largest magnitude of A's row r (of the
  // gated row with `gate`), from which the kernel derives the row's power-of-two scale
  const uint16_t* w2 = nullptr;
  int64_t w2_plane = 0, w2_kt = 0;
  const float* w_inv = nullptr;
  const float* a_amax = nullptr;
  int amax_parts = 1;  // row r's maximum = max of a_amax[r * amax_parts + 0 .. amax_parts - 1]
  // optional (f16x2 kernel with pre-split operands, gemm_f16x2p.hip): A pre-split by its producer into two f16 planes (hi, lo)
  // of the row-scaled value, K-tile-major like w2 (element (r, k) at (k / 32) * a2_kt + r * 32 + k % 32), `a2_plane` elements
  // apart, with a2_inv[r] = the exact inverse of row r's power-of-two scale (`a` may then be null; K a multiple of 32)
  const uint16_t* a2 = nullptr;
  int64_t a2_plane = 0, a2_kt = 0;
  const float* a2_inv = nullptr;
  // optional split-K workspace (un-batched GEMMs with few output tiles: skinny N or small M): partial [S][M][N]
  // slabs are written by S x tiles workgroups and summed, in fixed order, by a second tiny kernel (deterministic)
  float* splitk_ws = nullptr;
  int64_t splitk_ws_elems = 0;
  // optional (few-row kernel, K <= 512): A is the UN-normalised input; every workgroup normalises its 32 rows in registers
  // before the products -- LayerNorm (x - mean) / sqrt(var + eps) * norm_g (+ norm_b), biased variance, two pass; RMSNorm
  // x * rsqrt(mean(x^2) + eps) * norm_g -- as row_norm_kernel does: no norm launch, no [rows, K] round trip
  // optional (few-row kernel; bf16x3 kernel with w3_tab): the outer batch index z2 (< nb2 <= 4) picks its operands from these tables instead of
  // a / w / c + z2 * stride -- several projections with unrelated base pointers in one launch (the four sLSTM gates)
  const float* a_tab[4] = {nullptr, nullptr, nullptr, nullptr};
  const float* w_tab[4] = {nullptr, nullptr, nullptr, nullptr};
  float* c_tab[4] = {nullptr, nullptr, nullptr, nullptr};
  // (bf16x3 kernel with a_tab / c_tab: the split planes of w_tab[z2], `w3_plane` elements apart like w3's)
  const uint16_t* w3_tab[4] = {nullptr, nullptr, nullptr, nullptr};
  const float* norm_g = nullptr;
  const float* norm_b = nullptr;
  float norm_eps = 0.f;
  int norm_rms = 0;
  // set by the launcher (gemm_choose_xcd_split): the 8 XCDs (each with its own 4 MB L2) take an xcd_gm x xcd_gn grid of
  // output blocks, xcd_gm * xcd_gn == 8; 0 = the one-dimensional map (each XCD a contiguous run of tiles, M-major)
  int xcd_gm = 0, xcd_gn = 0;
  // ... or (panel_w > 0) the panel order: the tile grid is cut into column panels of panel_w tiles, walked row by row (odd
  // panels bottom-up), and every XCD takes one contiguous eighth of that walk
  int panel_w = 0;
  // caller's hint (pre-split kernel): this projection runs BESIDE another env slice's memory-bound kernels -- where the launch is
  // 64 .. 160 tiles of 256 x 256 the 8-phase kernel (one workgroup per CU on part of the chip, half the L2 -> CU traffic) is slower
  // alone and faster for the step (Mamba-48M in_proj at 2048 slots: 65 vs 53 us alone, step +2.8 %: profiles/r06_ab_mamba_in_proj_8phase.txt)
  int beside_memory_bound = 0;
  int mfma_prio = 0;      // set by the launcher: raise the wave's issue priority around the MFMA block
  int split_k = 1;        // set by the launcher
  int k_tiles_per_split = 0;
  GemmKnobs knobs;        // host only (no kernel reads it): the launch policy's knobs, behind every field a kernel reads
};
int gemm_choose_split_k(GemmArgs& g);                             // fills split_k / k_tiles_per_split, returns S
// Output-tile -> XCD map of the 128-column-tile projection kernels (bm = their tile height, bytes_per_elem = operand bytes
// per element as staged: 4 for fp32 / two f16 planes).  Hardware hands consecutive workgroup ids to the 8 XCDs in turn, so
// workgroups b, b + 8, ... share an L2.  Every XCD streams its M band of A once and wants its N band of W resident in
// its 4 MB L2: the split (gm, gn) minimises M * gn + N * gm over the splits whose W band fits and that divide the tile grid.
void gemm_choose_xcd_split(GemmArgs& g, int bm, int bn, int bytes_per_elem);
// (the tile a workgroup id maps to under that split, device side: gemm_tile_of in gemm_tile.h)
// The GEMM kernels are templated on <HAS_BIAS, HAS_RES>: calls f(has_bias, has_res) with the launch's two as
// std::integral_constant<bool, ...> (a generic lambda names its instance with decltype(has_bias)::value).
template <typename F>
inline void launch_bias_res(const GemmArgs& g, F&& f) {
  const bool hb = g.bias != nullptr, hr = g.residual != nullptr;
  if (hb && hr) f(std::true_type{}, std::true_type{});
  else if (hb) f(std::true_type{}, std::false_type{});
  else if (hr) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}
void launch_splitk_reduce(const GemmArgs& g, hipStream_t stream);  // C = sum_s ws[s] (+ bias) (+ residual)
void launch_gemm_f32(const GemmArgs& g, hipStream_t stream);      // exact fp32 MFMA (k-ordered fma chain)
bool gemm_small_m(const GemmArgs& g);                             // M <= 8: launch_gemm_f32 takes the GEMV path
bool gemm_skinny_supported(const GemmArgs& g);                    // few-row kernel: 32 x 32 fp32 MFMA tile per workgroup, K over the waves
bool gemm_skinny_norm_supported(const GemmArgs& g);               // ... with the row norm of A in its prologue (K <= 512)
void launch_gemm_skinny(const GemmArgs& g, hipStream_t stream);
bool gemm_bf16x3_supported(const GemmArgs& g);
void launch_gemm_bf16x3(const GemmArgs& g, hipStream_t stream);   // fp32-accurate, 3 x bf16 split operands
void launch_split_bf16x3(const float* w, uint16_t* out, size_t n, hipStream_t stream);
bool gemm_f16x2_supported(const GemmArgs& g);
void launch_gemm_f16x2(const GemmArgs& g, hipStream_t stream);    // fp32-accurate, 2 x f16 split operands, row-scaled
bool gemm_f16x2p_supported(const GemmArgs& g);
void launch_gemm_f16x2p(const GemmArgs& g, hipStream_t stream);   // the same with A pre-split too: DMA staging, MFMA-only loop
int gemm_f16x2p_tile(const GemmArgs& g, int S);                   // tile height (64 / 128) of a launch of either, S = its K splits
// narrow-output projection (N <= 96, K a multiple of 64; gemm_narrow.hip): exact fp32 MFMA, 16 rows per workgroup, W packed at upload
bool gemm_narrow_shape(int n, int k);
bool gemm_narrow_supported(const GemmArgs& g);
size_t gemm_narrow_pack_elems(int n, int k);
void launch_gemm_narrow_pack(const float* w, int n, int k, float* packed, hipStream_t stream);
void launch_gemm_narrow(const GemmArgs& g, const float* packed, hipStream_t stream);
// ... as f16x2 split products (g.w2 / w_inv = the K-tile-major planes of the f16x2 tile GEMMs, g.a_amax / amax_parts = A's row maxima)
bool gemm_narrow16_supported(const GemmArgs& g);
void launch_gemm_narrow16(const GemmArgs& g, hipStream_t stream);
bool gemm_f16x2_8p_supported(const GemmArgs& g);
void launch_gemm_f16x2_8p(const GemmArgs& g, hipStream_t stream); // ... as 256 x 256 tiles, 8 staggered waves, counted DMA waits (gemm_f16x2_8p.hip)
// planes[0 / 1] (K-tile-major: (r, k) at (k / 32) * kt + r * 32 + k % 32; `plane` elements apart) = hi / lo of
// scale_r * a[r][k] (* gate[r][k]), inv[r] = 1 / scale_r
void launch_row_split_f16x2(const float* a, int64_t lda, const float* gate, int64_t ldg, int rows, int k, uint16_t* planes,
                            int64_t kt, int64_t plane, float* inv, hipStream_t stream);
// amax[r] = max_k |a[r][k] (* gate[r][k])|
void launch_row_amax(const float* a, int64_t lda, const float* gate, int64_t ldg, int rows, int k, float* amax,
                     hipStream_t stream);
// planes [2][K tiles][rows][32] f16 (hi, lo of the row-scaled weight, K-tile-major, split_f16x2_plane_elems(rows, k) each),
// inv[rows] = 1 / scale
inline size_t split_f16x2_plane_elems(size_t rows, size_t k) { return rows * ((k + 31) / 32 * 32); }
void launch_split_f16x2(const float* w, int rows, int k, uint16_t* planes, float* inv, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// normalisation / elementwise
// ---------------------------------------------------------------------------------------------
// out[r, :] = norm(in[r, :]) * gamma (+ beta);  rms != 0 -> RMSNorm (no mean subtraction).
// (out2: optional second copy of the result, same row stride as out)
// (amax: optional [rows] largest output magnitude per row, the f16x2 GEMM's a_amax)
// scalar tokens built inside the norm launch (token front end of one timestep): rows b * T + 1 / + 2 = Linear(1, D) of rtg[b] / rew[b]
struct ScalarTokens {
  const float *rtg = nullptr, *rew = nullptr, *w_rtg = nullptr, *b_rtg = nullptr, *w_rew = nullptr, *b_rew = nullptr;
  int64_t in_stride = 1;
  int T = 3;
};
// (h2: optional f16x2 operand planes (hi, lo) of the row-scaled result, K-tile-major with h2_kt elements per K tile, h2_plane
// elements apart, + h2_inv[rows] inverse row scales -- the pre-split projection kernel's A operand; out may then be null)
void launch_row_norm(const float* in, int64_t in_stride, float* out, int64_t out_stride, const float* gamma,
                     const float* beta, int rows, int d, float eps, int rms, hipStream_t stream, float* out2 = nullptr,
                     float* amax = nullptr, const ScalarTokens* st = nullptr, uint16_t* h2 = nullptr, int64_t h2_plane = 0,
                     float* h2_inv = nullptr, int64_t h2_kt = 0);
// Mamba block entry: res_out = hidden (+ res_in);  normed = RMSNorm(res_out) * gamma.
void launch_add_rms_norm(const float* hidden, const float* res_in, float* res_out, float* normed,
                         const float* gamma, int rows, int d, float eps, hipStream_t stream,
                         float* amax = nullptr,     // [rows] largest |normed| per row (f16x2 GEMM's a_amax)
                         uint16_t* h2 = nullptr, int64_t h2_plane = 0, float* h2_inv = nullptr, int64_t h2_kt = 0);

// ---------------------------------------------------------------------------------------------
// front end / head
// ---------------------------------------------------------------------------------------------
// x[b,1,:] = rtg[b]*w_rtg + b_rtg ; x[b,2,:] = rew[b]*w_rew + b_rew   (x: [B,T,D], tokens 1 and 2)
// rtg / rew of env b are read at index b * in_stride (in_stride = L when they come from a [B, L] sequence)
void launch_embed_scalars(float* x, const float* rtg, const float* rew, int64_t in_stride, const float* w_rtg,
                          const float* b_rtg, const float* w_rew, const float* b_rew, int B, int T, int D,
                          hipStream_t stream);
// copy caller-provided state embeddings [B,D] into token slot 0 of x [B,T,D]
void launch_scatter_token0(float* x, const float* emb, int64_t emb_stride, int B, int T, int D, hipStream_t stream);
// compact row k of emb [n, D] -> token row 0 of env slot slot[k] (slot numbers of the whole batch x [B, T, D])
void launch_scatter_token0_indexed(float* x, const float* emb, const int32_t* slot, int n, int B, int T, int D,
                                   hipStream_t stream);
void launch_embed_chunk(float* x, const float* emb, int64_t emb_stride, const float* rtg, const float* rew, int64_t in_stride,
                        const float* w_rtg, const float* b_rtg, const float* w_rew, const float* b_rew, int B, int steps, int T,
                        int D, hipStream_t stream);
// The action head's geometry and the slot table's two device arrays ([envs] + [envs]: head mode / action dims in use per env
// slot; both null: no table), passed by value to every head kernel (action_head.h holds the row rules they share).
struct HeadGeom {
  int act_dim = 0, n_vocab = 0, n_discrete = 0, action_channels = 0;
  float tok_min = -1.f, tok_max = 1.f;
};
struct HeadSlots {
  const uint8_t* flags = nullptr;
  const uint8_t* act = nullptr;
};
// The allowed-action sets (lram_set_action_mask), next to the slot table: `words` uint32 per env slot, bit t & 31 of word t >> 5
// = token t may be taken; entry 0 = the launch's first env slot.  bits null: no mask, and the launch is the code it was
// before masks (a compile-time split, as the sampling table's).
struct HeadMask {
  const uint32_t* bits = nullptr;
  int words = 0;
};
// argmax over logits [B, act_dim*n_vocab] (+ de-tokenise); columns col_begin .. col_end - 1 (sample_kernels.hip)
void launch_action_argmax(const float* logits, float* actions, int32_t* tokens, int B, const HeadGeom& g, const HeadSlots& s,
                          int discrete, int col_begin, int col_end, hipStream_t stream, const HeadMask& mask = {});
// The sampling mode of the same head (sample_kernels.hip): the token is drawn from the row instead of being its argmax.
constexpr int kSampleMaxRow = 512;  // logits per row the sampling kernels hold in registers (8 per lane)
struct SampleArgs {
  double temperature = 1.0;  // MULTIPLIES the logits, as the reference's sample_from_logits does
  double top_p = 0.0;        // quantile of the logit values below which logits are dropped; 0 = off
  int top_k = 0;             // 0 = off
  uint64_t seed = 0;         // Philox key
  uint64_t slot0 = 0;        // global index of logits row 0's env slot (counter word 0)
  const uint64_t* draw = nullptr;  // device: action-producing calls since sampling was armed (counter words 2, 3)
};
// Per-slot settings (lram_set_sampling_slots): one entry per env slot, read by the wave in place of SampleArgs' scalars.
struct SampleSlot {
  double temperature = 1.0;
  double top_p = 0.0;
  int32_t top_k = 0;
  int32_t mode = 1;  // 0: greedy (the argmax rule), 1: sample
};
// slots: nullable device table, entry 0 = the launch's first env slot; null: the launch is what it was before the table
void launch_action_sample(const float* logits, float* actions, int32_t* tokens, int B, const HeadGeom& g, const HeadSlots& s,
                          int discrete, int col_begin, int col_end, const SampleArgs& sp, const SampleSlot* slots,
                          hipStream_t stream, const HeadMask& mask = {});
// logp[B, act_dim] of tokens[B, act_dim] under the distribution launch_action_sample draws from (filters applied; sp.draw unused)
void launch_action_logp(const float* logits, const int32_t* tokens, float* logp, int B, const HeadGeom& g, const HeadSlots& s,
                        int discrete, const SampleArgs& sp, const SampleSlot* slots, hipStream_t stream,
                        const HeadMask& mask = {});
void launch_sample_advance(uint64_t* draw, hipStream_t stream);  // ++*draw, one thread
// rows of n logits at logits + r * ld (ld = 0: every row is row 0), one caller uniform per row -> tokens[rows]
void launch_sample_tokens(const float* logits, int64_t rows, int n, int64_t ld, double temperature, int top_k, double top_p,
                          const double* uniform, int32_t* tokens, hipStream_t stream);
// the same with per-row settings (device arrays [rows]); uniform + tokens_out: draw, tokens_in + logp_out: score (each pair nullable)
void launch_sample_rows(const float* logits, int64_t rows, int n, int64_t ld, const uint8_t* mode, const double* temperature,
                        const int32_t* top_k, const double* top_p, const double* uniform, const int32_t* tokens_in,
                        int32_t* tokens_out, float* logp_out, hipStream_t stream, const HeadMask& mask = {});  // mask: [rows, words]
// out[s * act_dim + j] = the uniform of env slot slot_base + s, action dim j, draw `draw`
void launch_sample_uniforms(uint64_t seed, uint64_t slot_base, int64_t n_slots, int act_dim, uint64_t draw, double* out,
                            hipStream_t stream);
// The scoring mode of the same head (score_kernels.hip): greedy token / action and the log-probability of a given target per
// (row, action dim).  A launch covers the flat rows g = row0 .. row0 + rows - 1 of a [envs, inner] grid (g = env * inner + step):
// row g's logits are at logits + (g - row0) * ld, its outputs, targets and `valid` byte at row
// (g / inner) * outer + off + g % inner of the caller's tensors, its slot-table entry at g / inner.
struct ScoreArgs {
  const float* logits = nullptr;
  int64_t ld = 0;
  int64_t row0 = 0, rows = 0;
  int64_t inner = 1, outer = 1, off = 0;
  HeadGeom geom;
  HeadSlots slots;           // slot table [envs] + [envs], nullable
  int discrete = 0;          // 0 / 1; with a slot table the slot's flag decides
  int over = 0;              // logp normalises over 0: all n_vocab logits, 1: the selectable range
  double temperature = 1.0;  // MULTIPLIES the logits
  const float* target_actions = nullptr;   // [., act_dim] float actions, tokenised on the device -- or
  const int32_t* target_tokens = nullptr;  // [., act_dim] tokens (at most one of the two)
  const uint8_t* valid = nullptr;          // [.] nullable: rows with 0 get the fill values
  float* actions = nullptr;                // outputs, each nullable: [., act_dim]
  int32_t* tokens = nullptr;
  float* logp = nullptr;
  float* logits_out = nullptr;             // [., act_dim * n_vocab]: the rows as they were read
  // Stored contexts of per-env length (lram_score_ragged), nullable: device [envs], the call-timestep at which env's context
  // starts (outer - its length).  Row g then stands for call-timestep t = off + g % inner of its env: from start[env] on its
  // outputs, targets and `valid` byte are at row env * outer + t - start[env] (the caller's tensors are left-aligned); before
  // it the row is padding and writes the fill values to row env * outer + (outer - start[env]) + t, so that the launches of a
  // call over t = 0 .. outer - 1 write every row of the tensors exactly once.
  const int32_t* start = nullptr;
};
// mask: allowed sets [envs, words], nullable: the greedy range and the over = 1 normalisation obey it.  It is an argument of the
// masked kernels alone, so that the launch without one passes the argument block it always passed.
void launch_action_score(const ScoreArgs& a, hipStream_t stream, const HeadMask& mask = {});

// Stored contexts of per-env length (context_kernels.hip; the ragged and append entries).  start[b] = L - n_b is the
// call-timestep at which env b's context begins inside a call of L timesteps (n_b = 0: start[b] = L, the slot only sees padding or is held).
// launch_embed_chunk with a start per env: the token rows of call-timesteps t0 .. t0 + steps - 1; env b's rows of timestep t come
// from row t - start[b] of its (left-aligned) emb / rtg / rew, rows with t < start[b] are zeros.
void launch_embed_chunk_ragged(float* x, const float* emb, int64_t emb_stride, const float* rtg, const float* rew, int64_t in_stride,
                               const int32_t* start, int t0, const float* w_rtg, const float* b_rtg, const float* w_rew,
                               const float* b_rew, int B, int steps, int T, int D, hipStream_t stream);
// The two flag rows of every chunk: mask[c][b] = 1 where env b starts at chunk c and restarts from an empty state -- where the
// caller's reset[b] (nullable) is set, and with `replace` (the ragged entries; not the append ones) whenever 0 < start[b];
// hold[c][b] = 1 where it has not started by chunk c (start[b] > chunk_start[c]: handed to the state kernels by the append
// entries, which then write nothing of it).
void launch_context_flags(uint8_t* hold, uint8_t* mask, const int32_t* start, const int32_t* chunk_start, const uint8_t* reset,
                          bool replace, int n_chunks, int B, int L, hipStream_t stream);
// fill values (logp 0, token -1, action 0) into the padded rows [b, L - start[b] + t], t = 0 .. steps - 1, of [B, L, act_dim]
// tensors (each nullable): the call-timesteps ahead of the first chunk, which no score launch covers
void launch_score_fill_ragged(float* actions, int32_t* tokens, float* logp, const int32_t* start, int B, int L, int steps,
                              int act_dim, hipStream_t stream);
// rows of slots without a context (start[b] == L): actions 0, tokens -1 (each nullable)
void launch_action_fill_kept(float* actions, int32_t* tokens, const int32_t* start, int B, int L, int act_dim, hipStream_t stream);

// Context-window inference (window_kernels.hip; lram_step_window).  Every env slot has a ring of K entries -- ring_emb [B, K, D],
// ring_rtg / ring_rew [B, K] -- and its own position: pos[b] (device [B]) is where slot b's newest entry sits, the entry of age a
// at (pos[b] - a) mod K.  The kernels of a step run the first R slots (the live prefix) and leave every other slot alone.
// Per env, in this order, with pos[b] the position this call pushes at: reward of the newest existing entry <- prev_reward[b]
// where patch[b]; rtg of the newest relabel[b] entries <- the fp32 suffix sum of their rewards, accumulated from the newest
// backwards; then (rtg[b], 0) into position pos[b].
void launch_window_update(float* ring_rtg, float* ring_rew, const float* prev_reward, const float* rtg, const int32_t* patch,
                          const int32_t* relabel, const int32_t* pos, int R, int K, hipStream_t stream);
// emb [R, D] into position pos[b] of every env's ring (float4 rows)
void launch_window_push_rows(float* ring_emb, const float* emb, const int32_t* pos, int R, int K, int D, hipStream_t stream);
// The windows oldest to newest into [R, K, D] / [R, K] / [R, K] (each nullable): env b's count[b] entries end-aligned, or with `left`
// in rows [0, count[b]); every other row takes (pad_emb, 0, 0), or zeros where pad_emb is null.  No entry beyond count[b] is read.
void launch_window_gather(float* out_emb, float* out_rtg, float* out_rew, const float* ring_emb, const float* ring_rtg,
                          const float* ring_rew, const int32_t* count, const int32_t* pos, const float* pad_emb, bool left, int R,
                          int K, int D, hipStream_t stream);
// Whole windows between slots, one launch: the raw ring rows of slot dst[i] <- those of slot src[i] (device lists [n]); `swap`: and
// back.  Positions and counts travel on the host.  Every destination is distinct from every other slot of the call.
void launch_window_move(float* ring_emb, float* ring_rtg, float* ring_rew, const int32_t* src, const int32_t* dst, int n, bool swap,
                        int K, int D, hipStream_t stream);
// Position-free records [n, K (D + 2) + 1]: the window of slot slots[i] end-aligned, oldest to newest, zeros ahead of count[b] --
// [K, D] embeddings | [K] rtg | [K] rewards | the count as a float.  Load writes record row t to ring position t (newest at K - 1)
// and leaves the count to the host.
void launch_window_save(float* records, const float* ring_emb, const float* ring_rtg, const float* ring_rew, const int32_t* count,
                        const int32_t* pos, const int32_t* slots, int n, int K, int D, hipStream_t stream);
void launch_window_load(float* ring_emb, float* ring_rtg, float* ring_rew, const float* records, const int32_t* slots, int n, int K,
                        int D, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// xLSTM
// ---------------------------------------------------------------------------------------------
struct MlstmPreArgs {
  const float* u;        // [B*T, 2*inner]  proj_up output: x_mlstm | z
  float* conv_state;     // [B, K, inner]   in/out
  float* n_state;        // [B, NH, DH]     in/out
  float* m_state;        // [B, NH]         in/out
  const float* conv_w;   // [inner, K]      (nn.Conv1d weight [inner,1,K])
  const float* conv_b;   // [inner]
  const float* wq;       // [inner/4, 4, 4]
  const float* wk;
  const float* wv;
  const float* wi;       // [NH, 3*inner]
  const float* bi;       // [NH]
  const float* wf;
  const float* bf;
  float* q;              // [B*T, inner] out
  float* k;
  float* v;
  float* xa;             // [B*T, inner] out  silu(conv)
  float* scal;           // [B*T, NH, 4] out  (f_t, i_t, denom_t, m_t)
  const uint8_t* reset;  // [B] or null
  int B, T, inner, NH, K;
  int lean = 0;          // 1: q, k, v are not written (the lazy read pass rebuilds them from xa / u); T <= 4 kernel only
  // chunkwise prefill (T > kMaxTokens) only, see mlstm_chunk.hip
  float* gates = nullptr;  // [B*T, NH, 2] out  raw (i~, f~) gate pre-activations
  float* amat = nullptr;   // [B, NH, 64, 64] out  intra-chunk weights A[t][s]
  float* vec = nullptr;    // [B, NH, 3, 64] out   fcum_t | w_s | denom_t
  const uint8_t* hold = nullptr;  // [B] or null: envs that take no token in this launch (no state byte written, reset ignored)
};
void launch_mlstm_pre(const MlstmPreArgs& a, hipStream_t stream);

// The same front end for large launches of the lazy ("lean") path, several env slots per workgroup with the block's
// weights held in registers (mlstm_front.hip): inner = 1024, 4 heads, 3 tokens.  q / k / v are not written.
struct MlstmFrontArgs {
  const float* u = nullptr;   // [B*T, ldu]  x_m half of proj_up's output
  int64_t ldu = 0;
  float* conv_state = nullptr;  // [B, 4, inner] in/out
  float* n_state = nullptr;     // [B, NH, DH]   in/out
  float* m_state = nullptr;     // [B, NH]       in/out
  const float *conv_w = nullptr, *conv_b = nullptr, *wq = nullptr, *wk = nullptr;
  const float* gc = nullptr;    // [inner/4, 4*NH, 4] folded gate coefficients (launch_gate_coef)
  const float *bi = nullptr, *bf = nullptr;
  float* xa = nullptr;          // [B*T, inner] out  silu(conv)
  float* scal = nullptr;        // [B*T, NH, 4] out  (f_t, i_t, denom_t, m_t)
  const uint8_t* reset = nullptr;
  int B = 0, T = 0, inner = 0, NH = 0, K = 0;
  int epw = 0;                  // env slots per workgroup (0 = by slice size; lram_engine::front_epw)
};
bool mlstm_front_supported(int inner, int NH, int K, int T);
void launch_mlstm_front(const MlstmFrontArgs& a, hipStream_t stream);
// gc[cg][j][c] (j < 2 NH: coefficient of xa[4 cg + c], else of x_m[4 cg + c]) for the i / f gates of every head
void launch_gate_coef(const float* wq, const float* wk, const float* wv, const float* wi, const float* wf, int inner, int NH,
                      float* gc, hipStream_t stream);
// chunkwise path: front end + gate scan / A matrix (two launches), then the cell contraction
bool mlstm_chunk_supported(int inner, int NH, int K);
void launch_mlstm_chunk_pre(const MlstmPreArgs& a, hipStream_t stream);

struct MlstmCellArgs {
  float* C;            // [B, NH, DH, DH] in/out
  const float* q;      // [B*T, inner]
  const float* k;
  const float* v;
  const float* scal;   // [B*T, NH, 4]
  float* h;            // [B*T, inner] out: (q^T C_t) / denom_t
  const uint8_t* reset;
  int B, T, NH, DH;
  int unroll = 8;         // rows in flight per thread (8 or 16)
  int min_lds_bytes = 0;  // > 0: request at least this much LDS per workgroup (occupancy cap, see launcher)
  const float* amat = nullptr;  // chunkwise prefill only (written by launch_mlstm_chunk_pre)
  const float* vec = nullptr;
  int chunk_exact_fp32 = 0;     // chunkwise cell on the fp32-input matrix cores (LRAM_CHUNK_CELL=0) instead of the bf16x3 form
  const uint8_t* hold = nullptr;  // [B] or null: envs that take no token in this launch (no state byte written, reset ignored)
};
void launch_mlstm_cell(const MlstmCellArgs& a, hipStream_t stream);
void launch_mlstm_chunk_cell(const MlstmCellArgs& a, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Lazy matrix memory (mlstm_lazy.hip): C_t = g * C_base + sum_j coef_j khat_j v_j^T.  A step reads C_base once
// and appends its tokens to a window; C_base is rewritten (folded) once every `period` steps per env.
// ---------------------------------------------------------------------------------------------
constexpr int kLazyWindow = 48;  // window capacity in tokens
constexpr int kLazyWT = kLazyWindow + 4;  // row pitch of the per-step window scores (LDS): window + this step's tokens
// The fold class that is due at `step` (or at a launch's phase): the smallest b with (step + b) % period == 0.
constexpr int lazy_due_class(int64_t step, int period) { return (period - (int)(step % period)) % period; }
struct MlstmLazyArgs {
  float* C;               // [B, NH, DH, DH] C_base (fold: in/out; cell: in)
  float* wk;              // [B, NH, W, DH] window khat_j = k_j / sqrt(DH)
  float* wv;              // [B, NH, W, DH] window v_j
  const float* coef_in;   // [B, NH, W]   coefficients at the start of this step
  float* coef_out;        // book: coefficients after this step
  const float* g_in;      // [B, NH]      scale of C_base at the start of this step
  float* g_out;
  const int32_t* count_in;  // [B] tokens pending at the start of this step (bit 16: C_base logically zero)
  int32_t* count_out;
  const float* q;         // [B*T, inner]
  const float* k;
  const float* v;
  const float* scal;      // [B*T, NH, 4] (f_t, i_t, denom_t, m_t) from mlstm_pre_kernel
  float* h;               // [B*T, inner] out
  // lean front end (fused-score geometries): q, k, v rebuilt here from xa (conv branch) and u's x half with the
  // block-diagonal 4 x 4 weights, instead of being read back from HBM
  const float *lean_xa = nullptr, *lean_u = nullptr, *lean_wq = nullptr, *lean_wk = nullptr, *lean_wv = nullptr;
  // output group norm + learnable skip in the read pass's epilogue (one column slice per head only): h is then stored as
  // GN(h) * gn_g (+ gn_b) + gn_skip * xa, the output gate silu(z) is applied by proj_down while it stages its operand
  const float *gn_g = nullptr, *gn_b = nullptr, *gn_skip = nullptr;
  float gn_eps = 0.f;
  float* pw = nullptr;    // [B, NH, T, kLazyWT] window scores: only for geometries with several column slices per head
  const uint8_t* reset;   // [B] or null
  int B, T, NH, DH;
  int phase, period;      // env b folds when (phase + b) % period == 0 (staggered), or when the window would overflow
  int force;              // fold kernel: fold every env that has pending tokens (materialise)
  int compact = 0;        // fold kernel: launch only over the envs whose phase comes up (no window can overflow); 2: the same grid
                          // over parked env slots, by mlstm_lazy_fold_parked_kernel (view first, then the tile of C_base)
  int first = 0;          // set by the launcher
  int min_lds_bytes = 0;
};
void launch_mlstm_lazy_fold(const MlstmLazyArgs& a, hipStream_t stream);
void launch_mlstm_lazy_cell(const MlstmLazyArgs& a, hipStream_t stream);
// one column slice per head (DH 128 / 256): the cell kernel computes the window scores and the bookkeeping itself;
// otherwise launch_mlstm_lazy_book must run before it (fills a.pw, coef_out, g_out, count_out)
bool mlstm_lazy_fused_scores(int DH);
void launch_mlstm_lazy_book(const MlstmLazyArgs& a, hipStream_t stream);
bool mlstm_lazy_supported(int DH, int T);
// count[b] = 0, g[b, :] = 1 for masked envs (mask == nullptr: all), both parities handled by the caller
void launch_mlstm_lazy_clear(int32_t* count, float* g, const uint8_t* mask, int B, int NH, hipStream_t stream);
// The envs b = first, first + period, ... with pending tokens have been folded in every block ahead of their step (the tail
// fold completed outside it, lazy_finish_prefold): g != nullptr: one block's g[b, :] = 1; g == nullptr: count[b] = 0 (pending
// tokens and the zero bit).  One launch per block first -- they read the counts -- then the launch that clears them.
void launch_mlstm_lazy_folded(int32_t* count, float* g, int B, int NH, int first, int period, hipStream_t stream);
// The step's bookkeeping for `a.B` env slots that take no token this step (parked slots; the pointers start at the first of them,
// a.reset is null): the "out" side <- the "in" side; count 0 and g = 1 for the envs whose fold runs this step.
void launch_mlstm_lazy_parked(const MlstmLazyArgs& a, hipStream_t stream);
void launch_lazy_counts_as_float(const int32_t* count, float* out, int B, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// State of individual env slots (slot_state.hip): copy slot -> slot, save slots -> records, load records -> slots, every block
// and tensor in ONE launch each, driven by a device-resident segment table (built by the engine in state_alloc / lazy_alloc).
// A segment is one contiguous per-env piece of state: env b's piece is `numel` floats at base + b * stride.
// ---------------------------------------------------------------------------------------------
constexpr int kSlotChunk = 4096;  // floats per workgroup: 256 lanes x 4 pieces of 16 bytes
enum SlotSegKind : int32_t {
  kSlotSegState = 0,   // part of the record
  kSlotSegC = 1,       // mLSTM matrix memory: part of the record; in lazy mode the stored tensor is C_base (save computes C)
  kSlotSegSlstmY = 2,  // sLSTM hidden plane: part of the record; range-checked by a load where the f16x2 step form runs
  kSlotSegWindow = 3,  // lazy: window rows wk / wv (copy only)
  kSlotSegCoef = 4,    // lazy: coefficients of one ping-pong parity (copy only)
  kSlotSegG = 5,       // lazy: scale g of one parity (copy; a load writes 1)
  kSlotSegCount = 6,   // lazy: count word of one parity (copy; a load writes 0)
};
struct SlotSeg {
  float* base;
  int64_t stride;    // floats between consecutive env slots
  int64_t rec_off;   // offset of the piece inside an env's record (floats); -1: not in the record
  int32_t numel;     // floats per env slot
  int32_t kind;      // SlotSegKind
  int32_t parity;    // -1: always live; 0 / 1: the lazy bookkeeping's ping-pong side (live when equal to the call's parity)
  int32_t vec;       // bit 0: slot side moves as 16-byte pieces; bit 1: record side too (else the scalar path)
};
struct SlotChunk {   // workgroup x of a launch: floats [off, off + kSlotChunk) of segment seg
  int32_t seg, off;
};
struct SlotStateArgs {
  const SlotSeg* segs = nullptr;
  const SlotChunk* chunks = nullptr;   // the record's segments first (n_rec_chunks), then the lazy representation's
  int n_segs = 0, n_chunks = 0;
  const int32_t* src = nullptr;        // device [n]: copy: source slots; save / load: the listed slots
  const int32_t* dst = nullptr;        // device [n]: copy: destination slots
  int n = 0;
  float* records = nullptr;            // save: out, load: in   [n, rec_numel]
  int64_t rec_numel = 0;
  int lazy = 0, parity = 0;            // lazy representation in effect; its live ping-pong side
  int rec_vec = 1;                     // 0: the record buffer is not 16-byte aligned: scalar path for the record side
};
void launch_slot_copy(const SlotStateArgs& a, hipStream_t stream);
void launch_slot_swap(const SlotStateArgs& a, hipStream_t stream);   // slot src[i] <-> slot dst[i]: all 2n indices distinct
void launch_slot_save(const SlotStateArgs& a, hipStream_t stream);
void launch_slot_load(const SlotStateArgs& a, hipStream_t stream);
// flag |= any listed record's sLSTM hidden plane (kSlotSegSlstmY segments) holds a value outside (-limit, limit), NaN included
void launch_slot_y_range(const SlotStateArgs& a, float limit, int* flag, hipStream_t stream);
// lazy save of one mLSTM block: record C = g C_base + sum_j coef_j khat_j v_j^T (plain fp32 FMAs), for the listed slots
struct SlotLazySaveArgs {
  const float *C = nullptr, *wk = nullptr, *wv = nullptr, *coef = nullptr, *g = nullptr;  // coef / g / count: the live side
  const int32_t* count = nullptr;
  const int32_t* slots = nullptr;
  int n = 0, NH = 0, DH = 0;
  float* records = nullptr;
  int64_t rec_numel = 0, rec_off = 0;
  int rec_vec = 1;   // 0: the tile's rows in the record are not 16-byte aligned: scalar stores
};
void launch_slot_lazy_save(const SlotLazySaveArgs& a, hipStream_t stream);

// mode 0 (mLSTM): out[r, hd] = (GN(h)[r,hd] * gamma + skip*xa) * silu(z)      z = u[r, inner + hd]
// mode 1 (sLSTM): x[r, hd] += GN(h)[r,hd] * gamma
struct GroupNormArgs {
  const float* h;      // [rows, NH*DH]
  const float* gamma;  // [NH*DH]  (already 1 + w)
  const float* beta;   // optional
  const float* skip;   // mode 0
  const float* xa;     // mode 0 [rows, NH*DH]
  const float* u;      // mode 0 [rows, 2*NH*DH]
  float* out;          // mode 0: g [rows, NH*DH]; mode 1: x [rows, NH*DH] (+=)
  int rows, NH, DH, mode;
  float eps;
  float* amax = nullptr;  // mode 0, optional: [rows, NH] max |out| of the (row, head) segment (partial row maxima for the f16x2 GEMM)  // mode 0, optional: the output as the pre-split f16x2 GEMM's A operand instead of fp32 -- two f16 planes, K-tile-major
  // [inner / 32][rows][32] with K-tile pitch h2_kt elements, the lo plane h2_plane elements after the hi plane, of the row scaled by
  // pow2_scale(row maximum over ALL heads); h2_inv[row] = the exact inverse scale.  One workgroup per row (NH waves).
  uint16_t* h2 = nullptr;
  int64_t h2_plane = 0, h2_kt = 0;
  float* h2_inv = nullptr;
};
void launch_group_norm(const GroupNormArgs& a, hipStream_t stream);

struct SlstmConvArgs {
  const float* xn;      // [B*T, D]
  float* conv_state;    // [B, K, D]
  float* slstm_state;   // [4, B, D]  (zeroed for reset envs)
  const float* conv_w;  // [D, K]
  const float* conv_b;
  float* xc;            // [B*T, D] out silu(conv)
  const uint8_t* reset;
  int B, T, D, K;
  int state_B;          // env count of the full state tensor (stride of its leading [4] axis)
  const uint8_t* hold = nullptr;  // [B] or null: envs that take no token in this launch (no state byte written, reset ignored)
};
void launch_slstm_conv(const SlstmConvArgs& a, hipStream_t stream);

struct SlstmPointwiseArgs {
  const float* gates;  // [B*T, 4, H] gate-major (i,f,z,o) input pre-activations (Wx)
  const float* ry;     // [B, 4, H]   recurrent contribution for this token
  const float* bias;   // [4, H]
  float* state;        // [4, B, H] in/out
  float* yout;         // [B*T, H]  y written at row b*T + t
  int B, T, t, H;
  int state_B;         // env count of the full state tensor
  const uint8_t* hold = nullptr;  // [B] or null: envs that take no token in this launch (no state byte written, reset ignored)
};
void launch_slstm_pointwise(const SlstmPointwiseArgs& a, hipStream_t stream);

// recurrent projection + pointwise cell of ONE token in one launch (few env rows; xlstm_kernels.hip)
struct SlstmTokenArgs {
  const float* gates;  // [B*T, 4, H] input pre-activations (Wx)
  const float* rt;     // [NH, 4, SDH, SDH] recurrent weights (out, in)
  const float* bias;   // [4, H]
  const float* hprev;  // h_{t-1}: row b at hprev + b * hprev_ld (the state's h plane, or yout rows of token t - 1)
  int64_t hprev_ld;
  float* state;        // [4, state_B, H] in/out (h plane written only when write_h)
  float* yout;         // [B*T, H]
  int B, T, t, H, NH, state_B, write_h;
  const uint8_t* hold = nullptr;  // [B] or null: envs that take no token in this launch (no state byte written, reset ignored)
};
bool slstm_token_supported(int H, int NH);
void launch_slstm_token(const SlstmTokenArgs& a, hipStream_t stream);

// recurrent projection + pointwise cell of ALL T tokens of an env-step in one launch (head dim 128, any slice size; slstm_seq.hip)
struct SlstmSeqArgs {
  const float* gates = nullptr;  // [B*T, 4, H] input pre-activations (Wx)
  const float* rt2 = nullptr;    // [NH, SDH (k), SDH (channel), 4 (gate)] recurrent weights re-packed by launch_slstm_pack_rt
  const uint16_t* rt2h = nullptr;  // != nullptr: the f16x2 form -- two f16 planes of the row-scaled weights (launch_slstm_pack_rt16)
  const float* rinv = nullptr;     // ... and [NH, 4, SDH] inverse scales
  const float* bias = nullptr;   // [4, H]
  float* state = nullptr;        // [4, state_B, H] in/out (h, c, n, m planes)
  float* yout = nullptr;         // [B*T, H]
  int B = 0, T = 0, H = 0, NH = 0, state_B = 0;
  const uint8_t* hold = nullptr;  // [B] or null: envs that take no token in this launch (no state byte written, reset ignored)
};
void launch_slstm_h_range(const float* h, int64_t n, float limit, int* flag, hipStream_t stream);  // flag |= any element outside (-limit, limit), NaN included
bool slstm_seq_supported(int H, int NH, int T);
void launch_slstm_seq(const SlstmSeqArgs& a, hipStream_t stream);
void launch_slstm_pack_rt(const float* rt, float* rt2, int NH, int SDH, hipStream_t stream);  // rt: [NH, 4, out, in]
void launch_slstm_pack_rt16(const float* rt, uint16_t* rt2h, float* rinv, int NH, int SDH, hipStream_t stream);

// a[r, f] = gelu(p[r, f]) * p[r, F + f]      p: [rows, 2F]
void launch_gelu_gate(const float* p, float* a, int rows, int F, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Mamba
// ---------------------------------------------------------------------------------------------
struct MambaConvArgs {
  const float* xz;      // [B*T, 2*d_inner]  in_proj output: x | z
  float* conv_state;    // [B, d_inner, K]
  const float* conv_w;  // [d_inner, K]
  const float* conv_b;
  float* xc;            // [B*T, d_inner] out silu(conv)
  const uint8_t* reset;
  int B, T, d_inner, K;
  float* amax = nullptr;  // optional [B*T][d_inner / 64]: per-wave partial row maxima of xc (f16x2 GEMM's a_amax)
  const uint8_t* hold = nullptr;  // [B] or null: envs that take no token in this launch (no state byte written, reset ignored)
};
void launch_mamba_conv(const MambaConvArgs& a, hipStream_t stream);

struct MambaSsmArgs {
  float* ssm_state;     // [B, d_inner, N]
  const float* xc;      // [B*T, d_inner]
  const float* dtp;     // [B*T, d_inner]  dt_proj(dt) (no bias)
  const float* dt_bias; // [d_inner]
  const float* xdb;     // [B*T, R + 2N]   x_proj output (dt | B | C)
  const float* A_log;   // [d_inner, N]
  const float* Dp;      // [d_inner]
  const float* xz;      // [B*T, 2*d_inner] (z at + d_inner)
  float* y;             // [B*T, d_inner] out
  const uint8_t* reset;
  int B, T, d_inner, N, R;
  float* amax = nullptr;    // optional [B*T][d_inner / 64]: per-64-channel partial row maxima of y (f16x2 GEMM's a_amax)
  const float* dt_wt = nullptr;  // optional dt_proj.weight TRANSPOSED [R, d_inner]: dt_proj evaluated inside the kernel, dtp unused
  const uint8_t* hold = nullptr;  // [B] or null: envs that take no token in this launch (no state byte written, reset ignored)
};
inline bool mamba_ssm_dt_fusable(int N, int R) { return N == 16 && R >= 1 && R <= 128; }
void launch_transpose_f32(const float* src, int rows, int cols, float* dst, hipStream_t stream);
void launch_mamba_ssm(const MambaSsmArgs& a, hipStream_t stream);
// dtp[rows, d_inner] = xdb[rows, :R] (row pitch ldx) * w[d_inner, R]^T in plain fp32: for dt_rank / row pitches no GEMM kernel takes
inline bool mamba_dt_proj_needs_plain_kernel(int N, int R) { return (R & 3) != 0 || ((R + 2 * N) & 3) != 0; }
void launch_mamba_dt_proj(const float* xdb, int ldx, const float* w, int R, float* dtp, int64_t rows, int di, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// IMPALA-CNN image front end (impala_cnn.hip)
// ---------------------------------------------------------------------------------------------
struct Conv3x3Args {
  const void* in;         // [B, CIN, H, W] float (or uint8 when in_u8: scaled by 1/255 while staging)
  const float* w;         // [COUT, CIN, 3, 3]
  const float* bias;      // [COUT]
  const float* residual;  // optional [B, COUT, H, W], added to the output
  float* out;             // [B, COUT, H, W]
  int B, CIN, COUT, H, W;
  int in_relu, out_relu, in_u8;
  const int32_t* src = nullptr;  // optional frame list ({src, dst} pairs): input frame k is in[src[2 * k]] (uint8 first conv only)
};
constexpr int kConvMaxFrames = 16384;   // frames per conv3x3 launch (grid.y), far below the 65535 a grid's y extent holds
void launch_conv3x3(const Conv3x3Args& a, hipStream_t stream);
void launch_maxpool3s2(const float* in, float* out, int64_t planes, int H, int W, hipStream_t stream);
void launch_relu(float* x, int64_t n, hipStream_t stream);
// Stored contexts from frames: the device table of {src, dst} pairs (one per frame that counts; n_env envs hand in frames of L
// timesteps each, env k being slot slots[k] -- null: k -- with its first L - start[b] timesteps -- null: all L), and the ReLU of
// the Linear's compact rows placed at their dst rows of `out`.
void launch_frame_list(int32_t* list, const int32_t* start, const int32_t* slots, int n_env, int L, hipStream_t stream);
void launch_relu_place_rows(const float* rows, const int32_t* list, float* out, int64_t N, int D, hipStream_t stream);

// misc
void launch_pad_obs(const float* native, int n_native, const int32_t* inv_index, const float* mean, const float* stdv,
                    float* out, int B, int state_dim, hipStream_t stream);
void launch_pad_obs_slots(const float* native, int n_native, const int32_t* slot_row, const int32_t* inv_index,
                          const float* mean, const float* stdv, int n_rows, float* out, int B, int state_dim,
                          hipStream_t stream);
void launch_stream_copy(float* dst, const float* src, size_t numel, hipStream_t stream, int variant);  // variant: 4 = the default
void launch_stream_read(const float* buf, size_t numel, float* sink, hipStream_t stream, int variant);  // read only; sink: 1024 floats; variant: 1804 = the default
void launch_stream_rmw(float* buf, size_t numel, hipStream_t stream);  // in place, the cell kernel's access pattern
void launch_zero_rows(float* buf, const uint8_t* mask, int B, int64_t row_elems, int64_t outer, int64_t outer_stride,
                      hipStream_t stream);

}  // namespace lram
