// Internal header of the engine's host files (engine*.hip): the engine object, the context of one call (Pass) and the host
// functions that cross a file.  Not part of the C ABI (include/lram_hip.h) and not of the kernel launch interface (common.h).
//
//   engine.hip          lifecycle: create / destroy, weights, finalize, workspace + state allocation, the mode setters
//   engine_gemm.hip     the GEMM dispatcher and the standalone lram_gemm_* entries            (calls kernels only)
//   engine_streams.hip  events, env slices, fork / join, the profiler                          (calls nothing)
//   engine_xlstm.hip    the xLSTM stack and the lazy matrix memory's host side                 (calls gemm, streams)
//   engine_mamba.hip    the Mamba stack                                                        (calls gemm, streams)
//   engine_image.hip    the IMPALA-CNN image front end, its buffers, the frame list                (calls gemm)
//   engine_head.hip     the action head, its refusals, the entries that run the head alone        (calls gemm)
//   engine_step.hip     token front end, the chunk loop, the env-step and encoder entries          (calls the stacks, image, head, gemm, streams)
//   engine_context.hip  stored contexts: the chunk plan, the one body of the eight entries         (calls step, image, head, state)
//   engine_window.hip   context-window inference: the per-slot ring, lram_step_window                (calls context, gemm)
//   engine_state.hip    reset, export / import, the slot table and the per-slot state calls
#pragma once
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lram_hip.h"
#include "common.h"

namespace lram::host {

struct DevBuf {
  float* p = nullptr;
  size_t n = 0;
  void alloc(size_t numel) {
    release();
    if (numel == 0) return;
    LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), numel * sizeof(float)));
    n = numel;
  }
  void zero(hipStream_t s = nullptr) {
    if (p) LRAM_HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(float), s));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

struct BlockWeights {  // resolved device pointers (nullptr when absent / optional)
  // common
  const float *norm_g = nullptr, *norm_b = nullptr;
  // mLSTM
  const float *proj_up = nullptr, *conv_w = nullptr, *conv_b = nullptr, *wq = nullptr, *wk = nullptr, *wv = nullptr,
              *wi = nullptr, *bi = nullptr, *wf = nullptr, *bf = nullptr, *on_g = nullptr, *on_b = nullptr,
              *skip = nullptr, *proj_down = nullptr;
  // sLSTM
  const float *gate_w[4] = {nullptr, nullptr, nullptr, nullptr};  // i, f, z, o slots of the cell
  const float *rt = nullptr, *rbias = nullptr, *gn_g = nullptr, *gn_b = nullptr, *ffn_norm_g = nullptr,
              *ffn_norm_b = nullptr, *ffn_up = nullptr, *ffn_down = nullptr;
  // Mamba
  const float *in_proj = nullptr, *in_proj_b = nullptr, *x_proj = nullptr, *dt_proj = nullptr, *dt_bias = nullptr,
              *A_log = nullptr, *Dp = nullptr, *out_proj = nullptr, *out_proj_b = nullptr;
};

struct BlockState {
  DevBuf s0;    // mLSTM C | sLSTM state [4,B,D] | Mamba ssm
  DevBuf n;     // mLSTM n
  DevBuf m;     // mLSTM m
  DevBuf conv;  // conv state
  // lazy matrix memory (mlstm_lazy.hip): window rows and ping-pong bookkeeping, allocated in lazy mode only
  DevBuf wk, wv;    // [B, NH, W, DH] each
  DevBuf coef;      // [2][B, NH, W]
  DevBuf gsc;       // [2][B, NH]
  DevBuf pw;        // [B, NH, 4, kLazyWT] window scores (head dims with several column slices per head only)
};

struct GraphKey {
  const void *obs, *rtg, *rew, *mask, *act, *tok;
  int emb, discrete, B;   // B: the rows of the captured step (the live prefix)
  hipStream_t stream;
  bool operator==(const GraphKey& o) const {
    return obs == o.obs && rtg == o.rtg && rew == o.rew && mask == o.mask && act == o.act && tok == o.tok &&
           emb == o.emb && discrete == o.discrete && B == o.B && stream == o.stream;
  }
};

}  // namespace lram::host

// (a private header of the engine*.hip host files only: they all speak in these names)
using namespace lram;
using namespace lram::host;

constexpr int kTokenTapMaxBatch = 1024;  // larger batches skip the per-step copy of the embed_ln tokens (lram_get_taps)

struct lram_engine {
  lram_config cfg{};
  int device = 0;
  std::map<std::string, DevBuf> weights;
  bool finalized = false;
  std::vector<BlockWeights> bw;
  // bf16x3 GEMM: fp32 weight pointer -> its three bf16 planes (built in finalize)
  struct Split {
    uint16_t* p;
    size_t n;
  };
  std::map<const float*, Split> split;
  GemmKnobs gemm_knobs;    // the projection launchers' knobs as the environment had them at lram_create: gemm() hands them to every launch
  bool use_bf16x3 = true;  // LRAM_GEMM=f32 selects the exact fp32-MFMA kernel everywhere
  // f16x2 projection kernel (gemm_f16x2.hip): un-batched weights also get two row-scaled f16 planes + inverse scales;
  // LRAM_GEMM=bf16x3 keeps the three-plane bf16 kernel for them too
  bool use_f16x2 = true;
  int f16x2_min_rows = 256;   // LRAM_F16_MIN_ROWS
  struct Split16 {
    uint16_t* planes;  // [2][rows][k] f16
    float* inv;        // [rows] exact inverse of each weight row's power-of-two scale
    size_t rows, k;
  };
  std::map<const float*, Split16> split16;
  bool gemm_presplit = true;   // LRAM_GEMM_PRESPLIT=0: the norms ahead of proj_up / in_proj write fp32 + row maxima (round 3) instead of
                               // the f16x2 GEMM's operand planes (gemm_f16x2p.hip)
  int64_t slstm_counts[3] = {0, 0, 0};  // sLSTM recurrence launches per form: token kernel, step kernel, recurrent GEMM + pointwise (lram_slstm_counts)
  double gemm_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // launches / fp32-equivalent FLOPs per dispatcher family (lram_gemm_counts)
  std::vector<DevBuf> slstm_rt2;  // sLSTM: recurrent weights re-packed per block for slstm_seq.hip: fp32 [head][k][channel][gate], or
                                  // (f16x2 projections, the default) two f16 planes in the same bytes + slstm_rinv, the inverse row scales
  std::vector<DevBuf> slstm_rinv;
  int lazy_cap2_envs = 896;       // LRAM_LAZY_CAP2_ENVS: largest slice whose read pass runs two workgroups per CU (0 = never)
  std::map<const float*, DevBuf> narrow;   // narrow-output weights (Mamba x_proj) packed for gemm_narrow.hip (built in finalize)
  bool gemm_narrow_on = true;     // LRAM_GEMM_NARROW=0: x_proj through the tile GEMMs (split-K + reduce) as before round 6
  int gemm_narrow_min_rows = 256;
  bool upz_beside = true;         // LRAM_UPZ_8P=0: proj_up's z half (issued beside the slice's own state pass) never through the 8-phase kernel
  bool slstm_gates_one = true;    // LRAM_SLSTM_GATES_ONE=0: the four sLSTM gate projections of larger slices as four bf16x3 launches
  bool gemm_narrow_f16 = true;    // LRAM_GEMM_NARROW=2: its exact-fp32 form even where the projections run as f16x2
  bool gn_amax_handover = true;   // LRAM_GN_AMAX=0: proj_down's operand row maxima from their own launch, not from the group norm
  bool gn_planes = true;          // LRAM_GN_AMAX=1: the group norm writes fp32 + partial row maxima (round 5) instead of proj_down's operand planes
  bool slstm_seq_f32 = false;     // LRAM_SLSTM_SEQ=2: its exact-fp32 form even where the projections run as f16x2
  bool slstm_seq = true;          // LRAM_SLSTM_SEQ=0: per-token recurrent GEMM + pointwise launches for slices beyond the token kernel's
  std::vector<DevBuf> gate_coef;  // mLSTM: folded i / f gate coefficients per block (mlstm_front.hip), geometries it covers
  bool front_multi = true;     // LRAM_FRONT_MULTI=0: keep the one-workgroup-per-env front end for large launches too
  int front_min_envs = 256;    // LRAM_FRONT_MIN_ENVS: slices of at least this many env slots take the multi-env front end
  int front_epw = 0;           // LRAM_FRONT_EPW: envs per workgroup of the multi-env front end (1 .. 64); 0 = by slice size
  std::vector<DevBuf> dt_wt;   // Mamba: dt_proj.weight transposed to [dt_rank, d_inner] per block (state-update kernel's operand)
  DevBuf ASCALE;  // per-row maxima of a GEMM's A operand computed by launch_row_amax, one region per stream slot (like
  size_t ascale_rows = 0;  // the split-K slabs)
  // row maxima handed over by the kernels that produce the projections' operands, indexed like the rows of X:
  // XN (norm -> proj_up / ffn_up / in_proj), XA (Mamba conv -> x_proj), H (Mamba selective state update -> out_proj)
  DevBuf AMX_XN, AMX_XA, AMX_H;
  // front end / head
  const float *w_state = nullptr, *b_state = nullptr, *w_rtg = nullptr, *b_rtg = nullptr, *w_rew = nullptr,
              *b_rew = nullptr, *eln_g = nullptr, *eln_b = nullptr, *w_head = nullptr, *b_head = nullptr,
              *post_g = nullptr, *post_b = nullptr;
  // IMPALA-CNN image front end (optional: present when the embed_image.* weights were uploaded)
  struct ImgConv {
    const float *w = nullptr, *b = nullptr;
    int cin = 0, cout = 0;
  };
  ImgConv img_conv[3][5];  // [stage][stage conv, res0.conv_0, res0.conv_1, res1.conv_0, res1.conv_1]
  const float *img_lin_w = nullptr, *img_lin_b = nullptr;
  int img_channels = 0, img_flat = 0;  // input channels, flattened feature count of the linear layer
  DevBuf IMG_P, IMG_X0, IMG_X1, IMG_T;
  DevBuf IMG_EMB;                      // [B, D] state-token embeddings of lram_step_images
  // Stored contexts from frames (lram_embed_frames, lram_prefill_frames, lram_score_frames): the frames that count go through the
  // conv stages in tiles of img_tile frames -- the four work buffers above then hold max(B, tile) frames, an env-step's regions
  // where they always were -- every tile's last map into its rows of IMG_FLAT [N, img_flat]; ONE Linear over all N rows into
  // IMG_ROWS [N, D] (the dispatcher picks its kernel by row count: per-tile launches would make the embeddings depend on the
  // tile), then ReLU + placement.  IMG_LIST: the {src, dst} pairs, int32 [N][2].  All grown outside the launches, as SEQ_EMB is.
  DevBuf IMG_FLAT, IMG_ROWS, IMG_LIST;
  // LRAM_IMG_TILE (capped per frame size: frame_tile() in engine_image.hip).  206M, 64 envs x 512 timesteps of 64 x 64 frames, one
  // job: the CNN's share of lram_prefill_frames at tiles of 128 / 256 / 512 / 1024 / 2048 frames 126.6 / 74.3 / 57.1 / 48.6 / 46.1 ms
  // (the whole call 350.7 ms at 2048, 0.74 % ahead of 1024; profiles/image_contexts.txt).  The buffers follow the list: a call of
  // fewer frames than the tile allocates for its own number.
  int img_tile = 2048;
  int64_t img_counts[3] = {0, 0, 0};   // frames convolved, tiles launched, Linear launches of those calls (lram_image_counts)
  // lram_step_images (Pass::images, the frames of the env-step under way): every env slice runs the IMPALA-CNN on
  // its own frames on its own stream, and the state-pass stream takes fold_bubbles_images folds ahead of the first read pass --
  // the VALU-bound CNN and the HBM-bound folds share the start of the step
  // (206M, 512 slots, same box: two calls 31.03k env-steps/s; one call with 2 / 5 / 8 / 11 / 14 folds ahead 31.36k / 31.68k / 31.81k /
  // 31.65k / 31.31k; the second slice's CNN held back until the first slice's is done: 31.4k -- not kept)
  static constexpr int fold_bubbles_images = 8;
  // Slot table (lram_set_slot_table): head mode, action dims in use and observation kind per env slot.  Host copy + device
  // copy; the ascending list of image slots (frame k belongs to slot_img_list[k]) and its prefix counts give every env slice
  // its contiguous range of frames.
  bool slot_table = false;
  std::vector<uint8_t> slot_flags, slot_act;   // host [B] each
  std::vector<int32_t> slot_img_prefix;        // host [B + 1]: image slots below slot b
  uint8_t* slot_dev = nullptr;                 // device [2][B]: flags, act_dim
  int32_t* slot_img_list = nullptr;            // device [n_image_slots]
  int slot_n_image = 0;
  bool slot_has_discrete = false;
  // Allowed-action sets (lram_set_action_mask): mask_words uint32 per env slot, bit t & 31 of word t >> 5 = token t may be
  // taken.  Host copy + device copy [B, mask_words]; they stay with the slot INDEX, as the slot table does.  Every head launch
  // passes head_mask(); without a mask that is {null, 0} and the launch is the unmasked kernel.  mask_no_discrete_at: the first
  // slot that allows nothing below n_discrete (-1: none) -- what a discrete = 1 call is refused on before anything is launched.
  int mask_words = 0;
  std::vector<uint32_t> mask_bits;
  uint32_t* mask_dev = nullptr;
  int mask_no_discrete_at = -1;
  // tokens of slot b's set below n (words of a [., words] table)
  static int mask_count_below(const uint32_t* bits, int words, int b, int n) {
    int cnt = 0;
    for (int k = 0; k < words && k * 32 < n; ++k) {
      const int left = n - k * 32;
      cnt += __builtin_popcount(bits[(size_t)b * words + k] & (left >= 32 ? 0xffffffffu : (1u << left) - 1u));
    }
    return cnt;
  }
  // The first slot whose sub-row would be empty under the table `flags` (null: no table, every range is [0, n_vocab)); -1: none.
  int mask_first_empty(const uint32_t* bits, int words, const uint8_t* flags) const {
    for (int b = 0; b < B; ++b) {
      const int n = (flags != nullptr && (flags[b] & 1)) ? cfg.n_discrete : cfg.n_vocab;
      if (mask_count_below(bits, words, b, n) == 0) return b;
    }
    return -1;
  }
  void drop_action_mask() {
    if (mask_dev) (void)hipFree(mask_dev);
    mask_dev = nullptr, mask_words = 0, mask_no_discrete_at = -1;
    mask_bits.clear();
  }
  // lazy matrix memory: C_base read once per step, rewritten once per `lazy_period` steps (see mlstm_lazy.hip)
  int lazy_mode = 2;        // 0 materialised, 1 lazy, 2 auto (LRAM_STATE / lram_set_state_mode)
  bool lazy = false;        // effective choice for the current batch (decided in state_alloc / set_state_mode)
  bool lazy_ready = false;  // buffers allocated for the current batch
  int lazy_period = 13;
  int gn_fuse = 2;          // LRAM_GN_FUSE: output group norm + skip in the read pass's epilogue, gate in proj_down's
                            // operand staging.  0 off, 1 on, 2 auto = on from 2048 env slots (round 3, same box, two
                            // rounds: 391.1k / 393.5k off vs 395.8k / 397.5k on at 4096 slots; 1024 slots: -0.4 %)
  bool mamba_dt_fuse = true;  // LRAM_MAMBA_DT_FUSE: dt_proj inside the selective-state-update kernel (d_state 16, dt_rank <= 64)
  int slstm_fused_rows = 512;  // LRAM_SLSTM_FUSED_ROWS: slices of slstm_fused_min .. this many envs (at sLSTM head dim <= 128; fewer above:
                               // x 128 / head dim) take the one-launch sLSTM token kernel (0 = never)
  int gemm_skinny_rows = 384;  // LRAM_GEMM_SKINNY_ROWS: GEMMs with 9 .. this many operand rows (half of it for weights above 600k elements) ...
  static constexpr int slstm_gates_rows = 768;  // sLSTM gate projections (head dim <= 128) of up to this many rows on the few-row kernel as well
  int gemm_skinny_min = 5;     // LRAM_GEMM_SKINNY_MIN: fewest operand rows (below: the GEMV path; 16M at 1 env 0.372 vs 0.410 ms, at 2 envs 0.443 vs 0.418)
  static constexpr int gemm_skinny_k = 1024;  // ... and K up to this take the few-row kernel
  static constexpr int fold_bubbles = 2;  // folds before the first read pass; the rest behind the sLSTM blocks, all on the state-pass
                                          // stream (measured on one box: k = 0 -- own stream, one block ahead -- 364k, 1 367k, 2 368k,
                                          // 3 367k, 4 366k env-steps/s).  Counts the folds this step still has to launch: the blocks
                                          // the step before folded in its tail (below) are not among them; re-measured with it there.
  // Tail fold (two env slices): the folds of the first fold_tail_blocks mLSTM blocks that belong to step n + 1 are launched at the
  // end of step n, behind the last read pass on the state-pass stream -- that stream has nothing else to run while the last
  // slice's proj_down, norm and head finish -- and step n + 1 skips those launches (run_xlstm_stack).  `prefold` remembers what
  // was folded early; every entry that is not the matching next step completes the fold first (lazy_finish_prefold).
  // (Same box, three interleaved runs each, env-steps/s at 4096 slots, fold_bubbles / fold_tail_blocks: without 470.9k; 2 / 1 472.3k,
  // 3 / 1 475.4k, 1 / 2 475.9k, 2 / 2 476.5k, 3 / 2 477.8k, 1 / 3 476.9k, 2 / 3 477.7k -- the box's own spread was 0.8 %; with the host
  // synchronising every step, where the tail folds sit inside the caller's latency: without 456.2k, 2 / 1 467.7k, 2 / 2 468.2k,
  // 2 / 3 463.3k.  A fold alone on the chip takes ~170 us, beside the sLSTM chains 220-320; from the third on the tail folds only
  // lengthen the step's end.  profiles/fold_tail_ab.txt)
  bool fold_tail = true;    // LRAM_FOLD_TAIL=0: every fold inside its own step
  static constexpr int fold_tail_blocks = 2;
  struct Prefold {
    bool pending = false;
    int blocks = 0;         // the first `blocks` mLSTM blocks are folded for the envs due at `step`
    int64_t step = 0;       // the lazy_step those folds belong to
    int period = 0, B = 0;
  } prefold;
  int64_t lazy_step = 0;    // steps taken in lazy mode: fold phase and ping-pong parity
  std::vector<int> lazy_bound;  // host-side upper bound of pending tokens per fold class (b % period)
  bool lazy_dirty = false;      // a lazy step ran since the last materialise: windows may hold pending tokens
  DevBuf LZ_COUNT;          // [2][B] int32 pending tokens per env
  // State of individual env slots (slot_state.hip; lram_state_copy_slots / save / load): one segment per contiguous per-env
  // piece of state, cut into chunks of kSlotChunk floats -- the record's segments first, then the lazy representation's.
  // Built by slot_segments_build (state_alloc, lazy_alloc); the state pointers never change in between.
  std::vector<SlotSeg> slot_segs;        // host copy
  SlotSeg* slot_segs_dev = nullptr;
  SlotChunk* slot_chunks_dev = nullptr;
  int slot_n_chunks = 0, slot_n_rec_chunks = 0;
  int32_t* slot_idx_dev = nullptr;       // device [2][B]: the index lists of the call under way (stream-ordered)
  std::vector<int64_t> slot_c_off;       // record offset of block i's matrix memory (-1: not an mLSTM block)
  bool slot_y_checked = false;           // some sLSTM block runs the f16x2 step form: a load range-checks its hidden planes
  void drop_slot_segments() {
    if (slot_segs_dev) (void)hipFree(slot_segs_dev);
    if (slot_chunks_dev) (void)hipFree(slot_chunks_dev);
    if (slot_idx_dev) (void)hipFree(slot_idx_dev);
    slot_segs_dev = nullptr, slot_chunks_dev = nullptr, slot_idx_dev = nullptr;
    slot_segs.clear(), slot_c_off.clear();
    slot_n_chunks = slot_n_rec_chunks = 0;
  }
  // state + workspace
  int B = 0;
  // Live prefix (lram_set_live): the stepping calls run on slots [0, n_live) only; slots [n_live, B) are parked -- they keep their
  // recurrent state and no activation row of them is computed (lazy mode: their bookkeeping is carried over, run_xlstm_stack).  B stays what every state tensor is allocated and strided for; n_live is what a
  // stepping call's rows, slices and size rules are judged on.  state_alloc sets n_live = B.
  int n_live = 0;
  // Which slots a stored-context or encoder call runs on (lram_set_context_rows): 0 every allocated slot (refused while slots are
  // parked), 1 the live prefix, 2 the live prefix and in every chunk only the envs that have started.  state_alloc sets 0.
  int ctx_rows = 0;
  // The rows such a call's inputs, outputs and size rules are judged on.  (Mode 0 with parked slots never gets to use it: refused.)
  int context_rows() const { return ctx_rows == 0 ? B : n_live; }
  int64_t ctx_counts[4] = {0, 0, 0, 0};   // stored-context calls, chunks, env-timesteps, records saved to KEEP (lram_context_counts)
  // Lazy matrix memory: the lazy_step at which a parked slot may last have come by pending window tokens -- the live count
  // changed, or a swap / copy moved a window.  A parked slot takes no token, so once every fold class has come due since then
  // (lazy_period steps) all parked windows are empty, and the steps launch no fold over the parked range until this moves again.
  int64_t parked_dirty_step = 0;
  bool parked_windows_empty(int64_t step) const { return step - parked_dirty_step >= (int64_t)lazy_period; }
  std::vector<BlockState> st;
  DevBuf X, XN, TOK, HID, U, Q, K, V, XA, H, G, SCAL, RY, LOGITS, RES, DTP;
  DevBuf XN2;   // the norm output as f16x2 operand planes [2][B*T, D] f16 (pre-split projections): its own buffer -- a slice inside an
                // sLSTM block uses XN as fp32 while another slice's mLSTM block holds planes
  DevBuf GATES, AMAT, VEC;           // chunkwise mLSTM prefill work buffers (allocated with the first long chunk)
  DevBuf SEQ_EMB;                    // state embeddings of a stored context [B, L, D] (lram_prefill)
  // Stored contexts of per-env length (the ragged and append entries): CTX holds, as bytes of one allocation, int32 start[B]
  // (call-timestep at which each env's context begins), int32 chunk_start[L], the per-chunk reset masks uint8[n_chunks, B] and
  // behind them the per-chunk hold flags uint8[n_chunks, B] (passed to the chunks of the append entries only); KEEP the state
  // records of the slots a replace call leaves alone (length 0), saved ahead of the first chunk and loaded back behind the last.
  // Both grown outside the launches, as SEQ_EMB is.
  DevBuf CTX, KEEP;
  // Context-window inference (engine_window.hip; lram_window_alloc / lram_step_window): every env slot's ring of its last win_K
  // timesteps -- WIN_RING_EMB [B, K, D] state-token embeddings, WIN_RING_SC [2][B, K] rtg | reward -- with a position per slot
  // (win_pos[b]: where slot b's newest entry sits; only the slots a call runs push) and the per-env counts, both on the host and
  // uploaded with every call that changes them.  WIN_EMB [B, K, D] and WIN_SC [2][B, K] are the laid-out windows a call hands to
  // the stored-context body (WIN_EMB's head also takes the state Linear's rows on their way into the ring); WIN_PAD [D] the pad
  // entry's embedding; WIN_CTL, as bytes of one allocation, int32 patch[B] | relabel[B] | count[B] | pos[B] (counts and positions
  // persist: lram_window_peek and the window movers read them) and uint8 ones[B], the reset mask that restarts every env.
  // win_K == 0: no ring.  win_own: LRAM_WINDOW_SLOTS_OWN -- a window step runs the live prefix (lram_window_set_slots).
  DevBuf WIN_RING_EMB, WIN_RING_SC, WIN_EMB, WIN_SC, WIN_PAD, WIN_CTL;
  int win_K = 0;
  bool win_pad_set = false, win_own = false;
  std::vector<int32_t> win_count;   // host [B], each in 0 .. win_K
  std::vector<int32_t> win_pos;     // host [B], each in 0 .. win_K - 1 (K - 1 in a fresh ring: the first push lands at 0)
  void drop_window() {
    for (DevBuf* b : {&WIN_RING_EMB, &WIN_RING_SC, &WIN_EMB, &WIN_SC, &WIN_PAD, &WIN_CTL}) b->release();
    win_K = 0, win_pad_set = false, win_own = false;
    win_count.clear(), win_pos.clear();
  }
  // lram_score: the head's logits for a block of (env, timestep) rows of one chunk, one region per chunk lane / env slice in
  // flight.  A region holds at most score_rows rows of act_dim * n_vocab floats (default 4096 rows: 34 MiB at 8 x 274 logits;
  // LRAM_SCORE_ROWS at lram_create, at least 16); a chunk with more rows goes through it block by block.
  DevBuf SCORE_LG;
  int score_rows = 4096;
  static constexpr int kScoreMinRows = 16;   // blocks keep clear of the GEMV path (rows <= 8): one kernel, one rounding per row
  int last_head = -1;                // `discrete` of the last action-producing call (its logits are in LOGITS); -1: none yet
  int tok_cap = 0;                   // tokens per env the activation workspace holds (kMaxTokens until a prefill grows it)
  bool chunk_prefill = true;         // LRAM_PREFILL_CHUNK=0: keep the token-sequential kernels for prefill
  bool chunk_exact_fp32 = false;     // LRAM_PREFILL_CHUNK=2: chunkwise cell on the fp32-input matrix cores (the round 1-5 form)
  // Chunk lanes of lram_prefill: consecutive chunks of a stored context alternate between two activation workspaces and two
  // streams; block i of chunk c + 1 waits for block i of chunk c only (its recurrent state), so two chunks are in flight one
  // block apart -- the matrix-core-bound projections of one beside the HBM-bound state passes of the other, and the
  // token-sequential sLSTM launches of either hidden behind both (one env slice only; LRAM_PREFILL_CHUNK=3: off).
  bool chunk_lanes = true;
  static constexpr int kMaxLanes = 3;
  static constexpr int n_lanes = 3;  // chunks in flight (206M, 64 envs x 512 timesteps, same box: 1 lane 385 ms, 2 lanes 326, 3 lanes 305, 4 lanes 303)
  DevBuf twin[kMaxLanes - 1][21];    // further copies of the per-token activation workspace (see workspace_set())
  std::vector<hipEvent_t> lane_ev[kMaxLanes];             // "block i of the lane's current chunk is done"
  DevBuf SK;                         // split-K partial slabs: one slot per stream that may run a GEMM
  static constexpr size_t kSplitKSlotElems = 6u << 20;  // 6 Mi floats (24 MiB) >= S*M*N for any GEMM the chooser splits
  static constexpr int kSplitKSlots = 9;                 // caller's stream + up to 8 micro-batch streams
  size_t ucols = 0, icols = 0;  // allocated row pitch of U and of Q/K/V/XA/H/G (slice offsets use these)
  // graph replay
  bool graph_mode = false;
  bool graph_valid = false;
  GraphKey graph_key{};
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  hipStream_t capture_stream = nullptr;  // capture needs a non-default stream; replay runs on the caller's
  // micro-batch pipeline: env slices on their own streams, cell kernels serialised on hbm_stream
  int n_micro = 0;  // 0 = auto
  // reference-trajectory modes of the Mamba agent (lram_set_compat_mode)
  int compat_repeat = 1;      // forwards per env-step: action dim i is read from forward min(i, repeat - 1)
  // Repeated forwards share what does not depend on the recurrent state: the (s, rtg, r) token embeddings, and with them
  // layer 0's add + RMSNorm and in_proj (identical inputs in every pass).  Pass 0 keeps them in X0 / U0; later passes skip
  // the front end and layer 0's first stage (Pass::compat_pass / compat_passes: the pass under way).
  DevBuf X0, U0;
  bool compat_share = true;   // LRAM_COMPAT_SHARE=0: every repeated forward recomputes the front end and layer 0's in_proj
  bool compat_stale = false;  // a reset re-initialises layer 0 only; layers >= 1 keep the previous episode's state
  // action head, sampling mode (lram_set_sampling): the settings travel as kernel arguments; the draw counter is device memory,
  // read by every head launch of an env-step and advanced once behind them (a replayed graph has frozen arguments)
  bool sampling = false;
  SampleArgs sample;             // .slot0 holds slot_base; a slice adds its first env slot
  uint64_t* sample_draw = nullptr;
  // per-slot settings (lram_set_sampling_slots): host copy + device table [B], used in place of sample's temperature / top_k /
  // top_p while set.  They stay with the slot INDEX, as the Philox stream does.  The maxima below are what the per-call top_k
  // check reads (refreshed when this table or the slot table changes): the largest top_k of a sampling slot, and of one the
  // slot table marks discrete, each with the slot that holds it.
  std::vector<SampleSlot> sample_slots;
  SampleSlot* sample_slots_dev = nullptr;
  int sslot_k_max = 0, sslot_k_at = -1, sslot_kd_max = 0, sslot_kd_at = -1;
  void sample_slot_maxima() {
    sslot_k_max = sslot_kd_max = 0, sslot_k_at = sslot_kd_at = -1;
    for (size_t b = 0; b < sample_slots.size(); ++b) {
      const SampleSlot& t = sample_slots[b];
      if (t.mode == 0) continue;
      if (t.top_k > sslot_k_max) sslot_k_max = t.top_k, sslot_k_at = (int)b;
      if (slot_table && b < slot_flags.size() && (slot_flags[b] & 1) && t.top_k > sslot_kd_max)
        sslot_kd_max = t.top_k, sslot_kd_at = (int)b;
    }
  }
  void drop_sample_slots() {
    if (sample_slots_dev) (void)hipFree(sample_slots_dev);
    sample_slots_dev = nullptr;
    sample_slots.clear();
    sample_slot_maxima();
  }
  static constexpr int cell_unroll = 16;  // C rows in flight per thread of the materialised cell kernel
  std::vector<hipStream_t> micro_streams;
  hipStream_t hbm_stream = nullptr;
  std::vector<hipEvent_t> sync_events, edge_events;   // engine-internal edges (device-scope fence) / fork + join with the caller's stream
  size_t sync_used = 0, edge_used = 0;
  bool event_device_scope = true;   // LRAM_EVENT_SCOPE=system: default (system-scope) events for the internal edges too
  // profiling of the dominant recurrent kernel
  bool prof_on = false;
  int prof_every = 1;       // lram_profile_begin_sampled: every n-th lram_step is timed (its launches carry the event pairs)
  int64_t prof_calls = 0;   // lram_step calls since profiling was armed
  bool prof_live = true;    // the call under way is one of the timed ones (set by prof_tick at every entry that launches the stack, and
                            // by the lram_profile_* entries outside any call: the one per-call value that stays in the engine)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  std::vector<uint8_t> prof_aux;  // 1: the pair times a fold launch (adds to the total, is not a state-pass launch)
  size_t prof_used = 0;

  ~lram_engine() {
    drop_graph();
    if (capture_stream) (void)hipStreamDestroy(capture_stream);
    if (hbm_stream) (void)hipStreamDestroy(hbm_stream);
    for (hipStream_t ms : micro_streams) (void)hipStreamDestroy(ms);
    for (hipEvent_t ev : sync_events) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : edge_events) (void)hipEventDestroy(ev);
    for (auto& v : lane_ev)
      for (hipEvent_t ev : v) (void)hipEventDestroy(ev);
    for (auto& e : prof_events) {
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
    for (auto& kv : weights) kv.second.release();
    drop_splits();
    release_state();
    if (sample_draw) (void)hipFree(sample_draw);
    drop_sample_slots();
    drop_slot_table();
    drop_action_mask();
  }
  void drop_slot_table() {
    if (slot_dev) (void)hipFree(slot_dev);
    if (slot_img_list) (void)hipFree(slot_img_list);
    slot_dev = nullptr, slot_img_list = nullptr;
    slot_flags.clear(), slot_act.clear(), slot_img_prefix.clear();
    slot_n_image = 0, slot_has_discrete = false, slot_table = false;
    sample_slot_maxima();
  }
  void drop_splits() {
    for (auto& kv : split) (void)hipFree(kv.second.p);
    split.clear();
    for (auto& kv : split16) (void)hipFree(kv.second.planes), (void)hipFree(kv.second.inv);
    split16.clear();
    for (DevBuf& b : dt_wt) b.release();
    dt_wt.clear();
    for (auto& kv : narrow) kv.second.release();
    narrow.clear();
    for (DevBuf& b : gate_coef) b.release();
    gate_coef.clear();
    for (DevBuf& b : slstm_rt2) b.release();
    slstm_rt2.clear();
    for (DevBuf& b : slstm_rinv) b.release();
    slstm_rinv.clear();
  }
  void drop_graph() {
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    if (graph) (void)hipGraphDestroy(graph);
    graph_exec = nullptr;
    graph = nullptr;
    graph_valid = false;
  }
  void release_state() {
    for (auto& s : st) {
      s.s0.release();
      s.n.release();
      s.m.release();
      s.conv.release();
      s.wk.release();
      s.wv.release();
      s.coef.release();
      s.gsc.release();
      s.pw.release();
    }
    LZ_COUNT.release();
    lazy_ready = false;
    prefold = Prefold{};
    drop_slot_segments();
    st.clear();
    for (DevBuf* b : {&X, &XN, &TOK, &HID, &U, &Q, &K, &V, &XA, &H, &G, &SCAL, &RY, &LOGITS, &RES, &DTP, &SK, &GATES,
                      &AMAT, &VEC, &SEQ_EMB, &IMG_EMB, &IMG_FLAT, &IMG_ROWS, &IMG_LIST, &IMG_P, &IMG_X0, &IMG_X1, &IMG_T, &XN2, &ASCALE, &AMX_XN, &AMX_XA, &AMX_H, &X0, &U0, &SCORE_LG, &CTX, &KEEP})
      b->release();
    for (auto& t : twin)
      for (DevBuf& b : t) b.release();
    drop_window();
    ascale_rows = 0;
    last_head = -1;
    B = 0;
    n_live = 0;
    tok_cap = 0;
  }
  int dh() const { return cfg.inner / cfg.n_heads; }
  int sdh() const { return cfg.d_model / cfg.n_heads; }
};

namespace lram::host {

// A contiguous range of env slots processed on its own stream.  All activation buffers are indexed by
// row b*T + t, so a slice simply works on rows [b0*T, (b0+nb)*T) of the shared buffers.
struct Slice {
  int b0, nb;
  hipStream_t s;
};

// What one call hands down to the kernels' launch sequence: built on the stack by the entry (step_launches, stored_context_call,
// lram_encoder_step) and passed by const& through run_stack -> run_*_stack -> the block functions.  Nothing of it outlives the call.
struct Pass {
  // what the caller handed in
  const uint8_t* images = nullptr;   // lram_step_images / lram_step_slots: the call's frames
  int img_c = 0, img_h = 0, img_w = 0;
  bool slots = false;                // mixed front end (lram_step_slots)
  bool context = false;              // a stored-context entry's call: its chunks and rows are counted (lram_context_counts)
  // repeated forwards of the Mamba reference-trajectory mode: the forward under way, how many there are, and whether they
  // share the token front end and layer 0's in_proj (compat_shares())
  int compat_pass = 0, compat_passes = 1;
  bool compat_shared = false;
  // chunk lanes of lram_prefill: "block i of the chunk before this one is done" / "block i of this chunk is done"
  const std::vector<hipEvent_t>* lane_wait = nullptr;
  const std::vector<hipEvent_t>* lane_rec = nullptr;
  int n_slices = 1;                  // env slices of the stack pass under way (set by run_stack)
  // hold flags of a stored-context chunk (lram_prefill_append / lram_score_append), engine-owned: device [B] or null, offset by a
  // slice's b0 as the reset mask is.  hold[b] != 0: env b takes no token in this pass -- no state-writing kernel writes a byte of
  // its recurrent state, and its reset flag is ignored.  Null (every other call): the kernels' instances without the rule.
  const uint8_t* hold = nullptr;
};

// Per-timestep sink of a stored context (lram_score): where the head's outputs of EVERY timestep go.  Tensors are [B, L, act_dim]
// (logits [B, L, act_dim * n_vocab], valid [B, L]); every output is nullable.
struct ScoreSink {
  float* actions = nullptr;
  int32_t* tokens = nullptr;
  float* logp = nullptr;
  float* logits = nullptr;
  const float* target_actions = nullptr;
  const int32_t* target_tokens = nullptr;
  const uint8_t* valid = nullptr;
  int over = 0;
  double temperature = 1.0;
};

// The (state, rtg, reward) inputs of a call: [B, L, .] / [B, L] row-major (L = 1: one env-step).
struct Inputs {
  const float* obs;
  int emb;   // obs holds state-token embeddings [., d_model] instead of observations [., state_dim]
  const float *rtg, *rew;
  int L;
  // stored contexts from frames (lram_prefill_frames / lram_score_frames): uint8 [n, L, C, H, W], n the image slots of the slot
  // table in ascending order (no table: every env).  obs is then the [B, L, state_dim] rows of a mixed table's vector slots, or null.
  const uint8_t* frames = nullptr;
  int img_c = 0, img_h = 0, img_w = 0;
};

// Stored contexts of per-env length (the ragged and append entries): the contexts are end-aligned inside the call, env b
// starting at call-timestep L - n_b, and the chunks are cut so that every env starts on a chunk boundary (context_plan in
// engine_context.hip).  An env restarts at its own first timestep where its row of that chunk's mask says so; in an append call an
// env that has not started by a chunk is held in it (Pass::hold).  Device pointers into lram_engine::CTX, filled on the call's
// stream ahead of the first chunk.
struct ContextPlan {
  std::vector<int> starts;        // ascending call-timesteps at which the chunks start; the last chunk ends at L
  // per chunk: some env is reset at its start / held in it (a chunk without one passes no pointer at all, as a dense call does)
  std::vector<char> has_reset, has_hold;
  // per chunk, LRAM_CONTEXT_ROWS_STARTED only (empty otherwise: every chunk runs all the call's rows): the chunk runs rows [0, rows[c])
  std::vector<int> rows;
  const int32_t* lengths = nullptr;                        // the caller's host array [B]
  const int32_t* dev_start = nullptr;                      // [B]
  const uint8_t *dev_masks = nullptr, *dev_hold = nullptr;   // [n_chunks, B] each
};

// One call of the (state, rtg, reward) front end, as its entry describes it: built on the entry's stack (an env-step: lram_step*;
// a stored context: the eight entries of engine_context.hip) and read by const& from the chunk loop down to the head.  Either
// `actions` / `tokens` take the action at the last timestep, or -- `scored` -- the sink takes the head's outputs at every timestep.
struct Call {
  const char* who;                   // the entry's name, in every message
  Inputs in;
  const uint8_t* reset = nullptr;    // device [rows] or null: who restarts before the first timestep
  int discrete = 0;                  // head mode: 0, 1 or LRAM_HEAD_PER_SLOT
  float* actions = nullptr;          // [rows, act_dim]; null in a stored context: no head at all (tokens is nullable on its own)
  int32_t* tokens = nullptr;
  bool scored = false;               // lram_score*: the head at every timestep into `sink`, nothing drawn
  ScoreSink sink;
  // stored contexts only
  bool from_frames = false;          // an entry from frames: in.frames must be given
  bool ragged = false;               // per-env lengths: host_lengths [rows] must be given (else every context has in.L timesteps)
  const int32_t* host_lengths = nullptr;
  int append = 0;                    // with lengths: 1 the contexts continue the slots' states, 0 they replace them
  const ContextPlan* plan = nullptr; // the chunk plan while a call of per-env lengths is under way (set by stored_context_call)
  const int32_t* ctx_start() const { return plan ? plan->dev_start : nullptr; }   // device [rows]: where every env's context begins
};

struct FrameCount {
  int n_env;
  int64_t frames;
};

extern thread_local std::string g_last_error;   // lram_last_error (defined in engine.hip)

// Makes every listed buffer hold at least its number of floats: synchronises the device -- once -- only when one has to grow, then
// runs `ahead` (what may still refuse the call) and allocates.  Never reached between a fork and a join.
template <typename Ahead>
void grow(std::initializer_list<std::pair<DevBuf*, size_t>> want, Ahead&& ahead) {
  bool synced = false;
  for (const auto& w : want) {
    if (w.first->n >= w.second) continue;
    if (!synced) {
      LRAM_HIP_CHECK(hipDeviceSynchronize());
      ahead();
      synced = true;
    }
    w.first->alloc(w.second);
  }
}
inline void grow(std::initializer_list<std::pair<DevBuf*, size_t>> want) { grow(want, [] {}); }
inline void grow(DevBuf& b, size_t n) { grow({{&b, n}}); }

// engine.hip
void alloc_workspace(lram_engine* e, int tokens);
void swap_workspace(lram_engine* e, int lane);
bool twin_ready(lram_engine* e);
int prefill_chunk_steps(lram_engine* e, int L);
// engine_gemm.hip
bool takes_skinny(const lram_engine* e, const GemmArgs& g);
bool takes_skinny_with_norm(const lram_engine* e, const GemmArgs& g);
bool f16x2_rows(const lram_engine* e, int rows, int n, int k);
bool f16x2_weight(const lram_engine* e, const float* w, int ldw, GemmArgs* g);
bool presplit_for(const lram_engine* e, const float* w, int rows, int n, int k);
bool narrow32_for(const lram_engine* e, const float* w, int rows, int n, int k);
int env_int(const char* name, int dflt);   // for lram_create and the standalone entries only: nothing on the step path reads the environment
GemmKnobs gemm_knobs_from_env();
void gemm(lram_engine* e, GemmArgs& g, hipStream_t s);
void make_split(lram_engine* e, const float* w, size_t n);
// engine_streams.hip
hipEvent_t new_event(const lram_engine* e, bool boundary);
void prof_record(lram_engine* e, hipStream_t s, bool start, bool aux = false);
void prof_tick(lram_engine* e);
hipEvent_t ring_event(lram_engine* e, bool boundary = false);
void stream_after(lram_engine* e, hipStream_t dst, hipStream_t src, bool boundary = false);
std::vector<Slice> make_slices(lram_engine* e, hipStream_t s, hipStream_t* hbm);
void fork_slices(lram_engine* e, const std::vector<Slice>& sl, hipStream_t hbm, hipStream_t s);
void join_slices(lram_engine* e, const std::vector<Slice>& sl, hipStream_t hbm, hipStream_t s);
// engine_state.hip
void slot_lists_check(const char* what, const int32_t* src, const int32_t* dst, int n, int B, bool unique_src);
void save_slot_records(lram_engine* e, const int32_t* host_slots, int n, float* dev_records, hipStream_t s);
void load_slot_records(lram_engine* e, const int32_t* host_slots, int n, const float* dev_records, hipStream_t s);
// engine_image.hip
void check_frame_size(const lram_engine* e, int C, int H, int W, const char* who);
void step_image_buffers(lram_engine* e, int C, int H, int W, const char* who);
void embed_images(lram_engine* e, const uint8_t* images, int C, int H, int W, float* out, hipStream_t s, int b0, int nb);
void check_frame_list(const lram_engine* e, int64_t N, const char* who);
void frame_list_buffers(lram_engine* e, int C, int H, int W, int64_t N, const char* who);
void embed_frame_list(lram_engine* e, const uint8_t* frames, int H, int W, int64_t N, float* out, hipStream_t s);
// engine_head.hip
void score_chunk(lram_engine* e, const Call& call, const Slice& x, float* scratch, int64_t cap, int l0, int Lc);
void action_head(lram_engine* e, const Pass& pass, const Call& call, const std::vector<Slice>& sl, int Tc, int last_steps);
void sample_draw_advance(lram_engine* e, hipStream_t s);
void check_head_mode(const lram_engine* e, int discrete, const char* who);
void check_score_sink(const lram_engine* e, const char* who, int discrete, const ScoreSink& k);
// engine_step.hip
bool compat_shares(const lram_engine* e, int discrete);
void step_entry(lram_engine* e, const char* who);
void require_all_live(const lram_engine* e, const char* who);
void timesteps_launches(lram_engine* e, const Pass& base, const Call& call, hipStream_t s);
// engine_context.hip
FrameCount count_frames(const lram_engine* e, int L, const int32_t* lengths);
void context_checks(lram_engine* e, Call& c);
void context_launches(lram_engine* e, Call c, hipStream_t s);
// engine_xlstm.hip, engine_mamba.hip
void lazy_materialize(lram_engine* e, hipStream_t s);
void lazy_finish_prefold(lram_engine* e, hipStream_t s);
void run_xlstm_stack(lram_engine* e, const Pass& pass, int T, const uint8_t* reset, const std::vector<Slice>& sl, hipStream_t hbm);
void run_mamba_stack(lram_engine* e, const Pass& pass, int T, const uint8_t* reset, const std::vector<Slice>& sl);

// One mLSTM block's matrix memory over the batch, in bytes: what the lazy / side-stream-fold / two-slice thresholds compare.
// (0 for a stack without an mLSTM block -- Mamba, or xLSTM with slstm_at = all: no threshold is met, and there is nothing to be lazy about.)
inline bool has_mlstm_block(const lram_engine* e) {
  if (e->cfg.backbone != LRAM_BACKBONE_XLSTM) return false;
  for (int i = 0; i < e->cfg.n_blocks; ++i)
    if (!e->cfg.block_is_slstm[i]) return true;
  return false;
}
inline double mlstm_block_bytes(const lram_engine* e) {
  if (!has_mlstm_block(e)) return 0.0;
  const double dh = (double)e->cfg.inner / e->cfg.n_heads;
  return (double)e->B * e->cfg.n_heads * dh * dh * 4.0;
}

// ... over the live prefix: what a stepping call's schedule (two slices or one, side-stream folds) is judged on
inline double mlstm_live_bytes(const lram_engine* e) {
  if (!has_mlstm_block(e)) return 0.0;
  const double dh = (double)e->cfg.inner / e->cfg.n_heads;
  return (double)e->n_live * e->cfg.n_heads * dh * dh * 4.0;
}

inline bool lazy_active(const lram_engine* e, int T) {
  return e->lazy && e->lazy_ready && !e->graph_mode && T >= 1 && T <= 4;
}

inline int stream_slot(const lram_engine* e, hipStream_t s) {  // split-K slab / row-maximum region of the stream a GEMM runs on
  for (size_t i = 0; i < e->micro_streams.size() && i + 1 < (size_t)lram_engine::kSplitKSlots; ++i)
    if (e->micro_streams[i] == s) return (int)i + 1;
  return 0;
}

inline void count_gemm(lram_engine* e, int family, const GemmArgs& g) {
  e->gemm_counts[family] += 1.0;
  e->gemm_counts[4 + family] += 2.0 * g.m * g.n * g.k * g.nb1 * g.nb2;
}

template <typename Fn>
int32_t guarded(Fn&& fn) {
  try {
    fn();
    g_last_error.clear();
    return 0;
  } catch (const std::exception& ex) {
    g_last_error = ex.what();
    return 1;
  } catch (...) {
    g_last_error = "lram: unknown error";
    return 1;
  }
}

}  // namespace lram::host
