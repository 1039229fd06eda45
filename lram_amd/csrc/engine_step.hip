// One call from its inputs to its actions: the token front end, the block stack, the chunk loop that a stored context and an
// env-step share (timesteps_launches), repeated forwards, and the env-step and encoder entries (lram_step, lram_step_images,
// lram_step_slots, lram_encoder_step, lram_get_taps).
// Calls the stacks, the image front end, the head, gemm and the streams.
#include "engine.h"

namespace {

// ---------------------------------------------------------------------------------------------
// block stack on X [B*T, D] (in place residual stream) -> HID [B*T, D]
// ---------------------------------------------------------------------------------------------
void run_stack(lram_engine* e, Pass pass, int T, const uint8_t* reset, const std::vector<Slice>& sl, hipStream_t hbm) {
  pass.n_slices = (int)sl.size();
  if (e->cfg.backbone == LRAM_BACKBONE_MAMBA)
    run_mamba_stack(e, pass, T, reset, sl);
  else
    run_xlstm_stack(e, pass, T, reset, sl, hbm);
}

// Token front end of one env slice for the chunk of Lc timesteps that starts at timestep l: embeds the chunk's tokens into the
// slice's rows of X and applies embed_ln.  seq_emb: the state embeddings of a stored context, made ahead of the chunks
// (context_embeddings); null: an env-step, or a stored context that embeds its states timestep by timestep.
void embed_tokens(lram_engine* e, const Pass& pass, const Call& call, const float* seq_emb, const Slice& x, int l, int Lc) {
  const lram_config& c = e->cfg;
  const Inputs& in = call.in;
  const int D = c.d_model, T = c.tokens_per_step, Tc = T * Lc, L = in.L, emb = in.emb;
  const int64_t obs_w = emb ? D : c.state_dim;
  const float *obs = in.obs, *rtg = in.rtg, *rew = in.rew;
  const size_t r0 = (size_t)x.b0 * Tc, b0 = x.b0;
  float* X = e->X.p + r0 * D;
  if (call.plan != nullptr) {  // per-env lengths: every env's rows from its own (left-aligned) context, zeros ahead of it
    LRAM_REQUIRE(seq_emb != nullptr, "ragged context: no state embeddings");
    launch_embed_chunk_ragged(X, seq_emb + b0 * L * D, (int64_t)L * D, rtg + b0 * L, rew + b0 * L, L, call.plan->dev_start + b0, l,
                              e->w_rtg, e->b_rtg, e->w_rew, e->b_rew, x.nb, Lc, Tc, D, x.s);
    launch_row_norm(X, D, X, D, e->eln_g, e->eln_b, x.nb * Tc, D, 1e-5f, 0, x.s);
    return;
  }
  if (seq_emb != nullptr) {  // stored context: the chunk's token rows in one launch
    launch_embed_chunk(X, seq_emb + (b0 * L + l) * D, (int64_t)L * D, rtg + b0 * L + l, rew + b0 * L + l, L, e->w_rtg, e->b_rtg,
                       e->w_rew, e->b_rew, x.nb, Lc, Tc, D, x.s);
    launch_row_norm(X, D, X, D, e->eln_g, e->eln_b, x.nb * Tc, D, 1e-5f, 0, x.s);
    return;
  }
  // lram_step_slots: the slice's frames are the contiguous range [k0, k0 + nk) of the call's frames (frames come in slot
  // order); they go through the CNN into compact rows of IMG_EMB, every slice in its own region of the CNN work buffers
  const int k0 = pass.slots ? e->slot_img_prefix[b0] : 0;
  const int nk = pass.slots ? e->slot_img_prefix[b0 + x.nb] - k0 : 0;
  const size_t frame = (size_t)pass.img_c * pass.img_h * pass.img_w;
  if (pass.slots) {
    if (nk > 0)
      embed_images(e, pass.images + (size_t)k0 * frame, pass.img_c, pass.img_h, pass.img_w, e->IMG_EMB.p + (size_t)k0 * D, x.s, k0, nk);
  } else if (pass.images != nullptr)   // lram_step_images: this slice's frames -> its rows of `obs` (= IMG_EMB), on its own stream
    embed_images(e, pass.images + b0 * frame, pass.img_c, pass.img_h, pass.img_w, e->IMG_EMB.p + b0 * D, x.s, (int)b0, x.nb);
  for (int j = 0; j < Lc; ++j) {
    const float* o = obs + (b0 * L + l + j) * obs_w;
    float* Xj = X + (size_t)(T * j) * D;  // token slots 3j .. 3j+2 of every env row group
    if (pass.slots) {   // (L == 1) state Linear over the slice's rows, then the image slots' token 0 from the CNN rows
      if (nk < x.nb) {
        GemmArgs ge;
        ge.a = o, ge.lda = c.state_dim, ge.w = e->w_state, ge.ldw = c.state_dim, ge.c = Xj;
        ge.ldc = (int64_t)Tc * D, ge.bias = e->b_state, ge.m = x.nb, ge.n = D, ge.k = c.state_dim;
        gemm(e, ge, x.s);
      }
      launch_scatter_token0_indexed(e->X.p, e->IMG_EMB.p + (size_t)k0 * D, e->slot_img_list + k0, nk, e->B, Tc, D, x.s);
    } else if (emb) {
      launch_scatter_token0(Xj, o, (int64_t)L * D, x.nb, Tc, D, x.s);
    } else {
      GemmArgs ge;
      ge.a = o, ge.lda = (int64_t)L * c.state_dim, ge.w = e->w_state, ge.ldw = c.state_dim, ge.c = Xj;
      ge.ldc = (int64_t)Tc * D, ge.bias = e->b_state, ge.m = x.nb, ge.n = D, ge.k = c.state_dim;
      gemm(e, ge, x.s);
    }
    // (a single timestep per call: the scalar tokens are built by the embed_ln launch below)
    if (Lc > 1 || T != 3)
      launch_embed_scalars(Xj, rtg + b0 * L + l + j, rew + b0 * L + l + j, L, e->w_rtg, e->b_rtg, e->w_rew, e->b_rew,
                           x.nb, Tc, D, x.s);
  }
  // embed_ln in place; single env-steps of small batches also keep a copy for lram_get_taps (written by the same launch)
  ScalarTokens stok;
  const bool stok_on = Lc == 1 && T == 3;
  if (stok_on) {
    stok.rtg = rtg + b0 * L + l, stok.rew = rew + b0 * L + l, stok.in_stride = L, stok.T = T;
    stok.w_rtg = e->w_rtg, stok.b_rtg = e->b_rtg, stok.w_rew = e->w_rew, stok.b_rew = e->b_rew;
  }
  launch_row_norm(X, D, X, D, e->eln_g, e->eln_b, x.nb * Tc, D, 1e-5f, 0, x.s,
                  (L == 1 && e->B <= kTokenTapMaxBatch) ? e->TOK.p + r0 * D : nullptr, nullptr, stok_on ? &stok : nullptr);
}

// The state embeddings of ALL timesteps of a stored context, made on `s` ahead of the chunks (rows b * L + l, as the input lies)
// instead of one few-row GEMM per timestep (206M, 64 envs x 512 timesteps: 1024 launches of 12-26 us -> 1 + one per chunk).
// Three sources: the caller's own embeddings, the state Linear as one GEMM into SEQ_EMB, and the frames of a call from frames
// through the frame list.  Null: an env-step, a geometry or mode without this front end, or embeddings beyond 2 GiB -- the chunks
// then embed their states timestep by timestep (a call from frames has no other front end: its entry has refused what would not
// get here).  Grows SEQ_EMB and the frame-list buffers: called ahead of the fork.
const float* context_embeddings(lram_engine* e, const Pass& base, const Call& call, hipStream_t s) {
  const lram_config& c = e->cfg;
  const Inputs& in = call.in;
  const int D = c.d_model, L = in.L, R = e->context_rows();
  const float* seq_emb = nullptr;
  if ((L > 1 || call.plan != nullptr || in.frames != nullptr) && c.tokens_per_step == 3 && D % 4 == 0 && !base.compat_shared) {
    if (in.emb) {
      seq_emb = in.obs;
    } else if ((size_t)R * L * D <= ((size_t)1 << 29)) {   // <= 2 GiB
      const FrameCount fc = in.frames ? count_frames(e, L, call.plan ? call.plan->lengths : nullptr) : FrameCount{0, 0};
      if (fc.frames > 0) frame_list_buffers(e, in.img_c, in.img_h, in.img_w, fc.frames, "stored context from frames");
      grow(e->SEQ_EMB, (size_t)R * L * D);
      if (in.obs != nullptr) {   // (from frames: the vector slots of a mixed table; the image slots' rows are overwritten below)
        GemmArgs ge;
        ge.a = in.obs, ge.lda = c.state_dim, ge.w = e->w_state, ge.ldw = c.state_dim, ge.c = e->SEQ_EMB.p, ge.ldc = D;
        ge.bias = e->b_state, ge.m = R * L, ge.n = D, ge.k = c.state_dim;
        gemm(e, ge, s);
      }
      // Frames: the third source.  The list of the frames that count is built on the device from the per-env starts and the
      // slot table's image list; the CNN embeds exactly those into their rows b * L + l -- a padded frame is never read.
      if (fc.frames > 0) {   // (0: a mixed table whose image slots all have length 0)
        launch_frame_list(reinterpret_cast<int32_t*>(e->IMG_LIST.p), call.ctx_start(), e->slot_table ? e->slot_img_list : nullptr,
                          fc.n_env, L, s);
        embed_frame_list(e, in.frames, in.img_h, in.img_w, fc.frames, e->SEQ_EMB.p, s);
      }
      seq_emb = e->SEQ_EMB.p;
    }
  }
  LRAM_REQUIRE(in.frames == nullptr || seq_emb != nullptr, "stored context from frames: no state embeddings");
  return seq_emb;
}

// The chunks of a call.  Stored context is consumed in chunks: every block then reads and writes its recurrent state once per
// chunk instead of once per timestep.  Up to 4 timesteps (12 tokens) per chunk through the token-sequential kernels, up to 21
// (63 tokens) through the chunkwise matrix-core kernels (mlstm_chunk.hip).  With a plan (per-env lengths) the chunks are the
// plan's instead of the fixed `stride`.
// Chunk lanes (see lram_engine::chunk_lanes): the last chunk -- the one the action head reads -- is on lane 0 = the primary
// workspace and the caller's stream.  Where they apply they replace the automatic env slices of large batches as well: whole-batch
// launches, three chunks in flight (16M, 1024 envs x 252 timesteps: 224.4 -> 215.5 ms; 206M, 512 envs x 63: 295.3 -> 274.0 ms).
// (Mamba's stored contexts and the xLSTM geometries without a chunkwise form go through the token-sequential kernels in chunks
// of 4 timesteps: the lanes apply to them as they are.)
struct Chunks {
  std::vector<int> at;   // first timestep of every chunk, and L
  bool lanes;
  int n() const { return (int)at.size() - 1; }
};
Chunks call_chunks(lram_engine* e, const Pass& base, const Call& call, int stride) {
  const int L = call.in.L;
  Chunks ch;
  if (call.plan != nullptr)
    ch.at = call.plan->starts;
  else
    for (int l = 0; l < L; l += stride) ch.at.push_back(l);
  ch.at.push_back(L);
  ch.lanes = e->n_micro <= 1 && ch.n() >= 2 && e->chunk_lanes && !e->graph_mode && !base.compat_shared && twin_ready(e);
  return ch;
}

// Do the repeated forwards of the Mamba reference-trajectory mode share the token front end and layer 0's in_proj?  (below)
// ... then pass 0 keeps them in X0 / U0.  Called by lram_step BEFORE any stream capture begins: hipMalloc on a thread with
// an active capture fails with hipErrorStreamCaptureUnsupported and invalidates the capture (graph mode + repeated forwards).
void compat_prepare(lram_engine* e, int discrete) {
  if (e->B <= 0 || !compat_shares(e, discrete)) return;
  const size_t bt = (size_t)e->B * e->cfg.tokens_per_step;
  if (e->X0.n < bt * e->cfg.d_model) e->X0.alloc(bt * e->cfg.d_model);
  if (e->U0.n < bt * 2 * e->cfg.d_inner) e->U0.alloc(bt * 2 * e->cfg.d_inner);
}

void step_launches(lram_engine* e, Pass pass, const Call& call, hipStream_t s) {
  // compat_repeat (reference DiscreteDecisionMamba.get_action_pred, src/algos/decision_mamba.py:107-122): the same
  // (state, rtg, reward) tokens go through the stack once per action dim with the cache on, and action dim i is the
  // prediction of forward i.  Forward p writes action columns >= p, so column i keeps forward min(i, repeat - 1).
  pass.compat_passes = call.discrete ? 1 : std::max(1, std::min(e->compat_repeat, e->cfg.act_dim));
  pass.compat_shared = compat_shares(e, call.discrete);
  if (pass.compat_shared) {  // (allocated by compat_prepare ahead of this call: never inside a stream capture)
    const size_t bt = (size_t)e->n_live * e->cfg.tokens_per_step;   // (the rows of this call; compat_prepare allocates for the batch)
    LRAM_REQUIRE(e->X0.n >= bt * e->cfg.d_model && e->U0.n >= bt * 2 * e->cfg.d_inner,
                 "shared repeated forwards: workspace not prepared");
  }
  // every forward runs on the same slice streams: a slice's forward p + 1 follows its forward p in stream order (state, X0 / U0,
  // logits are per slice), so the slices are forked once and joined once instead of draining the two-slice pipeline per forward
  // (Mamba-48M at 2048 slots, 4 forwards per env-step, same box: 140.35k -> 141.0k env-steps/s)
  for (pass.compat_pass = 0; pass.compat_pass < pass.compat_passes; ++pass.compat_pass) timesteps_launches(e, pass, call, s);
  sample_draw_advance(e, s);
}

}  // namespace

namespace lram::host {

// L consecutive timesteps for every env slot (L = 1: one env-step).  The reset mask applies before the first timestep (of
// repeated forwards: of the first); the action head runs on the last timestep only (and only if an output buffer is given).
// One fork / join of the slice streams brackets the whole call -- of repeated forwards (base.compat_passes > 1): one fork ahead of
// the first, one join behind the last.
// A scored call (lram_score; `actions` is then null) has the head run at every timestep: after the stack pass of every chunk, on
// that chunk's stream and workspace (score_chunk), and once more on the last timestep through the very launches a call without
// a sink makes for it (action_head) -- row [b, L - 1] of the sink is what lram_prefill computes, and LOGITS is left as it leaves it.
// With a plan (per-env lengths) chunk c takes row c of the plan's reset masks instead of `reset` on the first chunk, and the front
// end and the sink place every env's rows by its own start.
// The rows of a stored context are R = lram_engine::context_rows() -- the batch, or the live prefix (lram_set_context_rows); an
// env-step's are the slices' (make_slices: the live prefix).  A plan with per-chunk rows clips every chunk's slices to them.
void timesteps_launches(lram_engine* e, const Pass& base, const Call& call, hipStream_t s) {
  const lram_config& c = e->cfg;
  const ContextPlan* plan = call.plan;
  const int T = c.tokens_per_step, L = call.in.L, R = e->context_rows();
  const bool score_chunks = call.scored && L > 1;   // (a one-timestep call has its only timestep scored by action_head)
  e->sync_used = 0, e->edge_used = 0;
  const int stride = L > 1 ? prefill_chunk_steps(e, L) : 1;   // (grows the workspace on first use: ahead of everything else)
  if (L > 1 || !lazy_active(e, T)) lazy_materialize(e, s);  // stored contexts go through the materialised kernels
  const float* seq_emb = context_embeddings(e, base, call, s);
  const Chunks ch = call_chunks(e, base, call, stride);
  const int n_chunks = ch.n();
  const bool lanes = ch.lanes;
  hipStream_t hbm = s;
  const std::vector<Slice> sl = lanes ? std::vector<Slice>{Slice{0, R, s}} : make_slices(e, s, &hbm);
  const bool multi = sl.size() > 1;
  const int NL = lanes ? e->n_lanes : 1;
  // scratch of the per-timestep head: one region per lane / slice
  const int64_t score_cap = std::max<int64_t>(lram_engine::kScoreMinRows, std::min<int64_t>(e->score_rows, (int64_t)R * stride));
  const size_t score_region = (size_t)score_cap * c.act_dim * c.n_vocab;
  if (score_chunks) grow(e->SCORE_LG, score_region * (lanes ? (size_t)NL : sl.size()));
  if (multi && base.compat_pass == 0) fork_slices(e, sl, hbm, s);
  hipStream_t lane_s[lram_engine::kMaxLanes] = {s, s, s};
  if (lanes) {
    while ((int)e->micro_streams.size() < NL - 1) {
      hipStream_t ns;
      LRAM_HIP_CHECK(hipStreamCreateWithFlags(&ns, hipStreamNonBlocking));
      e->micro_streams.push_back(ns);
    }
    for (int k = 1; k < NL; ++k) lane_s[k] = e->micro_streams[k - 1];
    for (auto& v : e->lane_ev)
      while ((int)v.size() < c.n_blocks) v.push_back(new_event(e, false));
    for (int k = 1; k < NL; ++k) stream_after(e, lane_s[k], s, true);
  }
  // The slices of a chunk that runs rows [0, rows) only: every slice keeps its stream and its first row -- an env never changes
  // streams between chunks -- and loses the rows beyond; `idx` keeps its number among the call's slices (its score scratch).
  std::vector<Slice> use;
  std::vector<size_t> use_idx;
  auto clip_slices = [&](int rows) {
    use.clear(), use_idx.clear();
    for (size_t i = 0; i < sl.size(); ++i)
      if (sl[i].b0 < rows) use.push_back(Slice{sl[i].b0, std::min(sl[i].nb, rows - sl[i].b0), sl[i].s}), use_idx.push_back(i);
  };
  const bool started = plan != nullptr && !plan->rows.empty();
  int Tc = T, last_steps = 1;
  for (int ci = 0; ci < n_chunks; ++ci) {
    const int l = ch.at[ci], Lc = ch.at[ci + 1] - l;
    Tc = T * Lc;
    last_steps = Lc;
    const int lane = (n_chunks - 1 - ci) % NL;
    if (lanes)
      use.assign(1, Slice{0, started ? plan->rows[ci] : R, lane_s[lane]}), use_idx.assign(1, (size_t)lane);
    else if (started)
      clip_slices(plan->rows[ci]);
    else if (ci == 0)
      clip_slices(sl.back().b0 + sl.back().nb);
    if (base.context) e->ctx_counts[1] += 1, e->ctx_counts[2] += (int64_t)(use.back().b0 + use.back().nb) * Lc;
    // (scope guard: an exception out of a launch below must not leave the engine on a lane's workspace)
    struct LaneScope {
      lram_engine* e;
      int lane;
      ~LaneScope() {
        if (lane) swap_workspace(e, lane);
      }
    } lane_scope{e, lane};
    if (lane) swap_workspace(e, lane);
    // Per-env lengths on env slices: a slice's rows of the shared workspace are [b0 * Tc, (b0 + nb) * Tc), and the plan's chunks
    // differ in length anywhere in the call, so the rows a slice takes for this chunk may be ones another slice -- the slices
    // run a block or more apart -- is still working on for the chunk before.  Every slice leaves that chunk before any enters
    // this one.  (A dense call's chunks are all of one length but the last.)
    if (plan != nullptr && multi && ci > 0 && Lc != l - ch.at[ci - 1]) {
      for (const Slice& x : sl) stream_after(e, hbm, x.s);
      for (const Slice& x : sl) stream_after(e, x.s, hbm);
    }
    // (shared repeated forwards: the tokens of this env-step were embedded by pass 0 -- X0 / U0)
    if (!(base.compat_shared && base.compat_pass > 0))
      for (const Slice& x : use) embed_tokens(e, base, call, seq_emb, x, l, Lc);
    Pass pass = base;
    if (lanes) pass.lane_wait = ci > 0 ? &e->lane_ev[(lane + 1) % NL] : nullptr, pass.lane_rec = &e->lane_ev[lane];
    const uint8_t* chunk_reset = l == 0 && base.compat_pass == 0 ? call.reset : nullptr;
    if (plan != nullptr) chunk_reset = plan->has_reset[ci] ? plan->dev_masks + (size_t)ci * R : nullptr;
    // (a chunk without a held env passes no hold pointer: it launches what a dense call launches)
    if (plan != nullptr && plan->has_hold[ci]) pass.hold = plan->dev_hold + (size_t)ci * R;
    run_stack(e, pass, Tc, chunk_reset, use, lanes ? lane_s[lane] : hbm);
    if (score_chunks)
      for (size_t i = 0; i < use.size(); ++i)
        score_chunk(e, call, use[i], e->SCORE_LG.p + use_idx[i] * score_region, score_cap, l, Lc);
  }
  for (int k = 1; k < NL; ++k) stream_after(e, s, lane_s[k], true);
  // the head on the rows of the last chunk (with per-chunk rows: the envs with a context; the others' rows take the fill values)
  if (started || lanes) clip_slices(started ? plan->rows.back() : R);
  if (call.scored || call.actions != nullptr) action_head(e, base, call, use, Tc, last_steps);
  if (multi && base.compat_pass == base.compat_passes - 1) join_slices(e, sl, hbm, s);
}

// Do the repeated forwards of the Mamba reference-trajectory mode share the token front end and layer 0's in_proj?
bool compat_shares(const lram_engine* e, int discrete) {
  const int passes = discrete ? 1 : std::max(1, std::min(e->compat_repeat, e->cfg.act_dim));
  return passes > 1 && e->cfg.backbone == LRAM_BACKBONE_MAMBA && e->compat_share && e->cfg.n_blocks >= 2;
}

// Stored contexts and encoder calls run on every allocated slot unless lram_set_context_rows says otherwise: refused, with nothing
// launched, while slots are parked.
void require_all_live(const lram_engine* e, const char* who) {
  if (e->ctx_rows != LRAM_CONTEXT_ROWS_ALL) return;   // (the live prefix is what the call runs on)
  LRAM_REQUIRE(e->n_live == e->B, std::string(who) + ": " + std::to_string(e->B - e->n_live) + " of " + std::to_string(e->B) +
                                      " env slots are parked (lram_set_live): stored contexts and encoder calls need every slot "
                                      "live -- call lram_set_live(batch) first");
}

// What the entries that run (state, rtg, reward) env-steps share: the state is allocated, the front end fits the geometry, the
// device is current, and the call counts for a sampled profile.
void step_entry(lram_engine* e, const char* who) {
  const std::string w(who);
  LRAM_REQUIRE(e && e->B > 0, w + ": state not allocated (call lram_state_alloc)");
  LRAM_REQUIRE(e->cfg.tokens_per_step == 3, w + ": the (state, rtg, reward) front end needs tokens_per_step == 3");
  LRAM_HIP_CHECK(hipSetDevice(e->device));
  prof_tick(e);
}

}  // namespace lram::host

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int32_t lram_step(lram_engine* e, const float* dev_obs, int32_t obs_is_embedding, const float* dev_rtg,
                  const float* dev_reward, const uint8_t* dev_reset_mask, int32_t discrete, float* dev_actions,
                  int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    step_entry(e, "lram_step");
    LRAM_REQUIRE(dev_obs && dev_rtg && dev_reward && dev_actions, "lram_step: null device pointer");
    check_head_mode(e, discrete, "lram_step");
    hipStream_t s = static_cast<hipStream_t>(stream);
    compat_prepare(e, discrete);  // (workspace of the shared repeated forwards: outside any capture)
    const Call call{"lram_step", Inputs{dev_obs, obs_is_embedding, dev_rtg, dev_reward, 1}, dev_reset_mask, discrete, dev_actions,
                    dev_tokens};
    if (e->graph_mode && !(e->prof_on && e->prof_live)) {  // (a sampled run's un-timed steps keep the graph path)
      GraphKey key{};
      key.obs = dev_obs, key.rtg = dev_rtg, key.rew = dev_reward, key.mask = dev_reset_mask, key.act = dev_actions;
      key.tok = dev_tokens, key.emb = obs_is_embedding, key.discrete = discrete, key.B = e->n_live, key.stream = s;
      if (!(e->graph_valid && key == e->graph_key)) {
        e->drop_graph();
        if (!e->capture_stream) LRAM_HIP_CHECK(hipStreamCreateWithFlags(&e->capture_stream, hipStreamNonBlocking));
        hipStream_t cs = e->capture_stream;
        LRAM_HIP_CHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
        try {
          step_launches(e, Pass{}, call, cs);
        } catch (...) {
          hipGraph_t g = nullptr;
          (void)hipStreamEndCapture(cs, &g);
          if (g) (void)hipGraphDestroy(g);
          throw;
        }
        LRAM_HIP_CHECK(hipStreamEndCapture(cs, &e->graph));
        LRAM_HIP_CHECK(hipGraphInstantiate(&e->graph_exec, e->graph, nullptr, nullptr, 0));
        e->graph_key = key;
        e->graph_valid = true;
      }
      LRAM_HIP_CHECK(hipGraphLaunch(e->graph_exec, s));
    } else {
      step_launches(e, Pass{}, call, s);
    }
  });
}

int32_t lram_step_images(lram_engine* e, const uint8_t* dev_images, int32_t channels, int32_t height, int32_t width,
                         const float* dev_rtg, const float* dev_reward, const uint8_t* dev_reset_mask, int32_t discrete,
                         float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    step_entry(e, "lram_step_images");
    LRAM_REQUIRE(dev_images && dev_rtg && dev_reward && dev_actions && channels > 0 && height > 0 && width > 0,
                 "lram_step_images: bad argument");
    LRAM_REQUIRE(e->img_lin_w != nullptr, "lram_step_images: no embed_image.* weights were uploaded");
    check_head_mode(e, discrete, "lram_step_images");
    step_image_buffers(e, channels, height, width, "lram_step_images");
    compat_prepare(e, discrete);
    Pass pass;   // (the frames belong to this call only)
    pass.images = dev_images, pass.img_c = channels, pass.img_h = height, pass.img_w = width;
    // (launch-per-kernel path also in graph mode: a captured step would pin one frame buffer)
    step_launches(e, pass, Call{"lram_step_images", Inputs{e->IMG_EMB.p, 1, dev_rtg, dev_reward, 1}, dev_reset_mask, discrete,
                                dev_actions, dev_tokens},
                  static_cast<hipStream_t>(stream));
  });
}

int32_t lram_step_slots(lram_engine* e, const float* dev_obs, const uint8_t* dev_images, int32_t channels, int32_t height,
                        int32_t width, const float* dev_rtg, const float* dev_reward, const uint8_t* dev_reset_mask,
                        float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    step_entry(e, "lram_step_slots");
    LRAM_REQUIRE(e->slot_table, "lram_step_slots: no slot table is set (lram_set_slot_table)");
    const int n_img = e->slot_img_prefix[e->n_live];   // the image slots of the live prefix: the frames this call is handed
    LRAM_REQUIRE(dev_rtg && dev_reward && dev_actions, "lram_step_slots: null device pointer");
    LRAM_REQUIRE(dev_obs != nullptr || n_img == e->n_live, "lram_step_slots: dev_obs is NULL and the table holds vector slots");
    check_head_mode(e, LRAM_HEAD_PER_SLOT, "lram_step_slots");
    if (n_img > 0) {
      LRAM_REQUIRE(e->img_lin_w != nullptr, "lram_step_slots: the table holds image slots and no embed_image.* weights were uploaded");
      LRAM_REQUIRE(dev_images && channels > 0 && height > 0 && width > 0, "lram_step_slots: the table holds image slots: frames needed");
      LRAM_REQUIRE(e->cfg.d_model % 4 == 0, "lram_step_slots: image slots need d_model to be a multiple of 4");
      step_image_buffers(e, channels, height, width, "lram_step_slots");
    }
    Pass pass;   // (the frames and the mixed front end belong to this call only)
    pass.slots = true;
    pass.images = n_img > 0 ? dev_images : nullptr, pass.img_c = channels, pass.img_h = height, pass.img_w = width;
    // (launch-per-kernel path also in graph mode: a captured step would pin one frame buffer, as in lram_step_images)
    step_launches(e, pass, Call{"lram_step_slots", Inputs{dev_obs, 0, dev_rtg, dev_reward, 1}, dev_reset_mask, LRAM_HEAD_PER_SLOT,
                                dev_actions, dev_tokens},
                  static_cast<hipStream_t>(stream));
  });
}

int32_t lram_encoder_step(lram_engine* e, const float* dev_inputs_embeds, int32_t tokens,
                          const uint8_t* dev_reset_mask, float* dev_hidden_out, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_encoder_step: state not allocated");
    LRAM_REQUIRE(dev_inputs_embeds && dev_hidden_out, "lram_encoder_step: null device pointer");
    require_all_live(e, "lram_encoder_step");
    const bool chunk_ok = e->cfg.backbone == LRAM_BACKBONE_XLSTM && e->chunk_prefill && !e->graph_mode &&
                          mlstm_chunk_supported(e->cfg.inner, e->cfg.n_heads, e->cfg.conv_k);
    LRAM_REQUIRE((tokens >= 1 && tokens <= 4) || tokens == 6 || tokens == 9 || tokens == 12 ||
                     (chunk_ok && tokens > kMaxTokens && tokens <= kChunkMaxTokens),
                 "lram_encoder_step: tokens must be 1..4, 6, 9 or 12 (13..64 too on xLSTM geometries with a head dim "
                 "that is a multiple of 128)");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    if (tokens > e->tok_cap) {
      LRAM_HIP_CHECK(hipDeviceSynchronize());
      alloc_workspace(e, kChunkMaxTokens);
      LRAM_HIP_CHECK(hipDeviceSynchronize());
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    prof_tick(e);
    // (the rows of the call: the slices below cut the live prefix, which is the batch unless lram_set_context_rows lets it differ)
    const size_t bytes = sizeof(float) * (size_t)e->context_rows() * tokens * e->cfg.d_model;
    lazy_finish_prefold(e, s);   // (only an env-step takes a tail fold over)
    if (!lazy_active(e, tokens)) lazy_materialize(e, s);
    LRAM_HIP_CHECK(hipMemcpyAsync(e->X.p, dev_inputs_embeds, bytes, hipMemcpyDeviceToDevice, s));
    e->sync_used = 0, e->edge_used = 0;
    hipStream_t hbm;
    const std::vector<Slice> sl = make_slices(e, s, &hbm);
    if (sl.size() > 1) fork_slices(e, sl, hbm, s);
    run_stack(e, Pass{}, tokens, dev_reset_mask, sl, hbm);
    if (sl.size() > 1) join_slices(e, sl, hbm, s);
    LRAM_HIP_CHECK(hipMemcpyAsync(dev_hidden_out, e->HID.p, bytes, hipMemcpyDeviceToDevice, s));
  });
}

int32_t lram_get_taps(lram_engine* e, float* dev_tokens_embed, float* dev_hidden, float* dev_logits, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_get_taps: state not allocated");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t btd = sizeof(float) * (size_t)e->n_live * e->cfg.tokens_per_step * e->cfg.d_model;   // (the live rows)
    if (dev_tokens_embed) {
      LRAM_REQUIRE(e->B <= kTokenTapMaxBatch,
                   "lram_get_taps: the embed_ln token tap is kept for batches of up to 1024 env slots only (it costs a "
                   "copy of the token buffer per step); pass NULL for it");
      LRAM_HIP_CHECK(hipMemcpyAsync(dev_tokens_embed, e->TOK.p, btd, hipMemcpyDeviceToDevice, s));
    }
    if (dev_hidden) LRAM_HIP_CHECK(hipMemcpyAsync(dev_hidden, e->HID.p, btd, hipMemcpyDeviceToDevice, s));
    if (dev_logits)
      LRAM_HIP_CHECK(hipMemcpyAsync(dev_logits, e->LOGITS.p, sizeof(float) * (e->LOGITS.n / e->B) * e->n_live, hipMemcpyDeviceToDevice, s));
  });
}

}  // extern "C"
