// The action head: its logits per env slice, then argmax, a sampled draw or a score (action_head); the head at every timestep of a
// stored-context chunk (score_chunk); what a call is refused for on account of its head (check_head_mode, check_score_sink); and
// the entries that run the head alone -- on the logits of the last call (lram_score_last, lram_score_last_sampled) or on the
// caller's (lram_score_tokens*, lram_sample_rows*, lram_sample_tokens, lram_sample_uniforms).
// Calls gemm.
#include "engine.h"

namespace {

// The engine's head geometry, and the slot table of a call as the slice from env slot b0 on sees it (none unless the call is
// per-slot).
HeadGeom head_geom(const lram_config& c) { return {c.act_dim, c.n_vocab, c.n_discrete, c.action_channels, c.tok_min, c.tok_max}; }
HeadSlots head_slots(const lram_engine* e, int discrete, size_t b0) {
  if (discrete != LRAM_HEAD_PER_SLOT) return {};
  return {e->slot_dev + b0, e->slot_dev + e->B + b0};
}

// The allowed-action sets as the slice from env slot b0 on sees them ({null, 0} without a mask: the unmasked kernels).
HeadMask head_mask(const lram_engine* e, size_t b0) {
  if (e->mask_dev == nullptr) return {};
  return {e->mask_dev + b0 * (size_t)e->mask_words, e->mask_words};
}

// What every score launch of a call shares: the head's geometry, the sink's tensors, the slot table of a per-slot call.
ScoreArgs score_args(const lram_engine* e, const ScoreSink& k, int discrete) {
  ScoreArgs a;
  a.geom = head_geom(e->cfg), a.slots = head_slots(e, discrete, 0);
  a.discrete = discrete == LRAM_HEAD_PER_SLOT ? 0 : discrete;
  a.over = k.over, a.temperature = k.temperature;
  a.target_actions = k.target_actions, a.target_tokens = k.target_tokens, a.valid = k.valid;
  a.actions = k.actions, a.tokens = k.tokens, a.logp = k.logp, a.logits_out = k.logits;
  return a;
}

// The head rules every caller shares, each checked before anything is launched (the recurrent state is untouched by a refused
// call); `w` names the entry.  kHeadRange: `discrete` is a caller's argument that has to be one of the three modes.  kHeadDraws:
// the call draws, or scores the distribution a draw comes from -- every sampling slot's top_k must fit the head the call gives
// that slot: n_discrete logits on a discrete head, n_vocab otherwise (checked when the table was set).
enum : int { kHeadRange = 1, kHeadDraws = 2 };
void check_head_rules(const lram_engine* e, int discrete, const std::string& w, int rules) {
  const bool per_slot = discrete == LRAM_HEAD_PER_SLOT;
  LRAM_REQUIRE(!(rules & kHeadRange) || discrete == 0 || discrete == 1 || per_slot, w + ": discrete must be 0, 1 or LRAM_HEAD_PER_SLOT");
  LRAM_REQUIRE(!per_slot || e->slot_table, w + ": LRAM_HEAD_PER_SLOT needs a slot table (lram_set_slot_table)");
  // (n_discrete = 0 is a legal geometry -- the reference's dmcontrol head -- but an argmax over no logits is no action)
  LRAM_REQUIRE(discrete != 1 || e->cfg.n_discrete >= 1, w + ": a discrete head needs n_discrete >= 1");
  if ((rules & kHeadDraws) && e->sampling && discrete != 0) {
    if (!e->sample_slots.empty()) {   // per-slot settings: read from the host-side maxima, no per-step cost
      const int k = per_slot ? e->sslot_kd_max : e->sslot_k_max, at = per_slot ? e->sslot_kd_at : e->sslot_k_at;
      LRAM_REQUIRE(k <= e->cfg.n_discrete, w + ": sampling top_k " + std::to_string(k) + " of slot " + std::to_string(at) +
                                               " exceeds the n_discrete = " + std::to_string(e->cfg.n_discrete) +
                                               " logits of the discrete head that slot gets");
    } else {
      LRAM_REQUIRE(!(per_slot && e->slot_has_discrete && e->sample.top_k > e->cfg.n_discrete),
                   w + ": sampling top_k exceeds n_discrete and the slot table holds a discrete slot");
    }
  }
  // A discrete = 1 call reads [0, n_discrete) on every slot: refused while some slot's allowed-action set holds nothing there.
  LRAM_REQUIRE(!(discrete == 1 && e->mask_no_discrete_at >= 0),
               w + ": the action mask (lram_set_action_mask) allows slot " + std::to_string(e->mask_no_discrete_at) +
                   " nothing below n_discrete: a discrete = 1 call would leave it an empty sub-row");
}

// What lram_score_last and lram_score_last_sampled share: there are logits to score, and the head mode they were made under
// (returned) still stands; `rules`: kHeadDraws where the armed distribution is scored.
int last_head_entry(lram_engine* e, const char* who, const int32_t* dev_tokens, const float* dev_logp, int rules) {
  const std::string w(who);
  LRAM_REQUIRE(e != nullptr, w + ": null engine");
  LRAM_REQUIRE(e->B > 0, w + ": state not allocated (call lram_state_alloc)");
  LRAM_HIP_CHECK(hipSetDevice(e->device));
  prof_tick(e);
  LRAM_REQUIRE(dev_tokens && dev_logp, w + ": null device pointer");
  LRAM_REQUIRE(e->last_head >= 0, w + ": no action-producing call since lram_state_alloc: there are no logits to score");
  LRAM_REQUIRE(!(rules & kHeadDraws) || e->sampling, w + ": sampling is not armed (lram_set_sampling): there is no drawn distribution");
  LRAM_REQUIRE(e->last_head != LRAM_HEAD_PER_SLOT || e->slot_table, w + ": the last call was per-slot and the slot table has been cleared since");
  check_head_rules(e, e->last_head, w, rules);
  return e->last_head;
}

// lram_score_tokens and lram_score_tokens_masked: the scoring head's row code on caller logits; `who` names the entry called.
void score_tokens_call(const char* who, const float* dev_logits, int64_t rows, const HeadGeom& geom, int discrete,
                       const float* dev_target_actions, const int32_t* dev_target_tokens, const uint8_t* dev_valid, int over,
                       double temperature, float* dev_actions, int32_t* dev_tokens, float* dev_logp, const HeadMask& mask,
                       void* stream) {
  const std::string w(who);
  LRAM_REQUIRE(dev_logits != nullptr, w + ": null device pointer");
  LRAM_REQUIRE(discrete == 0 || discrete == 1, w + ": discrete must be 0 or 1");
  ScoreArgs a;
  a.logits = dev_logits, a.ld = (int64_t)geom.act_dim * geom.n_vocab, a.rows = rows;
  a.geom = geom;
  a.discrete = discrete, a.over = over, a.temperature = temperature;
  a.target_actions = dev_target_actions, a.target_tokens = dev_target_tokens, a.valid = dev_valid;
  a.actions = dev_actions, a.tokens = dev_tokens, a.logp = dev_logp;
  launch_action_score(a, static_cast<hipStream_t>(stream), mask);
}

// lram_sample_rows and lram_sample_rows_masked: the row sampler on caller logits; `who` names the entry called.
void sample_rows_call(const char* who, const float* dev_logits, int64_t rows, int32_t n, int64_t ld, const uint8_t* dev_mode,
                      const double* dev_temperature, const int32_t* dev_top_k, const double* dev_top_p, const double* dev_uniform,
                      const int32_t* dev_tokens_in, int32_t* dev_tokens_out, float* dev_logp_out, const HeadMask& mask, void* stream) {
  const std::string w(who);
  LRAM_REQUIRE(dev_logits && dev_mode && dev_temperature && dev_top_k && dev_top_p, w + ": null device pointer");
  LRAM_REQUIRE((dev_uniform == nullptr) == (dev_tokens_out == nullptr), w + ": dev_uniform and dev_tokens_out go together");
  LRAM_REQUIRE((dev_tokens_in == nullptr) == (dev_logp_out == nullptr), w + ": dev_tokens_in and dev_logp_out go together");
  LRAM_REQUIRE(dev_tokens_out || dev_logp_out, w + ": neither a draw (dev_uniform, dev_tokens_out) nor a score "
                                                   "(dev_tokens_in, dev_logp_out) is asked for");
  LRAM_REQUIRE(ld == 0 || ld >= n, w + ": ld must be 0 (one shared row) or >= n");
  launch_sample_rows(dev_logits, rows, n, ld, dev_mode, dev_temperature, dev_top_k, dev_top_p, dev_uniform, dev_tokens_in,
                     dev_tokens_out, dev_logp_out, static_cast<hipStream_t>(stream), mask);
}

}  // namespace

namespace lram::host {

// The head at EVERY timestep of the chunk of Lc timesteps from l0 on that the slice has just run through the stack: the chunk's
// action-token rows of HID (row (b, l) at ((b * Lc + l) * T + pred) * D: one stride) against action_net, in blocks of at most
// `cap` rows into the region's scratch, each block scored into rows [b, l0 + l] of the call's sink.  The exact fp32 matrix-core
// kernel without split-K: a row's logits are one k-ordered fma chain whatever the block it falls into, so the outputs do not
// depend on the scratch bound.  (A last block of <= 8 rows would take the GEMV kernel, another summation order: it starts
// kScoreMinRows before the end instead and recomputes the rows it overlaps.)
void score_chunk(lram_engine* e, const Call& call, const Slice& x, float* scratch, int64_t cap, int l0, int Lc) {
  const lram_config& c = e->cfg;
  const int D = c.d_model, T = c.tokens_per_step;
  const int64_t nlog = (int64_t)c.act_dim * c.n_vocab, R = (int64_t)x.nb * Lc;
  for (int64_t r = 0; r < R;) {
    int64_t beg = r, nr = std::min(cap, R - r);
    r += nr;
    if (nr < lram_engine::kScoreMinRows && beg > 0) beg = R - lram_engine::kScoreMinRows, nr = lram_engine::kScoreMinRows;
    GemmArgs gh;
    gh.a = e->HID.p + (((size_t)x.b0 * Lc + beg) * T + c.pred_token) * D, gh.lda = (int64_t)T * D;
    gh.w = e->w_head, gh.ldw = D, gh.c = scratch, gh.ldc = nlog, gh.bias = e->b_head;
    gh.m = (int)nr, gh.n = (int)nlog, gh.k = D, gh.knobs = e->gemm_knobs;   // (a tile launcher without gemm())
    launch_gemm_f32(gh, x.s);
    count_gemm(e, 2, gh);
    ScoreArgs a = score_args(e, call.sink, call.discrete);
    a.logits = scratch, a.ld = nlog, a.row0 = (int64_t)x.b0 * Lc + beg, a.rows = nr;
    a.inner = Lc, a.outer = call.in.L, a.off = l0, a.start = call.ctx_start();
    launch_action_score(a, x.s, head_mask(e, 0));
  }
}

// Action head on the last timestep of the last chunk (Tc tokens per env, last_steps timesteps): logits per env slice, then
// argmax or a sampled draw into the call's actions / tokens.  What discrete = LRAM_HEAD_PER_SLOT needs was checked by the entry
// (check_head_mode).  A scored call (lram_score over L timesteps) has the same logits scored into row [b, L - 1] of its sink's
// tensors instead: no draw.
void action_head(lram_engine* e, const Pass& pass, const Call& call, const std::vector<Slice>& sl, int Tc, int last_steps) {
  const lram_config& c = e->cfg;
  const int D = c.d_model, T = c.tokens_per_step, L = call.in.L, discrete = call.discrete;
  const int64_t nlog = (int64_t)c.act_dim * c.n_vocab;
  const int pred = T * (last_steps - 1) + c.pred_token;  // rtg token of the last timestep in the last chunk
  // shared repeated forwards: pass p only has to produce action dim p (the last pass every dim from its own on), so
  // the head evaluates that column block of action_net alone
  const int col_begin = pass.compat_pass;
  const int col_end = (pass.compat_shared && col_begin + 1 < pass.compat_passes) ? col_begin + 1 : c.act_dim;
  const int col0 = pass.compat_shared ? col_begin : 0;
  e->last_head = discrete;
  const HeadGeom geom = head_geom(c);
  for (const Slice& x : sl) {
    const size_t r0 = (size_t)x.b0 * Tc, b0 = x.b0;
    GemmArgs gh;
    gh.a = e->HID.p + (r0 + pred) * D, gh.lda = (int64_t)Tc * D, gh.w = e->w_head + (size_t)col0 * c.n_vocab * D, gh.ldw = D;
    gh.c = e->LOGITS.p + b0 * nlog + (size_t)col0 * c.n_vocab, gh.ldc = nlog, gh.bias = e->b_head + (size_t)col0 * c.n_vocab;
    gh.m = x.nb, gh.n = (col_end - col0) * c.n_vocab, gh.k = D;
    gemm(e, gh, x.s);
    if (call.scored) {
      ScoreArgs a = score_args(e, call.sink, discrete);
      a.logits = e->LOGITS.p + b0 * nlog, a.ld = nlog, a.row0 = (int64_t)b0, a.rows = x.nb;
      a.inner = 1, a.outer = L, a.off = L - 1, a.start = call.ctx_start();
      launch_action_score(a, x.s, head_mask(e, 0));
      continue;
    }
    const float* logits = e->LOGITS.p + b0 * nlog;
    float* act = call.actions + b0 * c.act_dim;
    int32_t* tok = call.tokens ? call.tokens + b0 * c.act_dim : nullptr;
    const HeadSlots slots = head_slots(e, discrete, b0);
    if (e->sampling) {
      SampleArgs sp = e->sample;
      sp.slot0 += b0, sp.draw = e->sample_draw;
      launch_action_sample(logits, act, tok, x.nb, geom, slots, discrete, col_begin, col_end, sp,
                           e->sample_slots_dev ? e->sample_slots_dev + b0 : nullptr, x.s, head_mask(e, b0));
      continue;
    }
    launch_action_argmax(logits, act, tok, x.nb, geom, slots, discrete, col_begin, col_end, x.s, head_mask(e, b0));
  }
}

// Sampling mode: one draw per action-producing call.  Launched on the caller's stream behind the join of the env slices
// (and behind the last of the repeated forwards), so that every row of the call has read the same count; the next call's
// slices fork from this stream and see the new one.  In a captured step it is one more node on the graph's single chain.
void sample_draw_advance(lram_engine* e, hipStream_t s) {
  if (e->sampling) launch_sample_advance(e->sample_draw, s);
}

// What a call that takes an action is refused for on account of its head mode; `who` names the entry.
void check_head_mode(const lram_engine* e, int discrete, const char* who) {
  const std::string w(who);
  check_head_rules(e, discrete, w, kHeadDraws);
  LRAM_REQUIRE(discrete != LRAM_HEAD_PER_SLOT || e->compat_repeat <= 1,
               w + ": LRAM_HEAD_PER_SLOT cannot be combined with the Mamba repeated-forward mode "
                   "(mamba_repeat > 1 advances the state once per action dim of the env, which differs per slot)");
}

// The refusals of the score entries for the sink they were handed and its head mode; `who` names the entry.
void check_score_sink(const lram_engine* e, const char* who, int discrete, const ScoreSink& k) {
  const std::string w(who);
  LRAM_REQUIRE(e->compat_repeat <= 1, w + ": the Mamba repeated-forward mode is on (lram_set_compat_mode, mamba_repeat > 1): "
                                      "its trajectories advance the state once per action dim and are not scored");
  LRAM_REQUIRE(!(k.target_actions && k.target_tokens), w + ": both dev_target_actions and dev_target_tokens are given (at most one)");
  LRAM_REQUIRE(k.actions || k.tokens || k.logp || k.logits, w + ": no output is given");
  LRAM_REQUIRE(!k.logp || k.target_actions || k.target_tokens,
               w + ": dev_logp needs a target (dev_target_actions or dev_target_tokens)");
  LRAM_REQUIRE(k.over == 0 || k.over == 1, w + ": over must be 0 (the whole vocabulary) or 1 (the selectable range)");
  LRAM_REQUIRE(k.temperature > 0.0 && k.temperature < (double)INFINITY, w + ": temperature must be finite and > 0");
  check_head_rules(e, discrete, w, kHeadRange);   // (a score is never a draw)
}

}  // namespace lram::host

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int32_t lram_score_last(lram_engine* e, const int32_t* dev_tokens, int32_t over, double temperature, float* dev_logp,
                        void* stream) {
  return guarded([&] {
    const int head = last_head_entry(e, "lram_score_last", dev_tokens, dev_logp, 0);
    ScoreSink sink;
    sink.logp = dev_logp, sink.target_tokens = dev_tokens, sink.over = over, sink.temperature = temperature;
    ScoreArgs a = score_args(e, sink, head);
    a.logits = e->LOGITS.p, a.ld = (int64_t)e->cfg.act_dim * e->cfg.n_vocab, a.rows = e->n_live;
    launch_action_score(a, static_cast<hipStream_t>(stream), head_mask(e, 0));
  });
}

int32_t lram_score_last_sampled(lram_engine* e, const int32_t* dev_tokens, float* dev_logp, void* stream) {
  return guarded([&] {
    const int head = last_head_entry(e, "lram_score_last_sampled", dev_tokens, dev_logp, kHeadDraws);
    // (deterministic: no uniform is read, the draw counter is neither read nor advanced)
    launch_action_logp(e->LOGITS.p, dev_tokens, dev_logp, e->n_live, head_geom(e->cfg), head_slots(e, head, 0), head, e->sample,
                       e->sample_slots_dev, static_cast<hipStream_t>(stream), head_mask(e, 0));
  });
}

int32_t lram_sample_rows(const float* dev_logits, int64_t rows, int32_t n, int64_t ld, const uint8_t* dev_mode,
                         const double* dev_temperature, const int32_t* dev_top_k, const double* dev_top_p,
                         const double* dev_uniform, const int32_t* dev_tokens_in, int32_t* dev_tokens_out, float* dev_logp_out,
                         void* stream) {
  return guarded([&] {
    sample_rows_call("lram_sample_rows", dev_logits, rows, n, ld, dev_mode, dev_temperature, dev_top_k, dev_top_p, dev_uniform,
                     dev_tokens_in, dev_tokens_out, dev_logp_out, HeadMask{}, stream);
  });
}

int32_t lram_sample_rows_masked(const float* dev_logits, int64_t rows, int32_t n, int64_t ld, const uint8_t* dev_mode,
                                const double* dev_temperature, const int32_t* dev_top_k, const double* dev_top_p,
                                const double* dev_uniform, const int32_t* dev_tokens_in, int32_t* dev_tokens_out,
                                float* dev_logp_out, const uint32_t* dev_mask, int32_t words, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(dev_mask != nullptr, "lram_sample_rows_masked: null device pointer (dev_mask)");
    LRAM_REQUIRE(n >= 1 && words == (n + 31) / 32, "lram_sample_rows_masked: words must be ceil(n / 32)");
    sample_rows_call("lram_sample_rows_masked", dev_logits, rows, n, ld, dev_mode, dev_temperature, dev_top_k, dev_top_p,
                     dev_uniform, dev_tokens_in, dev_tokens_out, dev_logp_out, HeadMask{dev_mask, words}, stream);
  });
}

int32_t lram_score_tokens(const float* dev_logits, int64_t rows, int32_t act_dim, int32_t n_vocab, int32_t n_discrete,
                          int32_t action_channels, float tok_min, float tok_max, int32_t discrete, const float* dev_target_actions,
                          const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over, double temperature,
                          float* dev_actions, int32_t* dev_tokens, float* dev_logp, void* stream) {
  return guarded([&] {
    score_tokens_call("lram_score_tokens", dev_logits, rows, {act_dim, n_vocab, n_discrete, action_channels, tok_min, tok_max},
                      discrete, dev_target_actions, dev_target_tokens, dev_valid, over, temperature, dev_actions, dev_tokens,
                      dev_logp, HeadMask{}, stream);
  });
}

int32_t lram_score_tokens_masked(const float* dev_logits, int64_t rows, int32_t act_dim, int32_t n_vocab, int32_t n_discrete,
                                 int32_t action_channels, float tok_min, float tok_max, int32_t discrete,
                                 const float* dev_target_actions, const int32_t* dev_target_tokens, const uint8_t* dev_valid,
                                 int32_t over, double temperature, float* dev_actions, int32_t* dev_tokens, float* dev_logp,
                                 const uint32_t* dev_mask, int32_t words, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(dev_mask != nullptr, "lram_score_tokens_masked: null device pointer (dev_mask)");
    LRAM_REQUIRE(words == (n_vocab + 31) / 32, "lram_score_tokens_masked: words must be ceil(n_vocab / 32)");
    score_tokens_call("lram_score_tokens_masked", dev_logits, rows, {act_dim, n_vocab, n_discrete, action_channels, tok_min, tok_max},
                      discrete, dev_target_actions, dev_target_tokens, dev_valid, over, temperature, dev_actions, dev_tokens,
                      dev_logp, HeadMask{dev_mask, words}, stream);
  });
}

int32_t lram_sample_tokens(const float* dev_logits, int64_t rows, int32_t n, int64_t ld, double temperature, int32_t top_k,
                           double top_p, const double* dev_uniform, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(dev_logits && dev_uniform && dev_tokens, "lram_sample_tokens: null device pointer");
    LRAM_REQUIRE(temperature > 0.0 && temperature < (double)INFINITY, "lram_sample_tokens: temperature must be finite and > 0");
    LRAM_REQUIRE(top_p >= 0.0 && top_p <= 1.0, "lram_sample_tokens: top_p must be in [0, 1]");
    LRAM_REQUIRE(top_k >= 0 && top_k <= n, "lram_sample_tokens: top_k must be in 0 .. n");
    LRAM_REQUIRE(ld == 0 || ld >= n, "lram_sample_tokens: ld must be 0 (one shared row) or >= n");
    launch_sample_tokens(dev_logits, rows, n, ld, temperature, top_k, top_p, dev_uniform, dev_tokens,
                         static_cast<hipStream_t>(stream));
  });
}

int32_t lram_sample_uniforms(uint64_t seed, uint64_t slot_base, int64_t n_slots, int32_t act_dim, uint64_t draw,
                             double* dev_out, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(dev_out != nullptr, "lram_sample_uniforms: null device pointer");
    launch_sample_uniforms(seed, slot_base, n_slots, act_dim, draw, dev_out, static_cast<hipStream_t>(stream));
  });
}

}  // extern "C"
