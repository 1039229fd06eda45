// Stored contexts: the chunk plan of a call of per-env lengths (context_plan, RaggedCall), the one body of the eight entries
// (stored_context_call) and the entries themselves -- lram_prefill and lram_score, each dense, _ragged, _append and _frames -- with
// lram_context_plan and the context-row setting and counters.
// Calls the chunk loop (engine_step.hip), the head's and the image front end's checks, and the slot records (engine_state.hip).
#include "engine.h"

namespace {

// The length rules of a call of L timesteps over B contexts of per-env length: every length in 0 .. L, not all of them 0.
void check_lengths(const int32_t* lengths, int B, int L, const std::string& w) {
  bool any = false;
  for (int b = 0; b < B; ++b) {
    LRAM_REQUIRE(lengths[b] >= 0 && lengths[b] <= L, w + ": length " + std::to_string(lengths[b]) + " of env slot " +
                                                          std::to_string(b) + " is outside 0 .. timesteps = " + std::to_string(L));
    any = any || lengths[b] > 0;
  }
  LRAM_REQUIRE(any, w + ": every length is 0 (no env slot has a context)");
}

// The chunk plan of a call of L timesteps over contexts of per-env length (include/lram_hip.h: lram_context_plan): pure host code.
// Throws on a length outside 0 .. L or when every length is 0.
std::vector<int> context_plan(int L, int cap, const int32_t* lengths, int B, const char* who) {
  const std::string w(who);
  LRAM_REQUIRE(L >= 1 && cap >= 1 && B >= 1 && lengths != nullptr, w + ": bad argument (timesteps, cap, batch >= 1, lengths given)");
  check_lengths(lengths, B, L, w);
  std::vector<char> begins(L, 0);   // begins[t]: some env with a context starts at call-timestep t
  for (int b = 0; b < B; ++b)
    if (lengths[b] > 0) begins[L - lengths[b]] = 1;
  std::vector<int> bounds;
  for (int t = 0; t < L; ++t)
    if (begins[t]) bounds.push_back(t);
  std::vector<int> starts;
  if (bounds.size() == 1 && bounds[0] == 0) {   // no env starts inside the call: the dense call's own chunks
    for (int t = 0; t < L; t += cap) starts.push_back(t);
    return starts;
  }
  bounds.push_back(L);
  for (size_t i = 0; i + 1 < bounds.size(); ++i) {
    const int len = bounds[i + 1] - bounds[i];
    const int n = (len + cap - 1) / cap, step = (len + n - 1) / n;
    for (int t = bounds[i]; t < bounds[i + 1]; t += step) starts.push_back(t);
  }
  return starts;
}

// The per-env lengths of a stored-context call (Call::ragged: the ragged and append entries, and the entries from frames that
// were handed lengths).  check(): everything that refuses the call for its lengths, before anything is launched or allocated.
// run(): the plan and its device tables, then the chunks (`launch` runs the chunk loop with the plan).  A call whose lengths all
// equal `timesteps` never gets to run(): it is the dense entry's.
// What an env sees ahead of its context differs by kind.  Replace (the ragged entries): zero tokens through every kernel and a
// reset at its own first timestep, whatever the caller's mask says; the slots of length 0 have their records saved into KEEP
// ahead of the chunks and loaded back behind them.  `append`: the env is HELD in every chunk it has not started by
// (ContextPlan::dev_hold -> Pass::hold: no kernel writes its state) and restarts only where the caller's mask says so; KEEP is
// not touched and no memory is asked for.
struct RaggedCall {
  lram_engine* e;
  std::string w;   // the entry's name
  int L;
  const int32_t* lengths;
  bool append;
  ContextPlan plan;   // (made by run())

  void check(int obs_is_embedding) const {
    const lram_config& c = e->cfg;
    const int B = e->context_rows();
    LRAM_REQUIRE(lengths != nullptr, w + ": host_lengths is NULL");
    check_lengths(lengths, B, L, w);
    // (started rows are a prefix of the slots in every chunk: an env never starts after one that sits behind it)
    for (int b = 1; b < B && started(); ++b)
      LRAM_REQUIRE(lengths[b] <= lengths[b - 1],
                   w + ": LRAM_CONTEXT_ROWS_STARTED needs lengths that do not increase in slot order over the live prefix; length " +
                       std::to_string(lengths[b]) + " of env slot " + std::to_string(b) + " exceeds length " +
                       std::to_string(lengths[b - 1]) + " of env slot " + std::to_string(b - 1));
    LRAM_REQUIRE(c.d_model % 4 == 0, w + ": per-env lengths need d_model to be a multiple of 4 (the chunk front end moves float4)");
    LRAM_REQUIRE(e->compat_repeat <= 1, w + ": the Mamba repeated-forward mode is on (lram_set_compat_mode, mamba_repeat > 1): its "
                                            "trajectories advance the state once per action dim and take no per-env lengths");
    LRAM_REQUIRE(!e->compat_stale, w + ": the Mamba stale_state mode is on (lram_set_compat_mode): a reset re-initialises layer 0 "
                                       "only, so the padding ahead of a shorter context would leak into the other layers");
    LRAM_REQUIRE(obs_is_embedding || (size_t)B * L * c.d_model <= ((size_t)1 << 29),
                 w + ": the [batch, timesteps, d_model] state embeddings of the raw observations exceed 2 GiB");
  }
  bool started() const { return e->ctx_rows == LRAM_CONTEXT_ROWS_STARTED; }
  bool dense() const {
    for (int b = 0; b < e->context_rows(); ++b)
      if (lengths[b] != L) return false;
    return true;
  }

  // B below: the rows of the call (lram_engine::context_rows) -- every table is that wide.  LRAM_CONTEXT_ROWS_STARTED: a chunk runs
  // the envs that have started by it and nobody else, so no env is held, none is fed zero tokens, and a slot of length 0 is never
  // a row: nothing to keep.
  template <typename Launch>
  void run(const uint8_t* reset, hipStream_t s, Launch&& launch) {
    const int B = e->context_rows();
    std::vector<int32_t> kept;   // replace: the slots of length 0
    for (int b = 0; b < B && !append && !started(); ++b)
      if (lengths[b] == 0) kept.push_back(b);
    // scratch for the kept slots' records: refused, with nothing launched, when it would leave less than 2 GiB free
    const size_t need = kept.size() * (size_t)(lram_state_bytes_per_env(e) / 4);
    grow({{&e->KEEP, need}}, [&] {
      size_t free_b = 0, total_b = 0;
      LRAM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
      LRAM_REQUIRE(need * sizeof(float) + ((size_t)2 << 30) <= free_b + e->KEEP.n * sizeof(float),
                   w + ": the records of the " + std::to_string(kept.size()) + " slots of length 0 (" +
                       std::to_string(need * sizeof(float)) + " bytes) would leave less than 2 GiB of device memory free");
    });
    plan.starts = context_plan(L, L > 1 ? prefill_chunk_steps(e, L) : 1, lengths, B, w.c_str());
    const int n_chunks = (int)plan.starts.size();
    // CTX: int32 start[B] | int32 chunk_start[L] | uint8 masks[L, B] | uint8 hold[L, B], as floats of one allocation
    grow(e->CTX, (size_t)B + L + ((size_t)2 * L * B + 3) / 4);
    int32_t* dev_start = reinterpret_cast<int32_t*>(e->CTX.p);
    int32_t* dev_chunk = dev_start + B;
    uint8_t* dev_masks = reinterpret_cast<uint8_t*>(dev_chunk + L);
    uint8_t* dev_hold = dev_masks + (size_t)L * B;
    plan.dev_start = dev_start, plan.dev_masks = dev_masks, plan.dev_hold = dev_hold, plan.lengths = lengths;
    std::vector<int32_t> host(B + n_chunks);
    plan.has_reset.assign(n_chunks, 0);
    plan.has_hold.assign(n_chunks, 0);
    for (int b = 0; b < B; ++b) {
      const int sb = L - lengths[b];
      host[b] = sb;
      // (every env with a context starts on a chunk boundary: the chunk it starts at)
      const size_t at = sb < L ? std::lower_bound(plan.starts.begin(), plan.starts.end(), sb) - plan.starts.begin() : (size_t)n_chunks;
      // restarted at its start (context_flags_kernel's rule): where the caller's mask may say so; replace: every shorter context
      if (sb < L && (reset != nullptr || (!append && sb > 0))) plan.has_reset[at] = 1;
      for (size_t ci = 0; ci < at && append && !started(); ++ci) plan.has_hold[ci] = 1;   // append: held in every chunk before that one
    }
    for (int ci = 0; ci < n_chunks; ++ci) host[B + ci] = plan.starts[ci];
    if (started()) {   // rows of chunk ci: the envs with s_b <= its start -- a prefix, the lengths do not increase (check())
      plan.rows.assign(n_chunks, 0);
      for (int ci = 0, r = 0; ci < n_chunks; ++ci) {
        while (r < B && L - lengths[r] <= plan.starts[ci]) ++r;
        plan.rows[ci] = r;
      }
    }
    // ---- from here on the call launches ----
    lazy_materialize(e, s);   // stored contexts fold pending windows first (and complete a tail fold)
    e->ctx_counts[3] += (int64_t)kept.size();
    if (!kept.empty()) save_slot_records(e, kept.data(), (int)kept.size(), e->KEEP.p, s);
    // (pageable host memory: the copies have read `host` when they return; the device side is ordered on `s`)
    LRAM_HIP_CHECK(hipMemcpyAsync(dev_start, host.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LRAM_HIP_CHECK(hipMemcpyAsync(dev_chunk, host.data() + B, (size_t)n_chunks * sizeof(int32_t), hipMemcpyHostToDevice, s));
    launch_context_flags(dev_hold, dev_masks, dev_start, dev_chunk, reset, !append, n_chunks, B, L, s);
    {
      // every chunk on the materialised kernels, also the chunks of one timestep that an env-step would take through the lazy
      // read pass: a window left pending by a chunk in the middle of the call would be invisible to the chunk behind it
      struct LazyOff {
        lram_engine* e;
        bool was;
        ~LazyOff() { e->lazy = was; }
      } lazy_off{e, e->lazy};
      e->lazy = false;
      launch(plan);
    }
    if (!kept.empty()) load_slot_records(e, kept.data(), (int)kept.size(), e->KEEP.p, s);
  }
};

// What the entries from frames refuse ahead of every other check (the state need not even be allocated): no frames, an `append`
// that is no flag, a slot table that leaves the call without a frame or its vector slots without observations.  Returns whether
// dev_obs_seq is read at all: the vector slots of a mixed table hand in observations; nobody else's is ever looked at.
// (Judged on the rows of the call: the image slots of the live prefix where lram_set_context_rows says so, as lram_step_slots.)
bool frames_entry(const lram_engine* e, const Call& c) {
  const std::string w(c.who);
  LRAM_REQUIRE(c.in.frames != nullptr, w + ": dev_frames is NULL");
  LRAM_REQUIRE(c.append == 0 || c.append == 1, w + ": append must be 0 (replace) or 1 (append)");
  const int R = e->context_rows(), n_image = e->slot_table && R > 0 ? e->slot_img_prefix[R] : 0;
  const bool mixed = e->slot_table && n_image < R;
  LRAM_REQUIRE(!e->slot_table || n_image > 0, w + ": the slot table holds no image slot: there is no frame to take");
  LRAM_REQUIRE(!mixed || c.in.obs != nullptr, w + ": dev_obs_seq is NULL and the slot table holds vector slots");
  return mixed;
}

// What the entries from frames refuse beyond the others (lram_prefill_frames / lram_score_frames), before anything is launched or
// allocated: no image encoder, a frame size that does not fit it, a geometry or mode without the state-embedding front end, state
// embeddings or flattened maps beyond 2 GiB.
void check_frames_call(const lram_engine* e, const Call& call) {
  const std::string w(call.who);
  const lram_config& c = e->cfg;
  const Inputs& in = call.in;
  LRAM_REQUIRE(in.img_c > 0 && in.img_h > 0 && in.img_w > 0, w + ": channels, height and width must be >= 1");
  check_frame_size(e, in.img_c, in.img_h, in.img_w, call.who);
  LRAM_REQUIRE(c.d_model % 4 == 0, w + ": stored contexts from frames need d_model to be a multiple of 4 (the chunk front end moves float4)");
  LRAM_REQUIRE(e->compat_repeat <= 1 && !e->compat_stale && !compat_shares(e, 0),
               w + ": a Mamba reference-trajectory mode is on (lram_set_compat_mode): its calls do not take their state "
                   "embeddings from one pass ahead of the chunks, which is where the frames are embedded");
  LRAM_REQUIRE((size_t)e->context_rows() * in.L * c.d_model <= ((size_t)1 << 29),
               w + ": the [batch, timesteps, d_model] state embeddings of the frames exceed 2 GiB");
  check_frame_list(e, count_frames(e, in.L, call.ragged ? call.host_lengths : nullptr).frames, call.who);
}

// What the eight stored-context entries share, in this order: the refusals (the recurrent state is untouched by a refused call,
// nothing is launched or allocated), the launches, the draw count.  c.who names the entry in every message.  A scored call runs
// the head at every timestep and draws nothing; any other has c.actions / c.tokens (nullable) take the action at every env's own
// last timestep.
// (The two halves are lram::host functions: lram_step_window runs the refusals, then its own ring launches, then the launches.)
void stored_context_call(lram_engine* e, Call c, hipStream_t s) {
  context_checks(e, c);
  context_launches(e, c, s);
}

}  // namespace

namespace lram::host {

// The refusals of a stored-context call, all of them: launches nothing, allocates nothing, changes nothing but c.in.obs (a call
// from frames whose observations nobody reads) and the sampled profile's call count.
void context_checks(lram_engine* e, Call& c) {
  const std::string w(c.who);
  LRAM_REQUIRE(e != nullptr, w + ": null engine");
  if (c.from_frames && !frames_entry(e, c)) c.in.obs = nullptr;
  step_entry(e, c.who);
  require_all_live(e, c.who);
  LRAM_REQUIRE((c.in.obs || c.in.frames) && c.in.rtg && c.in.rew, w + ": null device pointer");
  LRAM_REQUIRE(c.in.L >= 1, w + ": timesteps must be >= 1");
  const RaggedCall rc{e, w, c.in.L, c.host_lengths, c.append != 0, {}};
  if (c.ragged) rc.check(c.in.emb);
  if (c.in.frames != nullptr) check_frames_call(e, c);
  if (c.scored)
    check_score_sink(e, c.who, c.discrete, c.sink);
  else if (c.actions != nullptr)
    check_head_mode(e, c.discrete, c.who);
}

// The launches and the draw count of a call that context_checks has passed.
void context_launches(lram_engine* e, Call c, hipStream_t s) {
  const std::string w(c.who);
  RaggedCall rc{e, w, c.in.L, c.host_lengths, c.append != 0, {}};
  const bool acts = !c.scored && c.actions != nullptr;
  e->ctx_counts[0] += 1;
  Pass pass;
  pass.context = true;
  const int R = e->context_rows();
  if (!c.ragged || rc.dense()) {   // every context of full length: the dense entry's own launches
    lazy_finish_prefold(e, s);     // (only an env-step takes a tail fold over)
    timesteps_launches(e, pass, c, s);
  } else {
    rc.run(c.reset, s, [&](const ContextPlan& plan) {
      // the call-timesteps ahead of the first chunk are padding for every env: their rows of the sink take the fill values here
      // (per-chunk rows: an env is in no chunk ahead of its start, so the fill covers every call-timestep -- for env b the
      // kernel keeps to its padded rows [n_b, timesteps))
      if (c.scored)
        launch_score_fill_ragged(c.sink.actions, c.sink.tokens, c.sink.logp, plan.dev_start, R, c.in.L,
                                 plan.rows.empty() ? plan.starts[0] : c.in.L, e->cfg.act_dim, s);
      c.plan = &plan;   // (the chunks take the plan's reset masks: c.reset went into them)
      timesteps_launches(e, pass, c, s);
      if (acts)   // slots without a context: 0 / -1 in place of the head's answer to the padding
        launch_action_fill_kept(c.actions, c.tokens, plan.dev_start, R, c.in.L, e->cfg.act_dim, s);
    });
  }
  // (a score is never a draw: the sampling mode and its counter are left alone)
  if (acts) sample_draw_advance(e, s);
}

}  // namespace lram::host

namespace {

// The entries fill a Call and hand it to the body.  Contexts of observations or embeddings: kReplace and kAppend take per-env
// lengths (host_lengths must be given), kDense takes none.
enum Lengths { kDense, kReplace, kAppend };
Call vector_call(const char* who, Lengths kind, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                 const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths, const uint8_t* dev_reset_mask,
                 int32_t discrete) {
  Call c{who, Inputs{dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps}, dev_reset_mask, discrete};
  c.ragged = kind != kDense, c.host_lengths = host_lengths, c.append = kind == kAppend;
  return c;
}
// Contexts from uint8 frames, a third source of the state embeddings: per-env lengths, where given, make it a ragged or -- with
// `append` -- an append call.
Call frames_call(const char* who, const uint8_t* dev_frames, int32_t channels, int32_t height, int32_t width,
                 const float* dev_obs_seq, const float* dev_rtg_seq, const float* dev_reward_seq, int32_t timesteps,
                 const int32_t* host_lengths, int32_t append, const uint8_t* dev_reset_mask, int32_t discrete) {
  Call c{who, Inputs{dev_obs_seq, 0, dev_rtg_seq, dev_reward_seq, timesteps}, dev_reset_mask, discrete};
  c.in.frames = dev_frames, c.in.img_c = channels, c.in.img_h = height, c.in.img_w = width;
  c.from_frames = true, c.ragged = host_lengths != nullptr, c.host_lengths = host_lengths, c.append = append;
  return c;
}
// ... then either the action outputs or a sink
Call taking(Call c, float* dev_actions, int32_t* dev_tokens) {
  c.actions = dev_actions, c.tokens = dev_tokens;
  return c;
}
Call scoring(Call c, const ScoreSink& sink) {
  c.scored = true, c.sink = sink;
  return c;
}

}  // namespace

namespace lram::host {

// The frames of a stored-context call that count, and the envs that hand frames in: the image slots of a slot table (every env
// without one) among the call's rows (lram_engine::context_rows), each with its own length (null: all L).
FrameCount count_frames(const lram_engine* e, int L, const int32_t* lengths) {
  FrameCount n{0, 0};
  for (int b = 0; b < e->context_rows(); ++b)
    if (!e->slot_table || (e->slot_flags[b] & LRAM_SLOT_IMAGE)) n.n_env += 1, n.frames += lengths ? lengths[b] : L;
  return n;
}

}  // namespace lram::host

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int32_t lram_prefill(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                     const float* dev_reward_seq, int32_t timesteps, const uint8_t* dev_reset_mask, int32_t discrete,
                     float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    const Call c = vector_call("lram_prefill", kDense, dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps, nullptr,
                               dev_reset_mask, discrete);
    stored_context_call(e, taking(c, dev_actions, dev_tokens), static_cast<hipStream_t>(stream));
  });
}

int32_t lram_score(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                   const float* dev_reward_seq, int32_t timesteps, const uint8_t* dev_reset_mask, int32_t discrete,
                   const float* dev_target_actions, const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over,
                   double temperature, float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits, void* stream) {
  return guarded([&] {
    const Call c = vector_call("lram_score", kDense, dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps, nullptr,
                               dev_reset_mask, discrete);
    const ScoreSink sink{dev_actions, dev_tokens, dev_logp, dev_logits, dev_target_actions, dev_target_tokens, dev_valid, over, temperature};
    stored_context_call(e, scoring(c, sink), static_cast<hipStream_t>(stream));
  });
}

int32_t lram_prefill_ragged(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                            const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                            const uint8_t* dev_reset_mask, int32_t discrete, float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    const Call c = vector_call("lram_prefill_ragged", kReplace, dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps,
                               host_lengths, dev_reset_mask, discrete);
    stored_context_call(e, taking(c, dev_actions, dev_tokens), static_cast<hipStream_t>(stream));
  });
}

int32_t lram_score_ragged(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                          const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                          const uint8_t* dev_reset_mask, int32_t discrete, const float* dev_target_actions,
                          const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over, double temperature,
                          float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits, void* stream) {
  return guarded([&] {
    const Call c = vector_call("lram_score_ragged", kReplace, dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps,
                               host_lengths, dev_reset_mask, discrete);
    const ScoreSink sink{dev_actions, dev_tokens, dev_logp, dev_logits, dev_target_actions, dev_target_tokens, dev_valid, over, temperature};
    stored_context_call(e, scoring(c, sink), static_cast<hipStream_t>(stream));
  });
}

int32_t lram_prefill_append(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                            const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                            const uint8_t* dev_reset_mask, int32_t discrete, float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    const Call c = vector_call("lram_prefill_append", kAppend, dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps,
                               host_lengths, dev_reset_mask, discrete);
    stored_context_call(e, taking(c, dev_actions, dev_tokens), static_cast<hipStream_t>(stream));
  });
}

int32_t lram_score_append(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                          const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                          const uint8_t* dev_reset_mask, int32_t discrete, const float* dev_target_actions,
                          const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over, double temperature,
                          float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits, void* stream) {
  return guarded([&] {
    const Call c = vector_call("lram_score_append", kAppend, dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps,
                               host_lengths, dev_reset_mask, discrete);
    const ScoreSink sink{dev_actions, dev_tokens, dev_logp, dev_logits, dev_target_actions, dev_target_tokens, dev_valid, over, temperature};
    stored_context_call(e, scoring(c, sink), static_cast<hipStream_t>(stream));
  });
}

int32_t lram_prefill_frames(lram_engine* e, const uint8_t* dev_frames, int32_t channels, int32_t height, int32_t width,
                            const float* dev_obs_seq, const float* dev_rtg_seq, const float* dev_reward_seq, int32_t timesteps,
                            const int32_t* host_lengths, int32_t append, const uint8_t* dev_reset_mask, int32_t discrete,
                            float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    const Call c = frames_call("lram_prefill_frames", dev_frames, channels, height, width, dev_obs_seq, dev_rtg_seq, dev_reward_seq,
                               timesteps, host_lengths, append, dev_reset_mask, discrete);
    stored_context_call(e, taking(c, dev_actions, dev_tokens), static_cast<hipStream_t>(stream));
  });
}

int32_t lram_score_frames(lram_engine* e, const uint8_t* dev_frames, int32_t channels, int32_t height, int32_t width,
                          const float* dev_obs_seq, const float* dev_rtg_seq, const float* dev_reward_seq, int32_t timesteps,
                          const int32_t* host_lengths, int32_t append, const uint8_t* dev_reset_mask, int32_t discrete,
                          const float* dev_target_actions, const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over,
                          double temperature, float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits,
                          void* stream) {
  return guarded([&] {
    const Call c = frames_call("lram_score_frames", dev_frames, channels, height, width, dev_obs_seq, dev_rtg_seq, dev_reward_seq,
                               timesteps, host_lengths, append, dev_reset_mask, discrete);
    const ScoreSink sink{dev_actions, dev_tokens, dev_logp, dev_logits, dev_target_actions, dev_target_tokens, dev_valid, over, temperature};
    stored_context_call(e, scoring(c, sink), static_cast<hipStream_t>(stream));
  });
}

int32_t lram_context_plan(int32_t timesteps, int32_t cap, const int32_t* host_lengths, int32_t batch, int32_t* out_starts,
                          int32_t max_chunks, int32_t* out_n) {
  return guarded([&] {
    LRAM_REQUIRE(out_n != nullptr, "lram_context_plan: out_n is NULL");
    const std::vector<int> starts = context_plan(timesteps, cap, host_lengths, batch, "lram_context_plan");
    *out_n = (int32_t)starts.size();
    LRAM_REQUIRE(out_starts != nullptr && (int64_t)starts.size() <= max_chunks,
                 "lram_context_plan: the plan has " + std::to_string(starts.size()) + " chunks, out_starts holds " +
                     std::to_string(max_chunks));
    std::copy(starts.begin(), starts.end(), out_starts);
  });
}

// Which slots the stored-context and encoder entries run on: host bookkeeping only.
int32_t lram_set_context_rows(lram_engine* e, int32_t mode) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_set_context_rows: null engine");
    LRAM_REQUIRE(mode >= LRAM_CONTEXT_ROWS_ALL && mode <= LRAM_CONTEXT_ROWS_STARTED,
                 "lram_set_context_rows: mode " + std::to_string(mode) + " is outside 0 .. 2 (LRAM_CONTEXT_ROWS_ALL, _LIVE, _STARTED)");
    e->ctx_rows = mode;
  });
}

int32_t lram_get_context_rows(const lram_engine* e) { return e ? e->ctx_rows : 0; }

int32_t lram_context_counts(lram_engine* e, int64_t* out, int32_t reset) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr && out != nullptr, "lram_context_counts: null argument");
    std::copy(e->ctx_counts, e->ctx_counts + 4, out);
    if (reset) std::fill(e->ctx_counts, e->ctx_counts + 4, (int64_t)0);
  });
}

}  // extern "C"
