// Context-window inference, the reference's cache-off evaluation (use_inference_cache = False, its default): at every env-step
// the model runs from an empty state over the env's last K timesteps.  The engine keeps those timesteps in a ring per env slot
// (window_kernels.hip), maintains it as the evaluation loop maintains its lists (reward patch, relabel, keep, push), lays the
// windows out and hands them to the stored-context body (engine_context.hip): lram_window_alloc, lram_window_set_pad,
// lram_step_window, lram_window_peek.  Every slot has its own ring position, so a step may run the live prefix alone
// (lram_window_set_slots) and whole windows move between slots and records (lram_window_copy_slots / _swap_slots / _save_slots /
// _load_slots).
// Calls the stored-context checks and launches, gemm, and the slot movers' list rules (engine_state.hip).
#include "engine.h"

namespace {

int32_t* ctl_patch(lram_engine* e) { return reinterpret_cast<int32_t*>(e->WIN_CTL.p); }
int32_t* ctl_relabel(lram_engine* e) { return ctl_patch(e) + e->B; }
int32_t* ctl_count(lram_engine* e) { return ctl_patch(e) + 2 * (size_t)e->B; }
int32_t* ctl_pos(lram_engine* e) { return ctl_patch(e) + 3 * (size_t)e->B; }
uint8_t* ctl_ones(lram_engine* e) { return reinterpret_cast<uint8_t*>(ctl_patch(e) + 4 * (size_t)e->B); }
float* ring_rtg(lram_engine* e) { return e->WIN_RING_SC.p; }
float* ring_rew(lram_engine* e) { return e->WIN_RING_SC.p + (size_t)e->B * e->win_K; }

// What every window entry asks of the engine before it looks at its own arguments.
void window_entry(const lram_engine* e, const std::string& w) {
  LRAM_REQUIRE(e != nullptr, w + ": null engine");
  LRAM_REQUIRE(e->B > 0, w + ": state not allocated (call lram_state_alloc)");
  LRAM_REQUIRE(e->win_K > 0, w + ": no window ring is allocated (call lram_window_alloc)");
}

// The state Linear over `rows` observations [rows, state_dim] into rows of pitch ldc: what context_embeddings does for SEQ_EMB.
void embed_states(lram_engine* e, const float* obs, int rows, float* out, int64_t ldc, hipStream_t s) {
  const lram_config& c = e->cfg;
  GemmArgs ge;
  ge.a = obs, ge.lda = c.state_dim, ge.w = e->w_state, ge.ldw = c.state_dim, ge.c = out, ge.ldc = ldc;
  ge.bias = e->b_state, ge.m = rows, ge.n = c.d_model, ge.k = c.state_dim;
  gemm(e, ge, s);
}

// The host's counts and positions of every slot onto the device, behind whatever `s` holds: a mover has changed them.
// (pageable host memory: the copy has read the vectors when it returns)
void upload_counts(lram_engine* e, hipStream_t s) {
  const size_t bytes = (size_t)e->B * sizeof(int32_t);
  LRAM_HIP_CHECK(hipMemcpyAsync(ctl_count(e), e->win_count.data(), bytes, hipMemcpyHostToDevice, s));
  LRAM_HIP_CHECK(hipMemcpyAsync(ctl_pos(e), e->win_pos.data(), bytes, hipMemcpyHostToDevice, s));
}

// The caller's index lists onto the device (lram_engine::slot_idx_dev, [2][B], stream-ordered as the state movers use it).
void upload_lists(lram_engine* e, const int32_t* host_a, const int32_t* host_b, int n, hipStream_t s) {
  LRAM_HIP_CHECK(hipMemcpyAsync(e->slot_idx_dev, host_a, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (host_b)
    LRAM_HIP_CHECK(hipMemcpyAsync(e->slot_idx_dev + e->B, host_b, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
}

int64_t record_numel(const lram_engine* e) { return (int64_t)e->win_K * (e->cfg.d_model + 2) + 1; }

// A window step of the live prefix runs the stored-context body on it: the context-rows mode is LIVE for the length of the call.
struct LiveRows {
  lram_engine* e;
  int was;
  LiveRows(lram_engine* e_, bool live) : e(e_), was(e_->ctx_rows) {
    if (live) e->ctx_rows = LRAM_CONTEXT_ROWS_LIVE;
  }
  ~LiveRows() { e->ctx_rows = was; }
};

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int32_t lram_window_alloc(lram_engine* e, int32_t timesteps) {
  return guarded([&] {
    const std::string w("lram_window_alloc");
    LRAM_REQUIRE(e != nullptr, w + ": null engine");
    LRAM_REQUIRE(e->B > 0, w + ": state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(timesteps >= 0, w + ": timesteps must be >= 1 (0 frees the ring)");
    const lram_config& c = e->cfg;
    const size_t B = (size_t)e->B, K = (size_t)timesteps, D = (size_t)c.d_model;
    if (timesteps > 0) {
      LRAM_REQUIRE(c.tokens_per_step == 3, w + ": the (state, rtg, reward) front end needs tokens_per_step == 3");
      LRAM_REQUIRE(c.d_model % 4 == 0, w + ": the window ring needs d_model to be a multiple of 4 (its kernels move float4)");
      LRAM_REQUIRE(B * K * D <= ((size_t)1 << 29), w + ": the [batch, timesteps, d_model] windows exceed 2 GiB");
    }
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    LRAM_HIP_CHECK(hipDeviceSynchronize());
    e->drop_window();   // (also: slots mode back to LRAM_WINDOW_SLOTS_SHARED)
    if (timesteps == 0) return;
    e->WIN_RING_EMB.alloc(B * K * D), e->WIN_EMB.alloc(B * K * D);
    e->WIN_RING_SC.alloc(2 * B * K), e->WIN_SC.alloc(2 * B * K);
    e->WIN_PAD.alloc(D);
    e->WIN_CTL.alloc(4 * B + (B + 3) / 4);
    // (zeroed: nothing of it is read before it is written, and a peek of an untouched ring must not depend on the allocator)
    for (DevBuf* b : {&e->WIN_RING_EMB, &e->WIN_RING_SC, &e->WIN_EMB, &e->WIN_SC, &e->WIN_PAD, &e->WIN_CTL}) b->zero();
    e->win_K = timesteps, e->win_pad_set = false;
    e->win_count.assign(B, 0);
    e->win_pos.assign(B, timesteps - 1);
    upload_counts(e, nullptr);
    LRAM_HIP_CHECK(hipMemsetAsync(ctl_ones(e), 1, B, nullptr));
    LRAM_HIP_CHECK(hipDeviceSynchronize());
  });
}

int32_t lram_window_set_pad(lram_engine* e, const float* dev_pad_obs, int32_t obs_is_embedding, void* stream) {
  return guarded([&] {
    const std::string w("lram_window_set_pad");
    window_entry(e, w);
    LRAM_REQUIRE(dev_pad_obs != nullptr, w + ": dev_pad_obs is NULL");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (obs_is_embedding)
      LRAM_HIP_CHECK(hipMemcpyAsync(e->WIN_PAD.p, dev_pad_obs, sizeof(float) * e->cfg.d_model, hipMemcpyDeviceToDevice, s));
    else
      embed_states(e, dev_pad_obs, 1, e->WIN_PAD.p, e->cfg.d_model, s);
    e->win_pad_set = true;
  });
}

// Which slots a window step runs: host bookkeeping only.
int32_t lram_window_set_slots(lram_engine* e, int32_t mode) {
  return guarded([&] {
    window_entry(e, "lram_window_set_slots");
    LRAM_REQUIRE(mode == LRAM_WINDOW_SLOTS_SHARED || mode == LRAM_WINDOW_SLOTS_OWN,
                 "lram_window_set_slots: mode " + std::to_string(mode) + " is neither LRAM_WINDOW_SLOTS_SHARED (0) nor LRAM_WINDOW_SLOTS_OWN (1)");
    e->win_own = mode == LRAM_WINDOW_SLOTS_OWN;
  });
}

int32_t lram_window_get_slots(const lram_engine* e) { return e && e->win_own ? LRAM_WINDOW_SLOTS_OWN : LRAM_WINDOW_SLOTS_SHARED; }

int32_t lram_step_window(lram_engine* e, const float* dev_obs, int32_t obs_is_embedding, const float* dev_rtg,
                         const float* dev_prev_reward, const uint8_t* host_reset, const int32_t* host_relabel,
                         const int32_t* host_keep, int32_t pad_mode, int32_t discrete, float* dev_actions, int32_t* dev_tokens,
                         void* stream) {
  return guarded([&] {
    const std::string w("lram_step_window");
    window_entry(e, w);
    const lram_config& c = e->cfg;
    const int B = e->B, K = e->win_K, D = c.d_model;
    // ---- the refusals: nothing is launched, the ring, its counts and positions and the recurrent state stay as they are ----
    LRAM_REQUIRE(dev_obs && dev_rtg && dev_prev_reward && dev_actions, w + ": null device pointer");
    LRAM_REQUIRE(pad_mode == LRAM_WINDOW_PAD_REFERENCE || pad_mode == LRAM_WINDOW_PAD_NONE,
                 w + ": pad_mode " + std::to_string(pad_mode) + " is neither LRAM_WINDOW_PAD_REFERENCE (0) nor LRAM_WINDOW_PAD_NONE (1)");
    LRAM_REQUIRE(pad_mode != LRAM_WINDOW_PAD_REFERENCE || e->win_pad_set,
                 w + ": LRAM_WINDOW_PAD_REFERENCE needs the pad entry (call lram_window_set_pad)");
    LRAM_REQUIRE(e->ctx_rows == LRAM_CONTEXT_ROWS_ALL,
                 w + ": the context-rows mode is not LRAM_CONTEXT_ROWS_ALL (lram_set_context_rows): a window step runs every slot");
    LRAM_REQUIRE(e->win_own || e->n_live == B,
                 w + ": " + std::to_string(B - e->n_live) + " of " + std::to_string(B) +
                     " env slots are parked (lram_set_live): a window step runs every slot (LRAM_WINDOW_SLOTS_OWN lifts this)");
    LRAM_REQUIRE(e->compat_repeat <= 1 && !e->compat_stale,
                 w + ": a Mamba reference-trajectory mode is on (lram_set_compat_mode): its trajectories are those of the cached path");
    const int R = e->n_live;   // the rows of the call: every slot, or (LRAM_WINDOW_SLOTS_OWN) the live prefix
    // patch | relabel | count | pos, as WIN_CTL holds them: [B] each -- a parked slot is patched and relabelled by nobody and keeps
    // its count and position
    std::vector<int32_t> ctl(4 * (size_t)B, 0);
    std::copy(e->win_count.begin(), e->win_count.end(), ctl.begin() + 2 * (size_t)B);
    std::copy(e->win_pos.begin(), e->win_pos.end(), ctl.begin() + 3 * (size_t)B);
    for (int b = 0; b < R; ++b) {
      const bool reset = host_reset != nullptr && host_reset[b] != 0;
      const int m = host_relabel ? host_relabel[b] : 0, keep = host_keep ? host_keep[b] : 0;
      LRAM_REQUIRE(m >= 0, w + ": relabel " + std::to_string(m) + " of env slot " + std::to_string(b) + " is negative");
      LRAM_REQUIRE(keep >= 0, w + ": keep " + std::to_string(keep) + " of env slot " + std::to_string(b) + " is negative");
      LRAM_REQUIRE(!(reset && m > 0), w + ": env slot " + std::to_string(b) + " is reset and relabelled (relabel " +
                                          std::to_string(m) + "): a reset drops the entries a relabel would rewrite");
      int n = reset ? 0 : e->win_count[b];
      ctl[b] = !reset && n > 0;
      ctl[(size_t)B + b] = std::min(m, n);
      if (keep > 0) n = std::min(n, keep);
      ctl[2 * (size_t)B + b] = std::min(n + 1, K);
      ctl[3 * (size_t)B + b] = (e->win_pos[b] + 1) % K;   // where this call pushes: the newest entry from here on
    }
    const bool ragged = pad_mode == LRAM_WINDOW_PAD_NONE;
    const int32_t* count = ctl.data() + 2 * (size_t)B;
    Call call{"lram_step_window", Inputs{e->WIN_EMB.p, 1, e->WIN_SC.p, e->WIN_SC.p + (size_t)B * K, K}, ctl_ones(e), discrete,
              dev_actions, dev_tokens};
    call.ragged = ragged, call.host_lengths = ragged ? count : nullptr;
    const LiveRows rows(e, R < B);   // (the stored-context body's rows, inputs and outputs: the R rows of this call)
    context_checks(e, call);   // (tokens_per_step, d_model % 4, the head mode and whatever else lram_prefill[_ragged] refuses)
    // ---- from here on the call launches ----
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (pageable host memory: the copy has read `ctl` when it returns; the device side is ordered on `s`)
    LRAM_HIP_CHECK(hipMemcpyAsync(ctl_patch(e), ctl.data(), ctl.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    launch_window_update(ring_rtg(e), ring_rew(e), dev_prev_reward, dev_rtg, ctl_patch(e), ctl_relabel(e), ctl_pos(e), R, K, s);
    const float* emb = dev_obs;
    if (!obs_is_embedding) {   // the state Linear's rows [R, D] rest in the head of WIN_EMB, which the gather below rewrites
      embed_states(e, dev_obs, R, e->WIN_EMB.p, D, s);
      emb = e->WIN_EMB.p;
    }
    launch_window_push_rows(e->WIN_RING_EMB.p, emb, ctl_pos(e), R, K, D, s);
    // (host and device counts and positions move together, here: should the launches below run out of memory, the ring has taken
    // the timestep and says so -- include/lram_hip.h)
    std::copy(count, count + B, e->win_count.begin());
    std::copy(ctl.begin() + 3 * (size_t)B, ctl.end(), e->win_pos.begin());
    // the entries of per-env length read left-aligned rows; the dense entry reads the windows end-aligned behind the pad entry
    launch_window_gather(e->WIN_EMB.p, e->WIN_SC.p, e->WIN_SC.p + (size_t)B * K, e->WIN_RING_EMB.p, ring_rtg(e), ring_rew(e),
                         ctl_count(e), ctl_pos(e), ragged ? nullptr : e->WIN_PAD.p, ragged, R, K, D, s);
    context_launches(e, call, s);
  });
}

int32_t lram_window_peek(lram_engine* e, float* dev_emb, float* dev_rtg, float* dev_reward, int32_t* host_counts, void* stream) {
  return guarded([&] {
    window_entry(e, "lram_window_peek");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    launch_window_gather(dev_emb, dev_rtg, dev_reward, e->WIN_RING_EMB.p, ring_rtg(e), ring_rew(e), ctl_count(e), ctl_pos(e), nullptr,
                         false, e->B, e->win_K, e->cfg.d_model, static_cast<hipStream_t>(stream));
    if (host_counts != nullptr) std::copy(e->win_count.begin(), e->win_count.end(), host_counts);
  });
}

// ---- windows of individual env slots ------------------------------------------------------------------------------------
int32_t lram_window_copy_slots(lram_engine* e, const int32_t* host_src, const int32_t* host_dst, int32_t n, void* stream) {
  return guarded([&] {
    const char* w = "lram_window_copy_slots";
    window_entry(e, w);
    LRAM_REQUIRE(n >= 0 && (n == 0 || (host_src && host_dst)), std::string(w) + ": bad argument");
    slot_lists_check(w, host_src, host_dst, n, e->B, false);
    if (n == 0) return;
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    upload_lists(e, host_src, host_dst, n, s);
    launch_window_move(e->WIN_RING_EMB.p, ring_rtg(e), ring_rew(e), e->slot_idx_dev, e->slot_idx_dev + e->B, n, false, e->win_K,
                       e->cfg.d_model, s);
    for (int i = 0; i < n; ++i)   // (no destination is a source: the order does not matter)
      e->win_count[host_dst[i]] = e->win_count[host_src[i]], e->win_pos[host_dst[i]] = e->win_pos[host_src[i]];
    upload_counts(e, s);
  });
}

int32_t lram_window_swap_slots(lram_engine* e, const int32_t* host_a, const int32_t* host_b, int32_t n, void* stream) {
  return guarded([&] {
    const char* w = "lram_window_swap_slots";
    window_entry(e, w);
    LRAM_REQUIRE(n >= 0 && (n == 0 || (host_a && host_b)), std::string(w) + ": bad argument");
    slot_lists_check(w, host_a, host_b, n, e->B, true);   // (all 2n indices distinct and in range)
    if (n == 0) return;
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    upload_lists(e, host_a, host_b, n, s);
    launch_window_move(e->WIN_RING_EMB.p, ring_rtg(e), ring_rew(e), e->slot_idx_dev, e->slot_idx_dev + e->B, n, true, e->win_K,
                       e->cfg.d_model, s);
    for (int i = 0; i < n; ++i) {
      std::swap(e->win_count[host_a[i]], e->win_count[host_b[i]]);
      std::swap(e->win_pos[host_a[i]], e->win_pos[host_b[i]]);
    }
    upload_counts(e, s);
  });
}

int64_t lram_window_slot_numel(const lram_engine* e) {
  if (!e || e->win_K <= 0) {
    g_last_error = "lram: lram_window_slot_numel: no window ring is allocated (call lram_window_alloc)";
    return 0;
  }
  return record_numel(e);
}

int32_t lram_window_save_slots(lram_engine* e, const int32_t* host_slots, int32_t n, float* dev_records, void* stream) {
  return guarded([&] {
    const char* w = "lram_window_save_slots";
    window_entry(e, w);
    LRAM_REQUIRE(n >= 0 && n <= e->B && (n == 0 || (host_slots && dev_records)),
                 std::string(w) + ": bad argument (at most `batch` slots per call)");
    slot_lists_check(w, host_slots, nullptr, n, e->B, false);
    if (n == 0) return;
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    upload_lists(e, host_slots, nullptr, n, s);
    launch_window_save(dev_records, e->WIN_RING_EMB.p, ring_rtg(e), ring_rew(e), ctl_count(e), ctl_pos(e), e->slot_idx_dev, n,
                       e->win_K, e->cfg.d_model, s);
  });
}

int32_t lram_window_load_slots(lram_engine* e, const int32_t* host_slots, int32_t n, const float* dev_records, void* stream) {
  return guarded([&] {
    const std::string w("lram_window_load_slots");
    window_entry(e, w);
    LRAM_REQUIRE(n >= 0 && (n == 0 || (host_slots && dev_records)), w + ": bad argument");
    slot_lists_check(w.c_str(), host_slots, nullptr, n, e->B, true);
    if (n == 0) return;
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // The host steers every later step by the counts, and they arrive in the records: one strided read-back of n floats and a
    // synchronisation of `s` (a rare call, as lram_state_load_slots' range check is) -- BEFORE anything is written.
    const int K = e->win_K;
    const int64_t rec = record_numel(e);
    std::vector<float> counts((size_t)n);
    LRAM_HIP_CHECK(hipMemcpy2DAsync(counts.data(), sizeof(float), dev_records + (rec - 1), (size_t)rec * sizeof(float), sizeof(float),
                                    (size_t)n, hipMemcpyDeviceToHost, s));
    LRAM_HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i)
      LRAM_REQUIRE(counts[i] >= 0.f && counts[i] <= (float)K && counts[i] == (float)(int)counts[i],
                   w + ": record " + std::to_string(i) + " does not end in a count in 0 .. timesteps = " + std::to_string(K) +
                       " (a record of lram_window_save_slots from a ring of the same timesteps and d_model)");
    upload_lists(e, host_slots, nullptr, n, s);
    launch_window_load(e->WIN_RING_EMB.p, ring_rtg(e), ring_rew(e), dev_records, e->slot_idx_dev, n, K, e->cfg.d_model, s);
    for (int i = 0; i < n; ++i) e->win_count[host_slots[i]] = (int)counts[i], e->win_pos[host_slots[i]] = K - 1;
    upload_counts(e, s);
  });
}

}  // extern "C"
