// Context-window inference, the reference's cache-off evaluation (use_inference_cache = False, its default): at every env-step
// the model runs from an empty state over the env's last K timesteps.  The engine keeps those timesteps in a ring per env slot
// (window_kernels.hip), maintains it as the evaluation loop maintains its lists (reward patch, relabel, keep, push), lays the
// windows out and hands them to the stored-context body (engine_context.hip): lram_window_alloc, lram_window_set_pad,
// lram_step_window, lram_window_peek.
// Calls the stored-context checks and launches and gemm.
#include "engine.h"

namespace {

int32_t* ctl_patch(lram_engine* e) { return reinterpret_cast<int32_t*>(e->WIN_CTL.p); }
int32_t* ctl_relabel(lram_engine* e) { return ctl_patch(e) + e->B; }
int32_t* ctl_count(lram_engine* e) { return ctl_patch(e) + 2 * (size_t)e->B; }
uint8_t* ctl_ones(lram_engine* e) { return reinterpret_cast<uint8_t*>(ctl_patch(e) + 3 * (size_t)e->B); }
float* ring_rtg(lram_engine* e) { return e->WIN_RING_SC.p; }
float* ring_rew(lram_engine* e) { return e->WIN_RING_SC.p + (size_t)e->B * e->win_K; }
int ring_newest(const lram_engine* e) { return (e->win_head + e->win_K - 1) % e->win_K; }

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
    e->drop_window();
    if (timesteps == 0) return;
    e->WIN_RING_EMB.alloc(B * K * D), e->WIN_EMB.alloc(B * K * D);
    e->WIN_RING_SC.alloc(2 * B * K), e->WIN_SC.alloc(2 * B * K);
    e->WIN_PAD.alloc(D);
    e->WIN_CTL.alloc(3 * B + (B + 3) / 4);
    // (zeroed: nothing of it is read before it is written, and a peek of an untouched ring must not depend on the allocator)
    for (DevBuf* b : {&e->WIN_RING_EMB, &e->WIN_RING_SC, &e->WIN_EMB, &e->WIN_SC, &e->WIN_PAD, &e->WIN_CTL}) b->zero();
    e->win_K = timesteps, e->win_head = 0, e->win_pad_set = false;
    e->win_count.assign(B, 0);
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

int32_t lram_step_window(lram_engine* e, const float* dev_obs, int32_t obs_is_embedding, const float* dev_rtg,
                         const float* dev_prev_reward, const uint8_t* host_reset, const int32_t* host_relabel,
                         const int32_t* host_keep, int32_t pad_mode, int32_t discrete, float* dev_actions, int32_t* dev_tokens,
                         void* stream) {
  return guarded([&] {
    const std::string w("lram_step_window");
    window_entry(e, w);
    const lram_config& c = e->cfg;
    const int B = e->B, K = e->win_K, D = c.d_model;
    // ---- the refusals: nothing is launched, the ring, its counts and the recurrent state stay as they are ----
    LRAM_REQUIRE(dev_obs && dev_rtg && dev_prev_reward && dev_actions, w + ": null device pointer");
    LRAM_REQUIRE(pad_mode == LRAM_WINDOW_PAD_REFERENCE || pad_mode == LRAM_WINDOW_PAD_NONE,
                 w + ": pad_mode " + std::to_string(pad_mode) + " is neither LRAM_WINDOW_PAD_REFERENCE (0) nor LRAM_WINDOW_PAD_NONE (1)");
    LRAM_REQUIRE(pad_mode != LRAM_WINDOW_PAD_REFERENCE || e->win_pad_set,
                 w + ": LRAM_WINDOW_PAD_REFERENCE needs the pad entry (call lram_window_set_pad)");
    LRAM_REQUIRE(e->ctx_rows == LRAM_CONTEXT_ROWS_ALL,
                 w + ": the context-rows mode is not LRAM_CONTEXT_ROWS_ALL (lram_set_context_rows): a window step runs every slot");
    LRAM_REQUIRE(e->n_live == B, w + ": " + std::to_string(B - e->n_live) + " of " + std::to_string(B) +
                                     " env slots are parked (lram_set_live): a window step runs every slot");
    LRAM_REQUIRE(e->compat_repeat <= 1 && !e->compat_stale,
                 w + ": a Mamba reference-trajectory mode is on (lram_set_compat_mode): its trajectories are those of the cached path");
    std::vector<int32_t> ctl(3 * (size_t)B);   // patch | relabel | count, as WIN_CTL holds them
    for (int b = 0; b < B; ++b) {
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
    }
    const bool ragged = pad_mode == LRAM_WINDOW_PAD_NONE;
    const int32_t* count = ctl.data() + 2 * (size_t)B;
    Call call{"lram_step_window", Inputs{e->WIN_EMB.p, 1, e->WIN_SC.p, e->WIN_SC.p + (size_t)B * K, K}, ctl_ones(e), discrete,
              dev_actions, dev_tokens};
    call.ragged = ragged, call.host_lengths = ragged ? count : nullptr;
    context_checks(e, call);   // (tokens_per_step, d_model % 4, the head mode and whatever else lram_prefill[_ragged] refuses)
    // ---- from here on the call launches ----
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int head = e->win_head;
    // (pageable host memory: the copy has read `ctl` when it returns; the device side is ordered on `s`)
    LRAM_HIP_CHECK(hipMemcpyAsync(ctl_patch(e), ctl.data(), ctl.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    launch_window_update(ring_rtg(e), ring_rew(e), dev_prev_reward, dev_rtg, ctl_patch(e), ctl_relabel(e), head, B, K, s);
    if (obs_is_embedding)
      launch_window_push_rows(e->WIN_RING_EMB.p, dev_obs, head, B, K, D, s);
    else
      embed_states(e, dev_obs, B, e->WIN_RING_EMB.p + (size_t)head * D, (int64_t)K * D, s);
    // (host and device counts move together, here: should the launches below run out of memory, the ring has taken the timestep
    // and says so -- include/lram_hip.h)
    std::copy(count, count + B, e->win_count.begin());
    e->win_head = (head + 1) % K;
    // the entries of per-env length read left-aligned rows; the dense entry reads the windows end-aligned behind the pad entry
    launch_window_gather(e->WIN_EMB.p, e->WIN_SC.p, e->WIN_SC.p + (size_t)B * K, e->WIN_RING_EMB.p, ring_rtg(e), ring_rew(e),
                         ctl_count(e), ragged ? nullptr : e->WIN_PAD.p, ragged, head, B, K, D, s);
    context_launches(e, call, s);
  });
}

int32_t lram_window_peek(lram_engine* e, float* dev_emb, float* dev_rtg, float* dev_reward, int32_t* host_counts, void* stream) {
  return guarded([&] {
    window_entry(e, "lram_window_peek");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    launch_window_gather(dev_emb, dev_rtg, dev_reward, e->WIN_RING_EMB.p, ring_rtg(e), ring_rew(e), ctl_count(e), nullptr, false,
                         ring_newest(e), e->B, e->win_K, e->cfg.d_model, static_cast<hipStream_t>(stream));
    if (host_counts != nullptr) std::copy(e->win_count.begin(), e->win_count.end(), host_counts);
  });
}

}  // extern "C"
