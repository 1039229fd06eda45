// Access to the recurrent state from outside a step: reset, whole-batch export / import, the lazy representation's peek, the
// slot table, the per-slot copy / save / load calls (slot_state.hip), and the standalone pad_obs / stream entries.
#include "engine.h"

namespace {

struct StateView {
  float* p;
  size_t n;
};
StateView state_view(const lram_engine* e, int block, int which) {
  if (block < 0 || block >= (int)e->st.size()) return {nullptr, 0};
  const BlockState& s = e->st[block];
  const bool mlstm = e->cfg.backbone == LRAM_BACKBONE_XLSTM && !e->cfg.block_is_slstm[block];
  switch (which) {
    case 0: return {s.s0.p, s.s0.n};
    case 1: return mlstm ? StateView{s.n.p, s.n.n} : StateView{nullptr, 0};
    case 2: return mlstm ? StateView{s.m.p, s.m.n} : StateView{nullptr, 0};
    case 3: return {s.conv.p, s.conv.n};
    default: return {nullptr, 0};
  }
}

}  // namespace

namespace lram::host {

// ---- state of individual env slots: host-side helpers of lram_state_copy_slots / save / load --------------------------
// Host-side rules of the index lists (the window movers of engine_window.hip take the same); `what` prefixes the message.
// dst == nullptr: one list (save / load).
void slot_lists_check(const char* what, const int32_t* src, const int32_t* dst, int n, int B, bool unique_src) {
  const std::string w(what);
  std::vector<uint8_t> seen(B, 0);   // bit 0: a source, bit 1: a destination
  for (int i = 0; i < n; ++i) {
    LRAM_REQUIRE(src[i] >= 0 && src[i] < B, w + ": slot index out of range");
    LRAM_REQUIRE(!unique_src || !(seen[src[i]] & 1), w + ": a slot is listed twice");
    seen[src[i]] |= 1;
  }
  if (dst == nullptr) return;
  for (int i = 0; i < n; ++i) {
    LRAM_REQUIRE(dst[i] >= 0 && dst[i] < B, w + ": destination slot index out of range");
    LRAM_REQUIRE(!(seen[dst[i]] & 2), w + ": a destination slot is listed twice");
    LRAM_REQUIRE(!(seen[dst[i]] & 1), w + ": a slot is both source and destination (permute by save then load)");
    seen[dst[i]] |= 2;
  }
}

}  // namespace lram::host

namespace {

SlotStateArgs slot_args(lram_engine* e, const int32_t* host_a, const int32_t* host_b, int n, hipStream_t s) {
  // (pageable host memory: the copy has read the caller's arrays when it returns; the device side is ordered on `s`)
  LRAM_HIP_CHECK(hipMemcpyAsync(e->slot_idx_dev, host_a, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (host_b)
    LRAM_HIP_CHECK(hipMemcpyAsync(e->slot_idx_dev + e->B, host_b, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SlotStateArgs a;
  a.segs = e->slot_segs_dev, a.chunks = e->slot_chunks_dev, a.n_segs = (int)e->slot_segs.size();
  a.src = e->slot_idx_dev, a.dst = host_b ? e->slot_idx_dev + e->B : nullptr, a.n = n;
  a.rec_numel = lram_state_bytes_per_env(e) / 4;
  // the lazy representation is what the state IS whenever its buffers exist and the mode is in effect (also while a graph or a
  // prefill runs the materialised kernels: the windows are then empty, which the same code handles)
  a.lazy = (e->lazy && e->lazy_ready) ? 1 : 0;
  a.parity = (int)(e->lazy_step & 1);   // what the next step reads = what the last one wrote
  return a;
}

}  // namespace

namespace lram::host {

// Records of the listed slots into dev_records (the body of lram_state_save_slots; lists checked by the caller).
void save_slot_records(lram_engine* e, const int32_t* host_slots, int n, float* dev_records, hipStream_t s) {
  lazy_finish_prefold(e, s);
  SlotStateArgs a = slot_args(e, host_slots, nullptr, n, s);
  a.n_chunks = e->slot_n_rec_chunks;
  a.records = dev_records;
  a.rec_vec = (reinterpret_cast<uintptr_t>(dev_records) & 15) == 0 ? 1 : 0;
  launch_slot_save(a, s);
  if (a.lazy) {   // C = g C_base + window, computed into the record: no fold, no write to engine state
    const size_t B = e->B, NH = e->cfg.n_heads;
    for (int i = 0; i < e->cfg.n_blocks; ++i) {
      if (e->slot_c_off[i] < 0) continue;
      BlockState& st = e->st[i];
      SlotLazySaveArgs la;
      la.C = st.s0.p, la.wk = st.wk.p, la.wv = st.wv.p;
      la.coef = st.coef.p + (size_t)a.parity * B * NH * kLazyWindow;
      la.g = st.gsc.p + (size_t)a.parity * B * NH;
      la.count = reinterpret_cast<const int32_t*>(e->LZ_COUNT.p) + (size_t)a.parity * B;
      la.slots = a.src, la.n = n, la.NH = (int)NH, la.DH = e->dh();
      la.records = dev_records, la.rec_numel = a.rec_numel, la.rec_off = e->slot_c_off[i];
      la.rec_vec = (a.rec_vec && la.rec_off % 4 == 0 && a.rec_numel % 4 == 0) ? 1 : 0;
      launch_slot_lazy_save(la, s);
    }
  }
}

// Records the engine itself saved, back into their slots (lram_prefill_ragged's kept slots): lram_state_load_slots without the
// range check of the sLSTM hidden planes, which the recurrence that produced them has kept.
void load_slot_records(lram_engine* e, const int32_t* host_slots, int n, const float* dev_records, hipStream_t s) {
  lazy_finish_prefold(e, s);
  SlotStateArgs a = slot_args(e, host_slots, nullptr, n, s);
  a.n_chunks = e->slot_n_rec_chunks;
  a.records = const_cast<float*>(dev_records);
  a.rec_vec = (reinterpret_cast<uintptr_t>(dev_records) & 15) == 0 ? 1 : 0;
  launch_slot_load(a, s);   // lazy mode: also empties the loaded slots' windows on the live side
}

}  // namespace lram::host

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int32_t lram_reset(lram_engine* e, const uint8_t* dev_env_mask, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_reset: state not allocated");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int B = e->B;
    lazy_finish_prefold(e, s);   // (a fold launched ahead of its step is completed in every block before windows are dropped)
    for (int i = 0; i < e->cfg.n_blocks; ++i) {
      if (e->compat_stale && i > 0) break;  // reference Mamba reset: layers >= 1 keep their cached state (Q1)
      BlockState& st = e->st[i];
      const bool slstm = e->cfg.backbone == LRAM_BACKBONE_XLSTM && e->cfg.block_is_slstm[i];
      if (slstm)
        launch_zero_rows(st.s0.p, dev_env_mask, B, e->cfg.d_model, 4, (int64_t)B * e->cfg.d_model, s);
      else
        launch_zero_rows(st.s0.p, dev_env_mask, B, (int64_t)(st.s0.n / B), 1, 0, s);
      if (st.n.p) launch_zero_rows(st.n.p, dev_env_mask, B, (int64_t)(st.n.n / B), 1, 0, s);
      if (st.m.p) launch_zero_rows(st.m.p, dev_env_mask, B, (int64_t)(st.m.n / B), 1, 0, s);
      launch_zero_rows(st.conv.p, dev_env_mask, B, (int64_t)(st.conv.n / B), 1, 0, s);
      if (e->lazy_ready && st.gsc.p != nullptr)  // pending window of a reset env is dropped with its C_base
        for (int p = 0; p < 2; ++p)
          launch_mlstm_lazy_clear(reinterpret_cast<int32_t*>(e->LZ_COUNT.p) + (size_t)p * B,
                                  st.gsc.p + (size_t)p * B * e->cfg.n_heads, dev_env_mask, B, e->cfg.n_heads, s);
    }
  });
}

int32_t lram_set_slot_table(lram_engine* e, const uint8_t* host_flags, const uint8_t* host_act_dim) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_set_slot_table: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE((host_flags == nullptr) == (host_act_dim == nullptr), "lram_set_slot_table: flags and act_dim go together");
    const int B = e->B;
    const lram_config& c = e->cfg;
    int n_img = 0;
    bool has_discrete = false;
    if (host_flags != nullptr) {  // validate before anything changes: a refused table leaves the one in effect as it is
      for (int b = 0; b < B; ++b) {
        const int f = host_flags[b], a = host_act_dim[b];
        const std::string at = " (slot " + std::to_string(b) + ")";
        LRAM_REQUIRE((f & ~(LRAM_SLOT_DISCRETE | LRAM_SLOT_IMAGE)) == 0, "lram_set_slot_table: unknown flag bit" + at);
        LRAM_REQUIRE(a >= 1 && a <= c.act_dim, "lram_set_slot_table: act_dim must be in 1 .. cfg.act_dim" + at);
        if (f & LRAM_SLOT_DISCRETE) {
          LRAM_REQUIRE(a == 1, "lram_set_slot_table: a discrete slot has act_dim 1" + at);
          LRAM_REQUIRE(c.n_discrete > 0, "lram_set_slot_table: a discrete slot needs n_discrete > 0" + at);
          has_discrete = true;
        }
        n_img += (f & LRAM_SLOT_IMAGE) ? 1 : 0;
      }
    }
    if (!e->mask_bits.empty()) {  // a mask in effect: the new table (or none) must leave every slot a non-empty sub-row
      const int at = e->mask_first_empty(e->mask_bits.data(), e->mask_words, host_flags);
      LRAM_REQUIRE(at < 0, "lram_set_slot_table: the action mask in effect (lram_set_action_mask) allows slot " + std::to_string(at) +
                               " nothing inside the selectable range this table gives it");
    }
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    LRAM_HIP_CHECK(hipDeviceSynchronize());  // steps in flight read the table they were launched with
    e->drop_graph();                         // the head launch and its table pointers are part of a captured step
    if (host_flags == nullptr) {
      e->drop_slot_table();
      return;
    }
    if (!e->slot_dev) LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->slot_dev), 2 * (size_t)B));
    if (!e->slot_img_list) LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->slot_img_list), sizeof(int32_t) * (size_t)B));
    e->slot_flags.assign(host_flags, host_flags + B);
    e->slot_act.assign(host_act_dim, host_act_dim + B);
    e->slot_img_prefix.assign(B + 1, 0);
    std::vector<int32_t> list;
    list.reserve(n_img);
    for (int b = 0; b < B; ++b) {
      const bool img = (host_flags[b] & LRAM_SLOT_IMAGE) != 0;
      if (img) list.push_back(b);
      e->slot_img_prefix[b + 1] = e->slot_img_prefix[b] + (img ? 1 : 0);
    }
    LRAM_HIP_CHECK(hipMemcpy(e->slot_dev, host_flags, B, hipMemcpyHostToDevice));
    LRAM_HIP_CHECK(hipMemcpy(e->slot_dev + B, host_act_dim, B, hipMemcpyHostToDevice));
    if (n_img > 0) LRAM_HIP_CHECK(hipMemcpy(e->slot_img_list, list.data(), sizeof(int32_t) * n_img, hipMemcpyHostToDevice));
    LRAM_HIP_CHECK(hipDeviceSynchronize());
    e->slot_n_image = n_img, e->slot_has_discrete = has_discrete, e->slot_table = true;
    e->sample_slot_maxima();   // which sampling slots are discrete has changed
  });
}

int32_t lram_set_action_mask(lram_engine* e, const uint32_t* host_bits, int32_t words) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_set_action_mask: state not allocated (call lram_state_alloc)");
    const int B = e->B, V = e->cfg.n_vocab, W = (V + 31) / 32;
    std::vector<uint32_t> bits;
    int no_discrete_at = -1;
    if (host_bits != nullptr) {  // validate before anything changes: a refused mask leaves the one in effect as it is
      LRAM_REQUIRE(words == W, "lram_set_action_mask: words must be ceil(n_vocab / 32) = " + std::to_string(W) + ", got " +
                                   std::to_string(words));
      bits.assign(host_bits, host_bits + (size_t)B * W);
      if (V & 31)  // bits at or above n_vocab are ignored and read back as 0
        for (int b = 0; b < B; ++b) bits[(size_t)b * W + W - 1] &= (1u << (V & 31)) - 1u;
      const int at = e->mask_first_empty(bits.data(), W, e->slot_table ? e->slot_flags.data() : nullptr);
      LRAM_REQUIRE(at < 0, "lram_set_action_mask: slot " + std::to_string(at) + " allows nothing inside its selectable range");
      for (int b = 0; b < B && no_discrete_at < 0; ++b)
        if (lram_engine::mask_count_below(bits.data(), W, b, e->cfg.n_discrete) == 0) no_discrete_at = b;
    }
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    LRAM_HIP_CHECK(hipDeviceSynchronize());  // steps in flight read the mask they were launched with
    e->drop_graph();                         // the head launch (masked or not) and its pointers are part of a captured step
    if (host_bits == nullptr) {
      e->drop_action_mask();
      return;
    }
    if (!e->mask_dev) LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->mask_dev), sizeof(uint32_t) * (size_t)B * W));
    LRAM_HIP_CHECK(hipMemcpy(e->mask_dev, bits.data(), sizeof(uint32_t) * (size_t)B * W, hipMemcpyHostToDevice));
    LRAM_HIP_CHECK(hipDeviceSynchronize());
    e->mask_bits = std::move(bits), e->mask_words = W, e->mask_no_discrete_at = no_discrete_at;
  });
}

int32_t lram_get_action_mask(lram_engine* e, uint32_t* host_bits, int32_t words, int32_t* on) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_get_action_mask: state not allocated (call lram_state_alloc)");
    const int W = (e->cfg.n_vocab + 31) / 32;
    if (host_bits != nullptr) {
      LRAM_REQUIRE(words == W, "lram_get_action_mask: words must be ceil(n_vocab / 32) = " + std::to_string(W));
      if (e->mask_bits.empty())
        std::memset(host_bits, 0, sizeof(uint32_t) * (size_t)e->B * W);
      else
        std::memcpy(host_bits, e->mask_bits.data(), sizeof(uint32_t) * (size_t)e->B * W);
    }
    if (on) *on = e->mask_bits.empty() ? 0 : 1;
  });
}

int32_t lram_get_slot_table(lram_engine* e, uint8_t* host_flags, uint8_t* host_act_dim, int32_t* n_image_slots) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_get_slot_table: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(e->slot_table, "lram_get_slot_table: no slot table is set");
    if (host_flags) std::memcpy(host_flags, e->slot_flags.data(), e->B);
    if (host_act_dim) std::memcpy(host_act_dim, e->slot_act.data(), e->B);
    if (n_image_slots) *n_image_slots = e->slot_n_image;
  });
}

int64_t lram_state_numel(const lram_engine* e, int32_t block, int32_t which) {
  if (!e || e->B <= 0) return 0;
  return (int64_t)state_view(e, block, which).n;
}

int32_t lram_state_export(lram_engine* e, int32_t block, int32_t which, float* dev_dst, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0 && dev_dst, "lram_state_export: bad argument");
    StateView v = state_view(e, block, which);
    LRAM_REQUIRE(v.p != nullptr, "lram_state_export: no such state tensor");
    lazy_materialize(e, static_cast<hipStream_t>(stream));
    LRAM_HIP_CHECK(hipMemcpyAsync(dev_dst, v.p, v.n * sizeof(float), hipMemcpyDeviceToDevice,
                                  static_cast<hipStream_t>(stream)));
  });
}

int32_t lram_state_import(lram_engine* e, int32_t block, int32_t which, const float* dev_src, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0 && dev_src, "lram_state_import: bad argument");
    StateView v = state_view(e, block, which);
    LRAM_REQUIRE(v.p != nullptr, "lram_state_import: no such state tensor");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool slstm = e->cfg.backbone == LRAM_BACKBONE_XLSTM && e->cfg.block_is_slstm[block];
    if (slstm && which == 0 && e->slstm_rinv[block].p != nullptr) {
      // The f16x2 form of the sLSTM step (slstm_seq16_kernel) keeps h_t in LDS as two binary16 planes of 2^12 h: every state the
      // recurrence itself produces has |h| < 1, a foreign one need not (|h| >= 16 overflows binary16 to inf and the next step
      // spreads NaN).  A rare call: one small reduction over the h plane [B, D] and a host synchronisation are affordable.
      LRAM_HIP_CHECK(hipSetDevice(e->device));
      const int64_t n = (int64_t)e->B * e->cfg.d_model;   // plane 0 of [4, B, D]
      int* dflag = nullptr;
      int hflag = 0;
      LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dflag), sizeof(int)));
      try {
        LRAM_HIP_CHECK(hipMemsetAsync(dflag, 0, sizeof(int), s));
        launch_slstm_h_range(dev_src, n, 15.9f, dflag, s);
        LRAM_HIP_CHECK(hipMemcpyAsync(&hflag, dflag, sizeof(int), hipMemcpyDeviceToHost, s));
        LRAM_HIP_CHECK(hipStreamSynchronize(s));
      } catch (...) {
        (void)hipFree(dflag);
        throw;
      }
      (void)hipFree(dflag);
      LRAM_REQUIRE(hflag == 0,
                   "lram_state_import: sLSTM hidden plane holds |h| >= 16 (or NaN): outside what the recurrence produces (|h| < 1) "
                   "and outside the binary16 planes of the f16x2 step kernel; import a state the model produced, or run the "
                   "engine with LRAM_SLSTM_SEQ=2 / LRAM_GEMM=f32 (exact fp32 recurrence, no range limit)");
    }
    lazy_materialize(e, s);
    LRAM_HIP_CHECK(hipMemcpyAsync(v.p, dev_src, v.n * sizeof(float), hipMemcpyDeviceToDevice, s));
  });
}

int32_t lram_lazy_peek(lram_engine* e, int32_t block, int32_t which, float* dev_dst, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0 && dev_dst, "lram_lazy_peek: bad argument");
    LRAM_REQUIRE(e->lazy && e->lazy_ready, "lram_lazy_peek: the lazy representation is not in effect");
    LRAM_REQUIRE(block >= 0 && block < e->cfg.n_blocks && !e->cfg.block_is_slstm[block] && which >= 0 && which <= 2,
                 "lram_lazy_peek: no such tensor");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    lazy_finish_prefold(e, s);   // (looks at a consistent representation: a fold launched ahead of its step is completed first)
    const size_t B = e->B, NH = e->cfg.n_heads;
    const int side = (int)(e->lazy_step & 1);  // what the next step reads = what the last one wrote
    if (which == 0) {
      LRAM_HIP_CHECK(hipMemcpyAsync(dev_dst, e->st[block].gsc.p + side * B * NH, B * NH * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else if (which == 1) {
      LRAM_HIP_CHECK(hipMemcpyAsync(dev_dst, e->st[block].m.p, B * NH * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else {
      launch_lazy_counts_as_float(reinterpret_cast<const int32_t*>(e->LZ_COUNT.p) + side * B, dev_dst, (int)B, s);
    }
  });
}

// ---- state of individual env slots (slot_state.hip) ------------------------------------------------------------------
int64_t lram_slot_state_numel(const lram_engine* e) {
  if (!e) {
    g_last_error = "lram: lram_slot_state_numel: null engine";
    return 0;
  }
  return lram_state_bytes_per_env(e) / 4;
}

int32_t lram_state_copy_slots(lram_engine* e, const int32_t* host_src, const int32_t* host_dst, int32_t n, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_state_copy_slots: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(n >= 0 && (n == 0 || (host_src && host_dst)), "lram_state_copy_slots: bad argument");
    slot_lists_check("lram_state_copy_slots", host_src, host_dst, n, e->B, false);
    if (n == 0) return;
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    lazy_finish_prefold(e, s);
    SlotStateArgs a = slot_args(e, host_src, host_dst, n, s);
    a.n_chunks = a.lazy ? e->slot_n_chunks : e->slot_n_rec_chunks;
    launch_slot_copy(a, s);
    e->parked_dirty_step = e->lazy_step;   // (a parked destination may hold a window now)
    if (a.lazy && (int)e->lazy_bound.size() == e->lazy_period) {
      // The copy carries its source's pending window into another fold class ((phase + b) % period): that class's host-side
      // bound must cover it, or the compact fold grid would skip an env whose window is about to overflow (the kernel's own
      // n_in + T > W guard only runs on the full grid).
      const int P = e->lazy_period;
      std::vector<int> before = e->lazy_bound;
      for (int i = 0; i < n; ++i)
        e->lazy_bound[host_dst[i] % P] = std::max(e->lazy_bound[host_dst[i] % P], before[host_src[i] % P]);
    }
  });
}

int32_t lram_state_swap_slots(lram_engine* e, const int32_t* host_a, const int32_t* host_b, int32_t n, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_state_swap_slots: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(n >= 0 && (n == 0 || (host_a && host_b)), "lram_state_swap_slots: bad argument");
    // (a slot on both sides, or twice on one, is refused by the copy's own rules: all 2n indices distinct and in range)
    slot_lists_check("lram_state_swap_slots", host_a, host_b, n, e->B, true);
    if (n == 0) return;
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    lazy_finish_prefold(e, s);
    SlotStateArgs a = slot_args(e, host_a, host_b, n, s);
    a.n_chunks = a.lazy ? e->slot_n_chunks : e->slot_n_rec_chunks;
    launch_slot_swap(a, s);
    e->parked_dirty_step = e->lazy_step;   // (a parked slot may hold a window now)
    if (a.lazy && (int)e->lazy_bound.size() == e->lazy_period) {
      // either slot's pending window now sits in the other's fold class: both classes' host-side bounds must cover both
      // (as a copy raises its destination's)
      const int P = e->lazy_period;
      const std::vector<int> before = e->lazy_bound;
      for (int i = 0; i < n; ++i) {
        const int ca = host_a[i] % P, cb = host_b[i] % P;
        e->lazy_bound[ca] = std::max(e->lazy_bound[ca], before[cb]);
        e->lazy_bound[cb] = std::max(e->lazy_bound[cb], before[ca]);
      }
    }
  });
}

int32_t lram_set_live(lram_engine* e, int32_t n_live, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_set_live: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(n_live >= 1 && n_live <= e->B, "lram_set_live: n_live must be in 1 .. batch = " + std::to_string(e->B));
    if (e->prefold.pending) {   // the tail fold belongs to the schedule of the rows it was launched for
      LRAM_HIP_CHECK(hipSetDevice(e->device));
      lazy_finish_prefold(e, static_cast<hipStream_t>(stream));
    }
    if (n_live == e->n_live) return;
    e->n_live = n_live;
    e->parked_dirty_step = e->lazy_step;   // (slots parked from here on hold the windows their last steps left)
    e->drop_graph();   // the captured step's launches cover the rows it was captured for
  });
}

int32_t lram_get_live(const lram_engine* e) { return e ? e->n_live : 0; }

int32_t lram_state_save_slots(lram_engine* e, const int32_t* host_slots, int32_t n, float* dev_records, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_state_save_slots: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(n >= 0 && n <= e->B && (n == 0 || (host_slots && dev_records)), "lram_state_save_slots: bad argument (at most `batch` slots per call)");
    slot_lists_check("lram_state_save_slots", host_slots, nullptr, n, e->B, false);
    if (n == 0) return;
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    save_slot_records(e, host_slots, n, dev_records, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_state_load_slots(lram_engine* e, const int32_t* host_slots, int32_t n, const float* dev_records, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_state_load_slots: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(n >= 0 && (n == 0 || (host_slots && dev_records)), "lram_state_load_slots: bad argument");
    slot_lists_check("lram_state_load_slots", host_slots, nullptr, n, e->B, true);
    if (n == 0) return;
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    lazy_finish_prefold(e, s);
    SlotStateArgs a = slot_args(e, host_slots, nullptr, n, s);
    a.n_chunks = e->slot_n_rec_chunks;
    a.records = const_cast<float*>(dev_records);
    a.rec_vec = (reinterpret_cast<uintptr_t>(dev_records) & 15) == 0 ? 1 : 0;
    if (e->slot_y_checked) {
      // lram_state_import's range rule for the sLSTM hidden planes, on the listed records only and BEFORE anything is written
      // (a rare call: one small launch and a host synchronisation are affordable)
      int* dflag = nullptr;
      int hflag = 0;
      LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dflag), sizeof(int)));
      try {
        LRAM_HIP_CHECK(hipMemsetAsync(dflag, 0, sizeof(int), s));
        launch_slot_y_range(a, 15.9f, dflag, s);
        LRAM_HIP_CHECK(hipMemcpyAsync(&hflag, dflag, sizeof(int), hipMemcpyDeviceToHost, s));
        LRAM_HIP_CHECK(hipStreamSynchronize(s));
      } catch (...) {
        (void)hipFree(dflag);
        throw;
      }
      (void)hipFree(dflag);
      LRAM_REQUIRE(hflag == 0,
                   "lram_state_load_slots: an sLSTM hidden plane holds |h| >= 16 (or NaN): outside what the recurrence produces "
                   "(|h| < 1) and outside the binary16 planes of the f16x2 step kernel (see lram_state_import)");
    }
    launch_slot_load(a, s);   // lazy mode: also empties the loaded slots' windows on the live side
  });
}

int32_t lram_pad_obs(const float* dev_native, int32_t n_native, const int32_t* dev_inv_index, const float* dev_mean,
                     const float* dev_std, float* dev_out, int32_t batch, int32_t state_dim, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(dev_native && dev_out && batch > 0 && state_dim > 0 && n_native > 0, "lram_pad_obs: bad argument");
    LRAM_REQUIRE(dev_inv_index != nullptr || n_native <= state_dim, "lram_pad_obs: observation wider than state_dim");
    LRAM_REQUIRE((dev_mean == nullptr) == (dev_std == nullptr), "lram_pad_obs: mean and std go together");
    launch_pad_obs(dev_native, n_native, dev_inv_index, dev_mean, dev_std, dev_out, batch, state_dim,
                   static_cast<hipStream_t>(stream));
  });
}

int32_t lram_pad_obs_slots(const float* dev_native, int32_t n_native, const int32_t* dev_slot_row, const int32_t* dev_inv_index,
                           const float* dev_mean, const float* dev_std, int32_t n_rows, float* dev_out, int32_t batch,
                           int32_t state_dim, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(dev_native && dev_out && dev_slot_row && batch > 0 && state_dim > 0 && n_native > 0 && n_rows > 0,
                 "lram_pad_obs_slots: bad argument");
    LRAM_REQUIRE(dev_inv_index != nullptr || n_native <= state_dim, "lram_pad_obs_slots: observation wider than state_dim");
    LRAM_REQUIRE((dev_mean == nullptr) == (dev_std == nullptr), "lram_pad_obs_slots: mean and std go together");
    launch_pad_obs_slots(dev_native, n_native, dev_slot_row, dev_inv_index, dev_mean, dev_std, n_rows, dev_out, batch,
                         state_dim, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_stream_copy(float* dev_dst, const float* dev_src, size_t numel, void* stream) {
  // (standalone measurement entry: its knob as the environment has it now)
  return guarded([&] { launch_stream_copy(dev_dst, dev_src, numel, static_cast<hipStream_t>(stream), env_int("LRAM_COPY_VARIANT", 4)); });
}

int32_t lram_stream_read(const float* dev_buf, size_t numel, float* dev_sink, void* stream) {
  return guarded([&] { launch_stream_read(dev_buf, numel, dev_sink, static_cast<hipStream_t>(stream), env_int("LRAM_READ_VARIANT", 1804)); });
}

int32_t lram_stream_rmw(float* dev_buf, size_t numel, void* stream) {
  return guarded([&] { launch_stream_rmw(dev_buf, numel, static_cast<hipStream_t>(stream)); });
}

}  // extern "C"
