// Stream plumbing of the engine: its events, the env slices of a call and their fork / join with the caller's stream, and the
// profiler of the dominant recurrent kernel.  Calls into no other engine file.
#include "engine.h"

namespace lram::host {

void prof_record(lram_engine* e, hipStream_t s, bool start, bool aux) {
  if (!e->prof_on || !e->prof_live) return;
  if (start) {
    if (e->prof_used == e->prof_events.size()) {
      hipEvent_t a, b;
      // (timing only: no system-scope fence -- the header's own advice for events that measure)
      const unsigned flags = e->event_device_scope ? hipEventDisableSystemFence : hipEventDefault;
      LRAM_HIP_CHECK(hipEventCreateWithFlags(&a, flags));
      LRAM_HIP_CHECK(hipEventCreateWithFlags(&b, flags));
      e->prof_events.emplace_back(a, b);
      e->prof_aux.push_back(0);
    }
    e->prof_aux[e->prof_used] = aux ? 1 : 0;
    LRAM_HIP_CHECK(hipEventRecord(e->prof_events[e->prof_used].first, s));
  } else {
    LRAM_HIP_CHECK(hipEventRecord(e->prof_events[e->prof_used].second, s));
    ++e->prof_used;
  }
}

// An ordering event (no timing) for the engine's internal edges or for the boundary with the caller's stream.
// boundary = false: both streams are the engine's own (slice streams, state-pass stream).  Those events are created with
// hipEventDisableSystemFence: a default event performs a SYSTEM-scope release / acquire when it is recorded -- cache write-back
// and invalidation for the host's and other devices' benefit -- ~150 times per env-step, between kernels of one device whose
// launches already order their memory at device scope.  boundary = true (fork from / join into the caller's stream): default
// events, the caller may hand the results to a copy engine or the host next.
hipEvent_t new_event(const lram_engine* e, bool boundary) {
  hipEvent_t nev;
  unsigned flags = hipEventDisableTiming;
  if (!boundary && e->event_device_scope) flags |= hipEventDisableSystemFence;
  LRAM_HIP_CHECK(hipEventCreateWithFlags(&nev, flags));
  return nev;
}

// The next event of the engine's own ring (device scope; boundary: of the ring of fork / join events), also for a record / wait
// pair placed apart.
// ring of events: a wait captures the record that precedes it at call time, so re-recording an event later
// (next timestep / next call) cannot disturb waits that are already enqueued
hipEvent_t ring_event(lram_engine* e, bool boundary) {
  constexpr size_t kRing = 512;
  std::vector<hipEvent_t>& pool = boundary ? e->edge_events : e->sync_events;
  size_t& used = boundary ? e->edge_used : e->sync_used;
  if (pool.size() < kRing && used >= pool.size()) pool.push_back(new_event(e, boundary));
  return pool[used++ % pool.size()];
}

// `dst` waits for everything enqueued so far on `src` (event from the engine's pool; also legal under
// stream capture, where it becomes a graph edge).
void stream_after(lram_engine* e, hipStream_t dst, hipStream_t src, bool boundary) {
  if (dst == src) return;
  hipEvent_t ev = ring_event(e, boundary);
  LRAM_HIP_CHECK(hipEventRecord(ev, src));
  LRAM_HIP_CHECK(hipStreamWaitEvent(dst, ev, 0));
}

// Slices for this call: they cut the live prefix [0, n_live) (lram_set_live; the whole batch unless the caller parked slots), and the
// rules below are judged on its rows.  One slice on the caller's stream unless micro-batching is on: then n_micro slices on
// engine-owned streams plus one stream that serialises the HBM-bound cell kernels (see run_xlstm_stack).
std::vector<Slice> make_slices(lram_engine* e, hipStream_t s, hipStream_t* hbm) {
  int n = e->n_micro;
  if (n == 0) {
    // auto: two slices where the second one has something long to hide behind.  xLSTM: one mLSTM block's matrix memory over the
    // batch of at least 512 MiB (16M from 512 env slots, 206M from 82); Mamba: from 1024 env slots.  Round 6, one box, one vs two
    // slices, env-steps/s: 206M at 64 / 96 / 128 / 256 envs 15.1k vs 14.9k / 18.5k vs 18.5k / 21.1k vs 21.6k / 25.1k vs 29.1k
    // (rounds 2-5 split from 512 envs only); 16M at 256 / 512 / 640 envs 219.8k vs 194.1k / 296.2k vs 297.1k / 304.8k vs 314.1k;
    // Mamba-48M at 512 / 768 / 1024 / 1536 envs 288.6k vs 275.0k / 380.4k vs 367.7k / 410.5k vs 416.9k / 432.8k vs 479.4k.
    if (e->cfg.backbone == LRAM_BACKBONE_MAMBA) {
      n = e->n_live >= 1024 ? 2 : 1;
    } else {
      n = mlstm_live_bytes(e) >= 512.0 * 1024 * 1024 ? 2 : 1;
    }
  }
  if (e->graph_mode) n = 1;  // graph replay targets small, launch-bound batches: one slice, one stream
  n = std::max(1, std::min(n, std::min(e->n_live, 8)));
  *hbm = s;
  if (n == 1) return {Slice{0, e->n_live, s}};
  while ((int)e->micro_streams.size() < n) {
    hipStream_t ns;
    LRAM_HIP_CHECK(hipStreamCreateWithFlags(&ns, hipStreamNonBlocking));
    e->micro_streams.push_back(ns);
  }
  if (!e->hbm_stream) LRAM_HIP_CHECK(hipStreamCreateWithFlags(&e->hbm_stream, hipStreamNonBlocking));
  *hbm = e->hbm_stream;
  std::vector<Slice> out;
  const int base = e->n_live / n, rem = e->n_live % n;
  int b0 = 0;
  for (int i = 0; i < n; ++i) {
    const int nb = base + (i < rem ? 1 : 0);
    out.push_back(Slice{b0, nb, e->micro_streams[i]});
    b0 += nb;
  }
  return out;
}

void fork_slices(lram_engine* e, const std::vector<Slice>& sl, hipStream_t hbm, hipStream_t s) {
  for (const Slice& x : sl) stream_after(e, x.s, s, true);
  stream_after(e, hbm, s, true);
}
void join_slices(lram_engine* e, const std::vector<Slice>& sl, hipStream_t hbm, hipStream_t s) {
  for (const Slice& x : sl) stream_after(e, s, x.s, true);
  stream_after(e, s, hbm, true);
}

// Every public entry that launches the stack counts as one call of a sampled profile (lram_profile_begin_sampled): whether ITS
// launches are timed is decided here, not inherited from whatever call came before.
void prof_tick(lram_engine* e) { e->prof_live = !e->prof_on || (e->prof_calls++ % e->prof_every) == 0; }

}  // namespace lram::host

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int32_t lram_profile_begin(lram_engine* e) { return lram_profile_begin_sampled(e, 1); }

int32_t lram_profile_begin_sampled(lram_engine* e, int32_t every_n_steps) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr && every_n_steps >= 1, "lram_profile_begin_sampled: null engine / every_n_steps < 1");
    e->prof_on = true;
    e->prof_used = 0;
    e->prof_every = every_n_steps;
    e->prof_calls = 0;
    e->prof_live = true;
  });
}

int32_t lram_profile_end(lram_engine* e, double* total_ms, int64_t* n_launches) {
  return guarded([&] {
    LRAM_REQUIRE(e && total_ms && n_launches, "lram_profile_end: bad argument");
    double tot = 0.0;
    size_t n_aux = 0;
    for (size_t i = 0; i < e->prof_used; ++i) {
      LRAM_HIP_CHECK(hipEventSynchronize(e->prof_events[i].second));
      float ms = 0.f;
      LRAM_HIP_CHECK(hipEventElapsedTime(&ms, e->prof_events[i].first, e->prof_events[i].second));
      tot += ms;
      if (e->prof_aux[i]) ++n_aux;
    }
    *total_ms = tot;
    *n_launches = (int64_t)(e->prof_used - n_aux);
    e->prof_on = false;
    e->prof_live = true;
    e->prof_used = 0;
  });
}

int32_t lram_profile_end_split(lram_engine* e, double* main_ms, int64_t* n_main, double* aux_ms, int64_t* n_aux) {
  return guarded([&] {
    LRAM_REQUIRE(e && main_ms && n_main && aux_ms && n_aux, "lram_profile_end_split: bad argument");
    double tm = 0.0, ta = 0.0;
    int64_t nm = 0, na = 0;
    for (size_t i = 0; i < e->prof_used; ++i) {
      LRAM_HIP_CHECK(hipEventSynchronize(e->prof_events[i].second));
      float ms = 0.f;
      LRAM_HIP_CHECK(hipEventElapsedTime(&ms, e->prof_events[i].first, e->prof_events[i].second));
      if (e->prof_aux[i]) {
        ta += ms;
        ++na;
      } else {
        tm += ms;
        ++nm;
      }
    }
    *main_ms = tm, *n_main = nm, *aux_ms = ta, *n_aux = na;
    e->prof_on = false;
    e->prof_live = true;
    e->prof_used = 0;
  });
}

}  // extern "C"
