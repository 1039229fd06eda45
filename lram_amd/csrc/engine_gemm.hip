// The engine's GEMM dispatcher -- which projection takes which kernel family -- and the standalone lram_gemm_* entries that run
// one kernel family on caller-supplied operands (tests, micro-benchmarks).  Calls the kernel launchers of common.h only.
#include "engine.h"

namespace lram::host {

// The few-row kernel's share of the dispatch (see gemm()).
bool takes_skinny(const lram_engine* e, const GemmArgs& g) {
  const bool shape = g.k <= e->gemm_skinny_k && (g.m <= e->gemm_skinny_rows / 2 || (int64_t)g.n * g.k <= 600000);
  return g.m >= e->gemm_skinny_min && g.m <= e->gemm_skinny_rows && shape && gemm_skinny_supported(g);
}
// ... and may the norm ahead of this projection move into its prologue?  (Then the caller skips the norm launch and hands
// the un-normalised rows over with norm_g / norm_b / norm_eps / norm_rms set.)
bool takes_skinny_with_norm(const lram_engine* e, const GemmArgs& g) {
  return takes_skinny(e, g) && gemm_skinny_norm_supported(g);
}

}  // namespace lram::host

namespace {

// The narrow-output kernel's share: a whole packed weight (x_proj), enough rows to fill the chip with 16-row workgroups.
bool narrow_takes(const lram_engine* e, const GemmArgs& g) {
  if (!e->gemm_narrow_on || g.m < e->gemm_narrow_min_rows || g.a2 != nullptr || (int)g.ldw != g.k) return false;
  return e->narrow.count(g.w) != 0 && gemm_narrow_supported(g);
}

}  // namespace

namespace lram::host {

// ---- which projections take the f16x2 kernels: ONE predicate for the dispatcher and for the producers of the operands ------
// Row threshold: from 256 rows, wider weights earlier (below).  (Rounds 3-5: 1024 / 512, from
// the time the f16x2 kernels needed a row-maximum launch per projection; the producers hand the maxima over since round 5.)
// Round 6, one box, one env slice, env-steps/s with the old / new thresholds: 206M at 64 / 128 / 256 envs 12.4k / 17.9k / 24.8k ->
// 15.0k / 21.1k / 25.1k; Mamba-48M at 128 / 256 envs 84.2k / 149.6k -> 99.2k / 178.7k; 16M at 64 / 128 / 256 envs 95.8k / 150.6k /
// 207.4k -> 95.8k / 151.7k / 219.5k (16M at 64 envs = 192 rows on f16x2: 94.0k, hence 256 for the narrow weights).
// Below 256 rows by weight size: >= 2.5 M elements (206M stack) from 48 rows (206M at 16 envs 6.13k -> 6.65k), >= 1.1 M (Mamba-48M's
// in_proj / out_proj; not the 16M stack's 2048 x 512) from 96 (Mamba-48M at 32 / 64 envs 37.4k / 50.7k -> 40.1k / 52.7k).
bool f16x2_rows(const lram_engine* e, int rows, int n, int k) {
  const int64_t nk = (int64_t)n * k;
  return e->use_f16x2 && (rows >= e->f16x2_min_rows || (rows >= 96 && nk >= 1100000) || (rows >= 48 && nk >= 2500000));
}
// The f16 planes of the weight tensor that contains w (a GEMM may address a row range of a weight: proj_up's halves): fills the
// operand fields of g and returns true when w starts on a whole row of a split weight whose K equals ldw.
bool f16x2_weight(const lram_engine* e, const float* w, int ldw, GemmArgs* g) {
  auto it = e->split16.upper_bound(w);
  if (it == e->split16.begin()) return false;
  --it;
  if (!(w < it->first + it->second.rows * it->second.k) || (int)it->second.k != ldw) return false;
  const size_t row0 = (size_t)(w - it->first) / it->second.k;
  if (row0 * it->second.k != (size_t)(w - it->first)) return false;   // planes are addressed by whole rows
  if (g != nullptr) {
    g->w2 = it->second.planes + row0 * 32;  // K-tile-major planes
    g->w2_plane = (int64_t)split_f16x2_plane_elems(it->second.rows, it->second.k), g->w2_kt = (int64_t)it->second.rows * 32;
    g->w_inv = it->second.inv + row0;
  }
  return true;
}

// Does the projection `rows x k` against weight w take the f16x2 kernel with BOTH operands pre-split (gemm_f16x2p.hip)?  The
// producer of A (a row norm) asks before it chooses its output format, gemm() asks the same question through the a2 operand:
// the two cannot drift apart.  K a multiple of the kernel's 32-deep tile (d_model <= 2048: the norm kernels' limit, checked by
// validate_config).
bool presplit_for(const lram_engine* e, const float* w, int rows, int n, int k) {
  if (!e->gemm_presplit || (k & 31) != 0 || e->XN2.p == nullptr || !f16x2_rows(e, rows, n, k)) return false;
  // (the kernel's LDS-DMA addresses an operand's two planes with 32-bit byte offsets: gemm_f16x2p_supported)
  GemmArgs probe;
  if ((int64_t)e->XN2.n * 4 >= (1ll << 31) || !f16x2_weight(e, w, k, &probe)) return false;
  return 4 * probe.w2_plane < (1ll << 31);
}

// Does gemm() send the projection `rows x k` against weight w to the exact-fp32 narrow kernel (which reads no row maxima)?  The
// producer of A (Mamba's conv kernel) asks before it skips writing them; gemm() decides with the same narrow_takes().  A as the
// engine's producers write it: rows of pitch k on a 16-byte boundary (the packed weight's own address stands in for it).
bool narrow32_for(const lram_engine* e, const float* w, int rows, int n, int k) {
  GemmArgs probe;
  probe.a = w, probe.lda = k, probe.w = w, probe.ldw = k, probe.m = rows, probe.n = n, probe.k = k;
  return narrow_takes(e, probe) && !(e->use_f16x2 && e->gemm_narrow_f16);
}

int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return v ? std::atoi(v) : dflt;
}

GemmKnobs gemm_knobs_from_env() {
  GemmKnobs k;
  k.tile = env_int("LRAM_GEMM_TILE", k.tile);
  k.stages = env_int("LRAM_F16P_STAGES", k.stages);
  k.panel = env_int("LRAM_GEMM_PANEL", k.panel);
  k.splitk_tiles = env_int("LRAM_SPLITK_TILES", k.splitk_tiles);
  return k;
}

// GEMM dispatch: f16x2 (both operands pre-split, or A split while it is staged) for the big un-batched projections, the
// few-row kernel for tens of rows, bf16x3 for the batched per-head GEMMs and whatever is left, exact fp32 MFMA as the fallback.
void gemm(lram_engine* e, GemmArgs& g, hipStream_t s) {
  g.knobs = e->gemm_knobs;
  if (e->SK.p != nullptr) {
    g.splitk_ws = e->SK.p + (size_t)stream_slot(e, s) * lram_engine::kSplitKSlotElems;
    g.splitk_ws_elems = (int64_t)lram_engine::kSplitKSlotElems;
  }
  if (g.a2 != nullptr) {  // A handed over as f16x2 operand planes by its producer (presplit_for() said this GEMM takes them)
    LRAM_REQUIRE(f16x2_weight(e, g.w, (int)g.ldw, &g) && gemm_f16x2p_supported(g),
                 "gemm: pre-split A operand for a projection the pre-split kernel does not serve");
    launch_gemm_f16x2p(g, s);
    count_gemm(e, 0, g);
    return;
  }
  if (narrow_takes(e, g)) {  // narrow outputs (Mamba x_proj): one launch, no split-K slabs / reduce launch
    if (e->use_f16x2 && e->gemm_narrow_f16 && g.a_amax != nullptr && f16x2_weight(e, g.w, (int)g.ldw, &g) && gemm_narrow16_supported(g)) {
      launch_gemm_narrow16(g, s);   // f16x2 split products (the operand's row maxima come from its producer)
      count_gemm(e, 0, g);
      return;
    }
    g.w2 = nullptr, g.w_inv = nullptr, g.w2_kt = 0;
    launch_gemm_narrow(g, e->narrow.find(g.w)->second.p, s);   // exact fp32
    count_gemm(e, 2, g);
    return;
  }
  if (f16x2_rows(e, g.m, g.n, g.k) && g.nb1 * g.nb2 == 1 && e->ASCALE.p != nullptr && (size_t)g.m <= e->ascale_rows) {
    if (f16x2_weight(e, g.w, (int)g.ldw, &g) && gemm_f16x2_supported(g)) {
      if (g.a_amax == nullptr) {  // no producer handed the row maxima over: one small launch ahead of the GEMM
        float* sc = e->ASCALE.p + (size_t)stream_slot(e, s) * e->ascale_rows;
        launch_row_amax(g.a, g.lda, g.gate, g.ldg, g.m, g.k, sc, s);
        g.a_amax = sc, g.amax_parts = 1;
      }
      launch_gemm_f16x2(g, s);
      count_gemm(e, 0, g);
      return;
    }
    g.w2 = nullptr, g.w_inv = nullptr, g.w2_kt = 0;
  }
  // few operand rows (more than the GEMV's 8, at most gemm_skinny_rows): one 32 x 32 fp32 matrix-core tile per workgroup, operands
  // straight into registers, no split-K slab / reduce launch
  // Where it wins (same box each, `profiles/r03_ab_gemm_few_rows.txt`): K <= 1024 -- a lane group walks its K range in rounds
  // of 8 float4, one memory round trip each, so a long K is a long serial chain where the tile kernels' split-K spreads it
  // over workgroups (Mamba x_proj / out_proj, K = 1536: -3 % each at 32 envs; the 206M stack's K = 1280 / 2560: -7 % at 64
  // envs) -- and up to 192 operand rows, 384 for weights of at most 600k elements (every 32-row tile re-reads the weight).
  // 16M at 4 / 12 / 32 / 64 / 128 envs: +17 / +17 / +16 / +12 / +10 %; C1 (2 blocks, D = 128) at 32 envs: 0.130 -> 0.093 ms.
  if (takes_skinny(e, g)) {
    launch_gemm_skinny(g, s);
    count_gemm(e, 3, g);
    return;
  }
  if (e->use_bf16x3 && !gemm_small_m(g)) {
    // planes of the weight tensor that contains g.w (a GEMM may address a row range of a weight: proj_up's halves)
    auto it = e->split.upper_bound(g.w);
    if (it != e->split.begin() && (--it, g.w < it->first + it->second.n)) {
      g.w3 = it->second.p + (g.w - it->first);
      g.w3_plane = (int64_t)it->second.n;
      if (gemm_bf16x3_supported(g)) {
        launch_gemm_bf16x3(g, s);
        count_gemm(e, 1, g);
        return;
      }
    }
  }
  LRAM_REQUIRE(g.gate == nullptr && g.act_silu_from < 0, "gemm: gated operand / output activation need the bf16x3 kernel");
  launch_gemm_f32(g, s);
  count_gemm(e, 2, g);
}

void make_split(lram_engine* e, const float* w, size_t n) {
  if (w == nullptr || e->split.count(w)) return;
  uint16_t* p = nullptr;
  LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), 3 * n * sizeof(uint16_t)));
  launch_split_bf16x3(w, p, n, nullptr);
  e->split[w] = lram_engine::Split{p, n};
}

}  // namespace lram::host

// ---- standalone entries: one kernel family on caller-supplied operands ------------------------------------------------
namespace {

// The operands every entry shares (the split planes / packed weights of a family are added by its entry), and the launch knobs
// as the environment has them NOW: these are standalone test / micro-benchmark entries.
GemmArgs entry_args(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc,
                    const float* dev_bias, int32_t accumulate, int32_t m, int32_t n, int32_t k) {
  GemmArgs g;
  g.a = dev_a, g.lda = lda, g.w = dev_w, g.ldw = ldw, g.c = dev_c, g.ldc = ldc, g.bias = dev_bias;
  g.residual = accumulate ? dev_c : nullptr;
  g.m = m, g.n = n, g.k = k;
  g.knobs = lram::host::gemm_knobs_from_env();
  return g;
}

// Device memory of one entry: freed when the entry returns or throws (the entry synchronises the stream before it returns).
template <typename T>
struct Scratch {
  T* p = nullptr;
  explicit Scratch(size_t numel) { LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), numel * sizeof(T))); }
  ~Scratch() { (void)hipFree(p); }
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
};

// The f16x2 entries' weight operand: splits g's contiguous [n, k] weight into `planes` (2 x split_f16x2_plane_elems(n, k), K-tile-
// major) and inv[n], and points g at them.
void entry_split_weight(GemmArgs& g, uint16_t* planes, float* inv, hipStream_t s) {
  launch_split_f16x2(g.w, g.n, g.k, planes, inv, s);
  g.w2 = planes, g.w2_plane = (int64_t)split_f16x2_plane_elems((size_t)g.n, (size_t)g.k), g.w2_kt = 32 * (int64_t)g.n, g.w_inv = inv;
}

// The pre-split entries: both operands split into K-tile-major f16 planes, then `launch` (the pre-split launcher, or the 8-phase
// kernel it dispatches to for large launches) on them.
void entry_presplit(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc, const float* dev_bias,
                    int32_t accumulate, int32_t m, int32_t n, int32_t k, void* stream, void (*launch)(const GemmArgs&, hipStream_t)) {
  LRAM_REQUIRE(ldw == k, "lram_gemm_f16x2_presplit: W must be contiguous [n, k]");
  LRAM_REQUIRE(k % 32 == 0 && k <= 3072, "lram_gemm_f16x2_presplit: k must be a multiple of 32, <= 3072");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t wn = (size_t)n * k, an = (size_t)m * k;   // (k a multiple of 32: the planes have no padding)
  Scratch<uint16_t> wp(2 * wn), ap(2 * an);
  Scratch<float> scales((size_t)n + m);  // [n] inverse weight scales, then [m] inverse activation scales
  GemmArgs g = entry_args(dev_a, lda, dev_w, ldw, dev_c, ldc, dev_bias, accumulate, m, n, k);
  entry_split_weight(g, wp.p, scales.p, s);
  launch_row_split_f16x2(dev_a, lda, nullptr, 0, m, k, ap.p, 32 * (int64_t)m, (int64_t)an, scales.p + n, s);
  g.a = nullptr, g.lda = k;   // A goes in as its two planes
  g.a2 = ap.p, g.a2_plane = (int64_t)an, g.a2_kt = 32 * (int64_t)m, g.a2_inv = scales.p + n;
  launch(g, s);
  LRAM_HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int32_t lram_gemm_counts(lram_engine* e, double* out8, int32_t reset) {
  if (e == nullptr || out8 == nullptr) return 1;
  for (int i = 0; i < 8; ++i) out8[i] = e->gemm_counts[i];
  if (reset)
    for (int i = 0; i < 8; ++i) e->gemm_counts[i] = 0.0;
  return 0;
}

int32_t lram_slstm_counts(lram_engine* e, int64_t* out3, int32_t reset) {
  if (e == nullptr || out3 == nullptr) return 1;
  for (int i = 0; i < 3; ++i) out3[i] = e->slstm_counts[i];
  if (reset)
    for (int i = 0; i < 3; ++i) e->slstm_counts[i] = 0;
  return 0;
}

int32_t lram_gemm_f32(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc,
                      const float* dev_bias, int32_t accumulate, int32_t m, int32_t n, int32_t k, void* stream) {
  return guarded([&] {
    GemmArgs g = entry_args(dev_a, lda, dev_w, ldw, dev_c, ldc, dev_bias, accumulate, m, n, k);
    launch_gemm_f32(g, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_gemm_skinny(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc,
                         const float* dev_bias, int32_t accumulate, int32_t m, int32_t n, int32_t k, void* stream) {
  return guarded([&] {
    GemmArgs g = entry_args(dev_a, lda, dev_w, ldw, dev_c, ldc, dev_bias, accumulate, m, n, k);
    launch_gemm_skinny(g, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_gemm_narrow(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc,
                         const float* dev_bias, int32_t accumulate, int32_t m, int32_t n, int32_t k, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(ldw == k && accumulate == 0, "lram_gemm_narrow: W must be contiguous [n, k]; no accumulation");
    LRAM_REQUIRE(gemm_narrow_shape(n, k), "lram_gemm_narrow: n <= 96, k a multiple of 64, >= 256");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch<float> packed(gemm_narrow_pack_elems(n, k));
    launch_gemm_narrow_pack(dev_w, n, k, packed.p, s);
    GemmArgs g = entry_args(dev_a, lda, dev_w, ldw, dev_c, ldc, dev_bias, accumulate, m, n, k);
    launch_gemm_narrow(g, packed.p, s);
    LRAM_HIP_CHECK(hipStreamSynchronize(s));
  });
}

int32_t lram_gemm_narrow_f16x2(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc,
                               const float* dev_bias, int32_t accumulate, int32_t m, int32_t n, int32_t k, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(ldw == k && accumulate == 0, "lram_gemm_narrow_f16x2: W must be contiguous [n, k]; no accumulation");
    LRAM_REQUIRE(gemm_narrow_shape(n, k), "lram_gemm_narrow_f16x2: n <= 96, k a multiple of 64, >= 256");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t numel = split_f16x2_plane_elems((size_t)n, (size_t)k);
    Scratch<uint16_t> planes(2 * numel);
    Scratch<float> scales((size_t)n + m);  // [n] inverse weight scales, then [m] row maxima of A
    GemmArgs g = entry_args(dev_a, lda, dev_w, ldw, dev_c, ldc, dev_bias, accumulate, m, n, k);
    entry_split_weight(g, planes.p, scales.p, s);
    launch_row_amax(dev_a, lda, nullptr, 0, m, k, scales.p + n, s);
    g.a_amax = scales.p + n, g.amax_parts = 1;
    launch_gemm_narrow16(g, s);
    LRAM_HIP_CHECK(hipStreamSynchronize(s));
  });
}

int32_t lram_gemm_bf16x3(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc,
                         const float* dev_bias, int32_t accumulate, int32_t m, int32_t n, int32_t k, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(ldw == k, "lram_gemm_bf16x3: W must be contiguous [n, k]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t numel = (size_t)n * k;
    Scratch<uint16_t> planes(3 * numel);
    launch_split_bf16x3(dev_w, planes.p, numel, s);
    GemmArgs g = entry_args(dev_a, lda, dev_w, ldw, dev_c, ldc, dev_bias, accumulate, m, n, k);
    g.w3 = planes.p, g.w3_plane = (int64_t)numel;
    launch_gemm_bf16x3(g, s);
    LRAM_HIP_CHECK(hipStreamSynchronize(s));
  });
}

int32_t lram_gemm_f16x2(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc,
                        const float* dev_bias, int32_t accumulate, int32_t m, int32_t n, int32_t k, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(ldw == k, "lram_gemm_f16x2: W must be contiguous [n, k]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t numel = split_f16x2_plane_elems((size_t)n, (size_t)k);  // (K-tile-major planes)
    Scratch<uint16_t> planes(2 * numel);
    Scratch<float> scales((size_t)n + m);  // [n] inverse weight scales, then [m] activation scales
    GemmArgs g = entry_args(dev_a, lda, dev_w, ldw, dev_c, ldc, dev_bias, accumulate, m, n, k);
    entry_split_weight(g, planes.p, scales.p, s);
    launch_row_amax(dev_a, lda, nullptr, 0, m, k, scales.p + n, s);
    g.a_amax = scales.p + n;
    launch_gemm_f16x2(g, s);
    LRAM_HIP_CHECK(hipStreamSynchronize(s));
  });
}

int32_t lram_gemm_f16x2_presplit(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc,
                                 const float* dev_bias, int32_t accumulate, int32_t m, int32_t n, int32_t k, void* stream) {
  return guarded([&] {
    entry_presplit(dev_a, lda, dev_w, ldw, dev_c, ldc, dev_bias, accumulate, m, n, k, stream, launch_gemm_f16x2p);
  });
}

int32_t lram_gemm_f16x2_presplit_8p(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c, int64_t ldc,
                                    const float* dev_bias, int32_t accumulate, int32_t m, int32_t n, int32_t k, void* stream) {
  return guarded([&] {
    entry_presplit(dev_a, lda, dev_w, ldw, dev_c, ldc, dev_bias, accumulate, m, n, k, stream, [](const GemmArgs& g, hipStream_t s) {
      LRAM_REQUIRE(gemm_f16x2p_supported(g) && gemm_f16x2_8p_supported(g), "lram_gemm_f16x2_presplit_8p: unsupported operand layout");
      launch_gemm_f16x2_8p(g, s);
    });
  });
}

}  // extern "C"
