// Engine: owns weights, per-env recurrent state and activation workspace on one MI355X, and issues the
// kernel sequence of one env-step (layer-major: every block consumes all T tokens of the timestep before
// the next block runs, so each block's recurrent state is read and written once per env-step).
// C ABI in include/lram_hip.h.
// This file: the engine's lifecycle -- create / destroy, weights and finalize, workspace and state allocation, the mode setters.
// The launch sequence of a step lives in engine_step.hip (front end, head, entries), engine_xlstm.hip / engine_mamba.hip (the
// stacks), engine_gemm.hip (the GEMM dispatcher) and engine_streams.hip (events, env slices, profiler); per-slot and whole-batch
// state access in engine_state.hip.  engine.h holds the engine object and what crosses these files.
#include "engine.h"

namespace {

const float* need(lram_engine* e, const std::string& name, size_t numel) {
  auto it = e->weights.find(name);
  if (it == e->weights.end()) throw Error("lram: missing weight '" + name + "'");
  if (it->second.n != numel)
    throw Error("lram: weight '" + name + "' has " + std::to_string(it->second.n) + " elements, expected " +
                std::to_string(numel));
  return it->second.p;
}
const float* optional(lram_engine* e, const std::string& name, size_t numel) {
  auto it = e->weights.find(name);
  if (it == e->weights.end()) return nullptr;
  if (it->second.n != numel)
    throw Error("lram: weight '" + name + "' has " + std::to_string(it->second.n) + " elements, expected " +
                std::to_string(numel));
  return it->second.p;
}

void validate_config(const lram_config& c) {
  LRAM_REQUIRE(c.abi_version == LRAM_ABI_VERSION, "config.abi_version does not match the library");
  LRAM_REQUIRE(c.backbone == LRAM_BACKBONE_XLSTM || c.backbone == LRAM_BACKBONE_MAMBA, "unknown backbone");
  LRAM_REQUIRE(c.d_model > 0 && c.d_model % 4 == 0 && c.d_model <= 2048, "d_model must be a multiple of 4, <= 2048");
  LRAM_REQUIRE(c.n_blocks > 0 && c.n_blocks <= LRAM_MAX_BLOCKS, "n_blocks out of range");
  LRAM_REQUIRE(c.tokens_per_step >= 1 && c.tokens_per_step <= 4, "tokens_per_step must be in 1..4");
  LRAM_REQUIRE(c.pred_token >= 0 && c.pred_token < c.tokens_per_step, "pred_token out of range");
  LRAM_REQUIRE(c.state_dim > 0 && c.state_dim % 4 == 0, "state_dim must be a positive multiple of 4");
  LRAM_REQUIRE(c.act_dim > 0 && c.n_vocab > 0 && c.n_discrete >= 0 && c.n_discrete <= c.n_vocab &&
                   c.action_channels > 0,
               "bad action head dimensions");
  if (c.backbone == LRAM_BACKBONE_XLSTM) {
    LRAM_REQUIRE(c.n_heads > 0 && c.inner > 0 && c.inner % (c.n_heads * 16) == 0,
                 "xLSTM inner dim must be a multiple of 16 * n_heads");
    LRAM_REQUIRE(c.d_model % c.n_heads == 0, "d_model must be a multiple of n_heads");
    // limits of the step kernels (xlstm_kernels.hip: kMaxGroups, kGnMaxV, the NH template instances), checked here so
    // that lram_create fails up front instead of a launch throwing in the middle of a step.  Every preset of the
    // reference's configs/agent_params/huggingface/xlstm_*.yaml passes (head dims 256 .. 896, inner <= 3584); head dims
    // that are not multiples of 64 (the *_half presets: 352, 544, 720) take 16-column cell slices and no lazy / chunkwise
    // path.  sLSTM blocks additionally need d_model / num_heads to be a multiple of 4 (checked below where they occur).
    LRAM_REQUIRE(c.n_heads == 1 || c.n_heads == 2 || c.n_heads == 4 || c.n_heads == 8, "xLSTM num_heads must be 1, 2, 4 or 8");
    LRAM_REQUIRE(c.inner <= 4096, "xLSTM inner dim (proj_factor * embedding_dim, rounded up to 64) must be <= 4096");
    LRAM_REQUIRE(c.inner / c.n_heads <= 1024, "mLSTM head dim must be <= 1024");
    LRAM_REQUIRE(c.d_model / c.n_heads <= 1024, "sLSTM head dim must be <= 1024");
    LRAM_REQUIRE(c.conv_k == 4, "conv1d_kernel_size must be 4");
    LRAM_REQUIRE(c.qkv_blocksize == 4, "qkv_proj_blocksize must be 4");
    bool any_s = false;
    for (int i = 0; i < c.n_blocks; ++i) any_s |= c.block_is_slstm[i] != 0;
    if (any_s) {
      LRAM_REQUIRE(c.ffn_dim > 0 && c.ffn_dim % 4 == 0, "ffn_dim must be a positive multiple of 4");
      LRAM_REQUIRE(c.d_model % (4 * c.n_heads) == 0, "sLSTM blocks need d_model to be a multiple of 4 * n_heads");
    }
  } else {
    LRAM_REQUIRE(c.d_inner > 0 && c.d_inner % 4 == 0 && c.d_conv == 4 && c.d_state > 0 && c.dt_rank > 0,
                 "bad Mamba dimensions");
    // limit of the selective-state-update kernels (mamba_kernels.hip: d_state / 4 lanes per channel, a power of two, reduced by
    // shuffles inside a wave quarter), checked here for the same reason as the xLSTM limits above
    LRAM_REQUIRE(c.d_state == 4 || c.d_state == 8 || c.d_state == 16 || c.d_state == 32 || c.d_state == 64,
                 "Mamba d_state must be 4, 8, 16, 32 or 64");
  }
}

void finalize(lram_engine* e) {
  const lram_config& c = e->cfg;
  const size_t D = c.d_model;
  e->w_state = need(e, "embed_state.weight", D * c.state_dim);
  e->b_state = need(e, "embed_state.bias", D);
  e->w_rtg = need(e, "embed_return.weight", D);
  e->b_rtg = need(e, "embed_return.bias", D);
  e->w_rew = need(e, "embed_rewards.weight", D);
  e->b_rew = need(e, "embed_rewards.bias", D);
  e->eln_g = need(e, "embed_ln.weight", D);
  e->eln_b = optional(e, "embed_ln.bias", D);
  e->w_head = need(e, "action_net.weight", (size_t)c.act_dim * c.n_vocab * D);
  e->b_head = need(e, "action_net.bias", (size_t)c.act_dim * c.n_vocab);
  e->post_g = need(e, "post_norm.gamma", D);
  e->post_b = optional(e, "post_norm.beta", D);
  e->bw.assign(c.n_blocks, BlockWeights());
  for (int i = 0; i < c.n_blocks; ++i) {
    BlockWeights& w = e->bw[i];
    const std::string p = "b" + std::to_string(i) + ".";
    w.norm_g = need(e, p + "norm.gamma", D);
    w.norm_b = optional(e, p + "norm.beta", D);
    if (c.backbone == LRAM_BACKBONE_MAMBA) {
      const size_t di = c.d_inner, N = c.d_state, R = c.dt_rank;
      w.in_proj = need(e, p + "in_proj", 2 * di * D);
      w.in_proj_b = optional(e, p + "in_proj_b", 2 * di);
      w.conv_w = need(e, p + "conv_w", di * 4);
      w.conv_b = optional(e, p + "conv_b", di);
      w.x_proj = need(e, p + "x_proj", (R + 2 * N) * di);
      w.dt_proj = need(e, p + "dt_proj", di * R);
      w.dt_bias = need(e, p + "dt_bias", di);
      w.A_log = need(e, p + "A_log", di * N);
      w.Dp = need(e, p + "D", di);
      w.out_proj = need(e, p + "out_proj", D * di);
      w.out_proj_b = optional(e, p + "out_proj_b", D);
    } else if (c.block_is_slstm[i]) {
      const size_t NH = c.n_heads, DH = D / NH, F = c.ffn_dim;
      w.conv_w = need(e, p + "conv_w", D * 4);
      w.conv_b = need(e, p + "conv_b", D);
      w.gate_w[0] = need(e, p + "gate_i", NH * DH * DH);
      w.gate_w[1] = need(e, p + "gate_f", NH * DH * DH);
      w.gate_w[2] = need(e, p + "gate_z", NH * DH * DH);
      w.gate_w[3] = need(e, p + "gate_o", NH * DH * DH);
      w.rt = need(e, p + "rt", NH * 4 * DH * DH);
      w.rbias = need(e, p + "rbias", 4 * D);
      w.gn_g = need(e, p + "gn.gamma", D);
      w.gn_b = optional(e, p + "gn.beta", D);
      w.ffn_norm_g = need(e, p + "ffn_norm.gamma", D);
      w.ffn_norm_b = optional(e, p + "ffn_norm.beta", D);
      w.ffn_up = need(e, p + "ffn_up", 2 * F * D);
      w.ffn_down = need(e, p + "ffn_down", D * F);
    } else {
      const size_t inner = c.inner, NH = c.n_heads;
      w.proj_up = need(e, p + "proj_up", 2 * inner * D);
      w.conv_w = need(e, p + "conv_w", inner * 4);
      w.conv_b = need(e, p + "conv_b", inner);
      w.wq = need(e, p + "wq", inner * 4);
      w.wk = need(e, p + "wk", inner * 4);
      w.wv = need(e, p + "wv", inner * 4);
      w.wi = need(e, p + "wi", NH * 3 * inner);
      w.bi = need(e, p + "bi", NH);
      w.wf = need(e, p + "wf", NH * 3 * inner);
      w.bf = need(e, p + "bf", NH);
      w.on_g = need(e, p + "outnorm.gamma", inner);
      w.on_b = optional(e, p + "outnorm.beta", inner);
      w.skip = need(e, p + "skip", inner);
      w.proj_down = need(e, p + "proj_down", D * inner);
    }
  }
  // optional image front end: embed_image.* with the reference's module names (image_encoders.py:39-56)
  e->img_lin_w = nullptr;
  e->img_channels = 0;
  {
    auto it = e->weights.find("embed_image.cnn.0.conv.weight");
    if (it != e->weights.end()) {
      const int chans[3] = {16, 32, 32};
      LRAM_REQUIRE(it->second.n % (16 * 9) == 0, "embed_image.cnn.0.conv.weight has an unexpected size");
      int cin = (int)(it->second.n / (16 * 9));
      e->img_channels = cin;
      for (int sidx = 0; sidx < 3; ++sidx) {
        const int cout = chans[sidx];
        const std::string p = "embed_image.cnn." + std::to_string(sidx) + ".";
        const char* names[5] = {"conv", "residual_0.conv_0", "residual_0.conv_1", "residual_1.conv_0", "residual_1.conv_1"};
        for (int k = 0; k < 5; ++k) {
          lram_engine::ImgConv& cv = e->img_conv[sidx][k];
          cv.cin = k == 0 ? cin : cout;
          cv.cout = cout;
          cv.w = need(e, p + names[k] + ".weight", (size_t)cout * cv.cin * 9);
          cv.b = need(e, p + names[k] + ".bias", (size_t)cout);
        }
        cin = cout;
      }
      auto lw = e->weights.find("embed_image.linear.0.weight");
      LRAM_REQUIRE(lw != e->weights.end() && lw->second.n % D == 0, "embed_image.linear.0.weight missing or mis-sized");
      e->img_flat = (int)(lw->second.n / D);
      e->img_lin_w = lw->second.p;
      e->img_lin_b = need(e, "embed_image.linear.0.bias", D);
    }
  }
  // bf16 split planes of every GEMM weight (LRAM_GEMM=f32 keeps the exact fp32-MFMA kernels instead)
  e->drop_splits();
  if (e->use_bf16x3 && e->use_f16x2) {
    // the big un-batched projections: (weight, rows, K); the per-head / per-gate batched GEMMs of the sLSTM block keep
    // bf16x3 (their operand rows would need one scale per head)
    const int D = c.d_model;
    auto rows_of = [&](const float* p, size_t k) -> size_t {
      for (auto& kv : e->weights)
        if (kv.second.p == p) return kv.second.n / k;
      return 0;
    };
    auto add16 = [&](const float* p, size_t k) {
      if (p == nullptr || k == 0 || (k & 7) != 0 || e->split16.count(p)) return;
      const size_t rows = rows_of(p, k);
      if (rows == 0) return;
      lram_engine::Split16 sp{nullptr, nullptr, rows, k};
      LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&sp.planes), 2 * split_f16x2_plane_elems(rows, k) * sizeof(uint16_t)));
      LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&sp.inv), rows * sizeof(float)));
      launch_split_f16x2(p, (int)rows, (int)k, sp.planes, sp.inv, nullptr);
      e->split16[p] = sp;
    };
    add16(e->w_head, D);
    if (e->img_lin_w != nullptr) add16(e->img_lin_w, (size_t)e->img_flat);
    for (const BlockWeights& w : e->bw) {
      add16(w.proj_up, D), add16(w.proj_down, c.inner), add16(w.ffn_up, D), add16(w.ffn_down, c.ffn_dim);
      add16(w.in_proj, D), add16(w.x_proj, c.d_inner), add16(w.out_proj, c.d_inner);
      // (dt_proj, K = dt_rank = 48: two K tiles, nothing to gain -- 24.8 us vs 20.8 us for bf16x3 at 6144 rows)
    }
  }
  if (e->use_bf16x3) {
    auto numel = [&](const float* p) -> size_t {
      for (auto& kv : e->weights)
        if (kv.second.p == p) return kv.second.n;
      return 0;
    };
    std::vector<const float*> ws = {e->w_head, e->img_lin_w};  // embed_state has K = state_dim (204): rows not 16-byte aligned
    for (const BlockWeights& w : e->bw)
      for (const float* p : {w.proj_up, w.proj_down, w.gate_w[0], w.gate_w[1], w.gate_w[2], w.gate_w[3], w.rt, w.ffn_up,
                             w.ffn_down, w.in_proj, w.x_proj, w.dt_proj, w.out_proj})
        ws.push_back(p);
    for (const float* p : ws)
      if (p != nullptr) make_split(e, p, numel(p));
    LRAM_HIP_CHECK(hipDeviceSynchronize());
  }
  e->gate_coef.assign(e->bw.size(), DevBuf());
  if (c.backbone == LRAM_BACKBONE_XLSTM && mlstm_front_supported(c.inner, c.n_heads, c.conv_k, c.tokens_per_step)) {
    for (size_t i = 0; i < e->bw.size(); ++i) {
      if (c.block_is_slstm[i]) continue;
      const BlockWeights& w = e->bw[i];
      e->gate_coef[i].alloc((size_t)c.inner * 4 * c.n_heads);
      launch_gate_coef(w.wq, w.wk, w.wv, w.wi, w.wf, c.inner, c.n_heads, e->gate_coef[i].p, nullptr);
    }
    LRAM_HIP_CHECK(hipDeviceSynchronize());
  }
  e->slstm_rt2.assign(e->bw.size(), DevBuf());
  e->slstm_rinv.assign(e->bw.size(), DevBuf());
  if (c.backbone == LRAM_BACKBONE_XLSTM && slstm_seq_supported(c.d_model, c.n_heads, c.tokens_per_step)) {
    for (size_t i = 0; i < e->bw.size(); ++i) {
      if (!c.block_is_slstm[i]) continue;
      const size_t sdh = (size_t)c.d_model / c.n_heads;
      e->slstm_rt2[i].alloc((size_t)c.n_heads * 4 * sdh * sdh);
      if (e->use_f16x2 && !e->slstm_seq_f32) {  // (two f16 planes: the bytes of the fp32 copy)
        e->slstm_rinv[i].alloc((size_t)c.n_heads * 4 * sdh);
        launch_slstm_pack_rt16(e->bw[i].rt, reinterpret_cast<uint16_t*>(e->slstm_rt2[i].p), e->slstm_rinv[i].p, c.n_heads, (int)sdh, nullptr);
      } else {
        launch_slstm_pack_rt(e->bw[i].rt, e->slstm_rt2[i].p, c.n_heads, (int)sdh, nullptr);
      }
    }
    LRAM_HIP_CHECK(hipDeviceSynchronize());
  }
  if (c.backbone == LRAM_BACKBONE_MAMBA && e->gemm_narrow_on && gemm_narrow_shape(c.dt_rank + 2 * c.d_state, c.d_inner)) {
    const int nx = c.dt_rank + 2 * c.d_state;
    for (const BlockWeights& w : e->bw) {
      if (w.x_proj == nullptr || e->narrow.count(w.x_proj)) continue;
      DevBuf& pk = e->narrow[w.x_proj];
      pk.alloc(gemm_narrow_pack_elems(nx, c.d_inner));
      launch_gemm_narrow_pack(w.x_proj, nx, c.d_inner, pk.p, nullptr);
    }
    LRAM_HIP_CHECK(hipDeviceSynchronize());
  }
  e->dt_wt.assign(e->bw.size(), DevBuf());
  if (c.backbone == LRAM_BACKBONE_MAMBA && e->mamba_dt_fuse && mamba_ssm_dt_fusable(c.d_state, c.dt_rank)) {
    for (size_t i = 0; i < e->bw.size(); ++i) {
      e->dt_wt[i].alloc((size_t)c.d_inner * c.dt_rank);
      launch_transpose_f32(e->bw[i].dt_proj, c.d_inner, c.dt_rank, e->dt_wt[i].p, nullptr);
    }
    LRAM_HIP_CHECK(hipDeviceSynchronize());
  }
  e->finalized = true;
}

// Activation workspace for `tokens` tokens per env slot (rows b * T + t of every buffer).
size_t workspace_floats_per_token(const lram_config& c) {
  const size_t D = c.d_model;
  if (c.backbone == LRAM_BACKBONE_MAMBA) return 5 * D + 4 * (size_t)c.d_inner + c.dt_rank + 2 * c.d_state + (size_t)c.d_inner;
  const size_t inner = c.inner;
  const size_t ucols = std::max<size_t>(std::max<size_t>(2 * inner, 4 * D), 2 * (size_t)c.ffn_dim);
  const size_t icols = std::max<size_t>(std::max<size_t>(inner, D), (size_t)c.ffn_dim);
  return 4 * D + ucols + 6 * icols + 6 * (size_t)c.n_heads;
}

// The per-token activation buffers a chunk of a stored context goes through (xLSTM and Mamba): what a second chunk in flight needs its own copy of.
// (SK / ASCALE are per stream already; LOGITS / TOK belong to the last timestep, which always runs on the primary set.)
std::array<DevBuf*, 21> workspace_set(lram_engine* e) {
  return {&e->X, &e->XN, &e->XN2, &e->HID, &e->U, &e->Q, &e->K, &e->V, &e->XA, &e->H, &e->G, &e->SCAL, &e->RY, &e->GATES,
          &e->AMAT, &e->VEC, &e->AMX_XN, &e->AMX_H, &e->RES, &e->DTP, &e->AMX_XA};
}

}  // namespace

namespace lram::host {

thread_local std::string g_last_error;   // lram_last_error

void alloc_workspace(lram_engine* e, int tokens) {
  const lram_config& c = e->cfg;
  const size_t B = e->B, D = c.d_model, BT = B * (size_t)tokens;
  e->SK.alloc(lram_engine::kSplitKSlotElems * lram_engine::kSplitKSlots);
  e->ascale_rows = BT;
  e->ASCALE.alloc(BT * lram_engine::kSplitKSlots);
  const size_t parts = c.backbone == LRAM_BACKBONE_MAMBA ? std::max<size_t>(1, c.d_inner / 64) : 0;
  e->AMX_XN.alloc(BT);
  if (parts) e->AMX_XA.alloc(BT * parts), e->AMX_H.alloc(BT * parts);
  if (c.backbone == LRAM_BACKBONE_XLSTM && e->use_f16x2) e->AMX_H.alloc(BT * (size_t)c.n_heads);  // group norm -> proj_down: per-head maxima
  e->X.alloc(BT * D);
  e->XN.alloc(BT * D);
  if (e->gemm_presplit && e->use_f16x2) e->XN2.alloc(BT * D);
  e->TOK.alloc(BT * D);
  e->HID.alloc(BT * D);
  e->LOGITS.alloc(B * c.act_dim * c.n_vocab);
  if (c.backbone == LRAM_BACKBONE_MAMBA) {
    const size_t di = c.d_inner;
    e->RES.alloc(BT * D);
    e->U.alloc(BT * 2 * di);                        // xz
    e->XA.alloc(BT * di);                           // xc
    e->Q.alloc(BT * (c.dt_rank + 2 * c.d_state));   // x_proj output
    e->DTP.alloc(BT * di);
    e->H.alloc(BT * di);                            // y
  } else {
    const size_t inner = c.inner;
    const size_t ucols = std::max<size_t>(std::max<size_t>(2 * inner, 4 * D), 2 * (size_t)c.ffn_dim);
    const size_t icols = std::max<size_t>(std::max<size_t>(inner, D), (size_t)c.ffn_dim);
    e->ucols = ucols, e->icols = icols;
    e->U.alloc(BT * ucols);
    e->Q.alloc(BT * icols);
    e->K.alloc(BT * icols);
    e->V.alloc(BT * icols);
    e->XA.alloc(BT * icols);
    e->H.alloc(BT * icols);
    e->G.alloc(BT * icols);
    e->SCAL.alloc(BT * c.n_heads * 4);
    e->RY.alloc(B * 4 * D);
    if (tokens > kMaxTokens) {
      e->GATES.alloc(BT * c.n_heads * 2);
      e->AMAT.alloc(B * c.n_heads * kChunkMaxTokens * kChunkMaxTokens);
      e->VEC.alloc(B * c.n_heads * 3 * kChunkMaxTokens);
    }
  }
  e->tok_cap = tokens;
}

void swap_workspace(lram_engine* e, int lane) {   // lane >= 1: primary <-> that lane's copy
  const auto ws = workspace_set(e);
  for (size_t i = 0; i < ws.size(); ++i) std::swap(*ws[i], e->twin[lane - 1][i]);
}
// Second workspace for the chunk lanes, sized like the first; false (no lanes) if the device has no room for it.
bool twin_ready(lram_engine* e) {
  const auto ws = workspace_set(e);
  bool same = true;
  size_t want = 0;
  for (int l = 0; l + 1 < e->n_lanes; ++l)
    for (size_t i = 0; i < ws.size(); ++i) same = same && e->twin[l][i].n == ws[i]->n, want += ws[i]->n * sizeof(float);
  if (same) return true;
  LRAM_HIP_CHECK(hipDeviceSynchronize());
  for (auto& t : e->twin)
    for (DevBuf& b : t) b.release();
  size_t free_b = 0, total_b = 0;
  LRAM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if (want + ((size_t)2 << 30) > free_b) return false;  // keep 2 GiB of headroom
  for (int l = 0; l + 1 < e->n_lanes; ++l)
    for (size_t i = 0; i < ws.size(); ++i) e->twin[l][i].alloc(ws[i]->n);
  LRAM_HIP_CHECK(hipDeviceSynchronize());
  return true;
}

// Timesteps per state pass for a stored context of L timesteps.  xLSTM geometries the chunkwise kernels cover
// take up to 21 timesteps (63 tokens) per pass, in equal chunks; everything else 4 (the token-sequential kernels).
// Grows the activation workspace on first use when the device has room for it.
int prefill_chunk_steps(lram_engine* e, int L) {
  const lram_config& c = e->cfg;
  const int T = c.tokens_per_step;
  const int seq = kMaxTokens / T;
  if (!e->chunk_prefill || c.backbone != LRAM_BACKBONE_XLSTM || L <= seq || e->graph_mode ||
      !mlstm_chunk_supported(c.inner, c.n_heads, c.conv_k))
    return seq;
  const int max_steps = kChunkMaxTokens / T;
  const int n_chunks = (L + max_steps - 1) / max_steps;
  const int steps = (L + n_chunks - 1) / n_chunks;
  if (steps * T <= kMaxTokens) return seq;
  if (steps * T > e->tok_cap) {
    LRAM_HIP_CHECK(hipDeviceSynchronize());
    size_t free_b = 0, total_b = 0;
    LRAM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t have = workspace_floats_per_token(c) * 4 * (size_t)e->B * e->tok_cap;
    const size_t want = workspace_floats_per_token(c) * 4 * (size_t)e->B * kChunkMaxTokens +
                        (size_t)e->B * c.n_heads * (kChunkMaxTokens + 3) * kChunkMaxTokens * 4;
    if (want > have + free_b - std::min<size_t>(free_b, (size_t)2 << 30)) return seq;  // keep 2 GiB of headroom
    alloc_workspace(e, kChunkMaxTokens);
    LRAM_HIP_CHECK(hipDeviceSynchronize());
  }
  return steps;
}

}  // namespace lram::host

namespace {

// ---- lazy matrix memory plumbing ------------------------------------------------------------------------
bool lazy_geometry_ok(const lram_engine* e) {
  return has_mlstm_block(e) && mlstm_lazy_supported(e->cfg.inner / e->cfg.n_heads, e->cfg.tokens_per_step);
}

// Segment and chunk tables of the per-slot state calls (common.h: SlotSeg).  Record layout = blocks in order, within a block
// the tensors that exist in `which` order 0..3, each the env's slice in the reference layout (include/lram_hip.h).
void slot_segments_build(lram_engine* e) {
  e->drop_slot_segments();
  if (e->B <= 0) return;
  const lram_config& c = e->cfg;
  const int64_t B = e->B;
  std::vector<SlotSeg>& segs = e->slot_segs;
  int64_t rec = 0;
  const int64_t rec_numel = lram_state_bytes_per_env(e) / 4;
  auto add = [&](float* base, int64_t stride, int64_t numel, int kind, int parity, bool in_record) {
    if (base == nullptr || numel <= 0) return;
    SlotSeg sg{};
    sg.base = base, sg.stride = stride, sg.numel = (int32_t)numel, sg.kind = kind, sg.parity = parity;
    sg.rec_off = in_record ? rec : -1;
    const bool slot_ok = numel % 4 == 0 && stride % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
    const bool rec_ok = in_record && rec % 4 == 0 && rec_numel % 4 == 0;
    sg.vec = (slot_ok ? 1 : 0) | (slot_ok && rec_ok ? 2 : 0);
    if (in_record) rec += numel;
    segs.push_back(sg);
  };
  e->slot_c_off.assign(c.n_blocks, -1);
  e->slot_y_checked = false;
  for (int i = 0; i < c.n_blocks; ++i) {
    BlockState& s = e->st[i];
    if (c.backbone == LRAM_BACKBONE_MAMBA) {
      add(s.s0.p, (int64_t)c.d_inner * c.d_state, (int64_t)c.d_inner * c.d_state, kSlotSegState, -1, true);
      add(s.conv.p, (int64_t)c.d_inner * c.d_conv, (int64_t)c.d_inner * c.d_conv, kSlotSegState, -1, true);
    } else if (c.block_is_slstm[i]) {
      const int64_t D = c.d_model;
      const bool checked = e->slstm_rinv.size() > (size_t)i && e->slstm_rinv[i].p != nullptr;
      e->slot_y_checked = e->slot_y_checked || checked;
      for (int p = 0; p < 4; ++p)   // [4, B, D]: y, c, n, m planes
        add(s.s0.p + p * B * D, D, D, p == 0 && checked ? kSlotSegSlstmY : kSlotSegState, -1, true);
      add(s.conv.p, (int64_t)c.conv_k * D, (int64_t)c.conv_k * D, kSlotSegState, -1, true);
    } else {
      const int64_t NH = c.n_heads, DH = e->dh();
      e->slot_c_off[i] = rec;
      add(s.s0.p, NH * DH * DH, NH * DH * DH, kSlotSegC, -1, true);
      add(s.n.p, c.inner, c.inner, kSlotSegState, -1, true);
      add(s.m.p, NH, NH, kSlotSegState, -1, true);
      add(s.conv.p, (int64_t)c.conv_k * c.inner, (int64_t)c.conv_k * c.inner, kSlotSegState, -1, true);
    }
  }
  LRAM_REQUIRE(rec == rec_numel, "slot state: the segment table does not add up to the record size");
  const size_t n_rec_segs = segs.size();
  if (e->lazy_ready) {  // the lazy representation (copy only): window rows, and both ping-pong sides of the bookkeeping
    const int64_t NH = c.n_heads, DH = e->dh(), W = kLazyWindow;
    for (int i = 0; i < c.n_blocks; ++i) {
      if (c.block_is_slstm[i]) continue;
      BlockState& s = e->st[i];
      add(s.wk.p, NH * W * DH, NH * W * DH, kSlotSegWindow, -1, false);
      add(s.wv.p, NH * W * DH, NH * W * DH, kSlotSegWindow, -1, false);
      for (int p = 0; p < 2; ++p) {
        add(s.coef.p + p * B * NH * W, NH * W, NH * W, kSlotSegCoef, p, false);
        add(s.gsc.p + p * B * NH, NH, NH, kSlotSegG, p, false);
      }
      // (s.pw, the window scores, is scratch of one step -- written by the score kernel and read by the read pass of the SAME
      // step, first n + T entries of a row only -- and is not state: nothing to move)
    }
    for (int p = 0; p < 2; ++p) add(e->LZ_COUNT.p + p * B, 1, 1, kSlotSegCount, p, false);   // one count word per env, all blocks
  }
  std::vector<SlotChunk> chunks;
  for (size_t k = 0; k < segs.size(); ++k) {
    if (k == n_rec_segs) e->slot_n_rec_chunks = (int)chunks.size();
    for (int32_t off = 0; off < segs[k].numel; off += kSlotChunk) chunks.push_back(SlotChunk{(int32_t)k, off});
  }
  if (segs.size() == n_rec_segs) e->slot_n_rec_chunks = (int)chunks.size();
  e->slot_n_chunks = (int)chunks.size();
  LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->slot_segs_dev), segs.size() * sizeof(SlotSeg)));
  LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->slot_chunks_dev), chunks.size() * sizeof(SlotChunk)));
  LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->slot_idx_dev), 2 * (size_t)B * sizeof(int32_t)));
  LRAM_HIP_CHECK(hipMemcpy(e->slot_segs_dev, segs.data(), segs.size() * sizeof(SlotSeg), hipMemcpyHostToDevice));
  LRAM_HIP_CHECK(hipMemcpy(e->slot_chunks_dev, chunks.data(), chunks.size() * sizeof(SlotChunk), hipMemcpyHostToDevice));
}

void lazy_alloc(lram_engine* e) {
  if (e->lazy_ready || e->B <= 0 || !lazy_geometry_ok(e)) return;
  const lram_config& c = e->cfg;
  const size_t B = e->B, NH = c.n_heads, DH = e->dh();
  for (int i = 0; i < c.n_blocks; ++i) {
    if (c.block_is_slstm[i]) continue;
    BlockState& s = e->st[i];
    s.wk.alloc(B * NH * kLazyWindow * DH);
    s.wv.alloc(B * NH * kLazyWindow * DH);
    s.coef.alloc(2 * B * NH * kLazyWindow);
    s.gsc.alloc(2 * B * NH);
    if (!mlstm_lazy_fused_scores((int)DH)) {
      s.pw.alloc(B * NH * 4 * kLazyWT);
      s.pw.zero();
    }
    s.coef.zero();
  }
  e->LZ_COUNT.alloc(2 * B);
  e->LZ_COUNT.zero();
  for (int i = 0; i < c.n_blocks; ++i) {
    if (c.block_is_slstm[i]) continue;
    BlockState& s = e->st[i];
    for (int p = 0; p < 2; ++p)
      launch_mlstm_lazy_clear(reinterpret_cast<int32_t*>(e->LZ_COUNT.p) + p * B, s.gsc.p + p * B * NH, nullptr, (int)B,
                              (int)NH, nullptr);
  }
  LRAM_HIP_CHECK(hipDeviceSynchronize());
  e->lazy_step = 0;
  e->parked_dirty_step = 0;
  e->prefold = lram_engine::Prefold{};
  e->lazy_ready = true;
  slot_segments_build(e);
}

// auto: lazy where the state pass dominates -- one mLSTM block's matrix memory of at least 128 MiB over the batch
// (16M geometry from 128 env slots, 206M from 21); below that the extra launches per block cost more than the saved
// bytes.  Round 6, one box, lazy vs materialised env-steps/s: 16M at 128 / 256 / 384 envs 151.4k vs 145.4k / 207.2k vs 191.0k /
// 269.8k vs 233.1k; 206M at 8 / 16 / 32 / 64 envs 3.27k vs 3.69k / 6.00k vs 6.13k / 9.78k vs 9.33k / 12.35k vs 11.21k.
// (Rounds 2-5 used 512 MiB, from round 2's kernels: 16M at 256 envs 174k lazy vs 178k materialised then.)
bool lazy_choice(const lram_engine* e) {
  if (e->lazy_mode == 0 || !lazy_geometry_ok(e)) return false;
  if (e->lazy_mode == 1) return true;
  return mlstm_block_bytes(e) >= 128.0 * 1024 * 1024;
}

// Environment knobs of lram_create (measurement / test switches), in the order of the table in DESIGN.md section 5.  (The projection
// launchers' four knobs are read beside this table, by gemm_knobs_from_env().)
struct Knob {
  const char* name;
  void (*set)(lram_engine& e, const char* v);
};
const Knob kKnobs[] = {
    {"LRAM_STATE", [](lram_engine& e, const char* v) {
       const std::string m(v);
       e.lazy_mode = m == "lazy" ? 1 : (m == "eager" || m == "materialised" || m == "materialized") ? 0 : 2;
     }},
    {"LRAM_LAZY_PERIOD", [](lram_engine& e, const char* v) { e.lazy_period = std::max(1, std::min(14, std::atoi(v))); }},
    {"LRAM_LAZY_CAP2_ENVS", [](lram_engine& e, const char* v) { e.lazy_cap2_envs = std::max(0, std::atoi(v)); }},
    {"LRAM_FOLD_TAIL", [](lram_engine& e, const char* v) { e.fold_tail = std::atoi(v) != 0; }},
    {"LRAM_GN_FUSE", [](lram_engine& e, const char* v) { e.gn_fuse = std::max(0, std::min(2, std::atoi(v))); }},
    {"LRAM_GEMM", [](lram_engine& e, const char* v) {
       const std::string kind(v);
       e.use_bf16x3 = kind != "f32", e.use_f16x2 = kind != "f32" && kind != "bf16x3";
     }},
    {"LRAM_F16_MIN_ROWS", [](lram_engine& e, const char* v) { e.f16x2_min_rows = std::max(9, std::atoi(v)); }},
    {"LRAM_GEMM_PRESPLIT", [](lram_engine& e, const char* v) { e.gemm_presplit = std::atoi(v) != 0; }},
    {"LRAM_GEMM_NARROW", [](lram_engine& e, const char* v) { e.gemm_narrow_on = std::atoi(v) != 0, e.gemm_narrow_f16 = std::atoi(v) != 2; }},
    {"LRAM_UPZ_8P", [](lram_engine& e, const char* v) { e.upz_beside = std::atoi(v) != 0; }},
    {"LRAM_SLSTM_GATES_ONE", [](lram_engine& e, const char* v) { e.slstm_gates_one = std::atoi(v) != 0; }},
    {"LRAM_GN_AMAX", [](lram_engine& e, const char* v) { e.gn_amax_handover = std::atoi(v) != 0, e.gn_planes = std::atoi(v) >= 2; }},
    {"LRAM_GEMM_SKINNY_ROWS", [](lram_engine& e, const char* v) { e.gemm_skinny_rows = std::max(0, std::atoi(v)); }},
    {"LRAM_GEMM_SKINNY_MIN", [](lram_engine& e, const char* v) { e.gemm_skinny_min = std::max(1, std::atoi(v)); }},
    {"LRAM_SLSTM_FUSED_ROWS", [](lram_engine& e, const char* v) { e.slstm_fused_rows = std::max(0, std::atoi(v)); }},
    {"LRAM_SLSTM_SEQ", [](lram_engine& e, const char* v) { e.slstm_seq = std::atoi(v) != 0, e.slstm_seq_f32 = std::atoi(v) == 2; }},
    {"LRAM_FRONT_MULTI", [](lram_engine& e, const char* v) { e.front_multi = std::atoi(v) != 0; }},
    {"LRAM_FRONT_MIN_ENVS", [](lram_engine& e, const char* v) { e.front_min_envs = std::max(1, std::atoi(v)); }},
    {"LRAM_FRONT_EPW", [](lram_engine& e, const char* v) { e.front_epw = std::max(0, std::min(64, std::atoi(v))); }},
    {"LRAM_MAMBA_DT_FUSE", [](lram_engine& e, const char* v) { e.mamba_dt_fuse = std::atoi(v) != 0; }},
    {"LRAM_COMPAT_SHARE", [](lram_engine& e, const char* v) { e.compat_share = std::atoi(v) != 0; }},
    {"LRAM_PREFILL_CHUNK", [](lram_engine& e, const char* v) {
       e.chunk_prefill = std::atoi(v) != 0, e.chunk_exact_fp32 = std::atoi(v) == 2, e.chunk_lanes = std::atoi(v) != 3;
     }},
    {"LRAM_SCORE_ROWS", [](lram_engine& e, const char* v) { e.score_rows = std::max(lram_engine::kScoreMinRows, std::atoi(v)); }},
    {"LRAM_IMG_TILE", [](lram_engine& e, const char* v) { e.img_tile = std::max(1, std::min(kConvMaxFrames, std::atoi(v))); }},
    {"LRAM_EVENT_SCOPE", [](lram_engine& e, const char* v) { e.event_device_scope = std::string(v) != "system"; }},
};

void state_alloc(lram_engine* e, int B) {
  LRAM_REQUIRE(e->finalized, "lram_finalize must be called before lram_state_alloc");
  LRAM_REQUIRE(B > 0 && B <= 65535, "batch must be in 1..65535");
  LRAM_HIP_CHECK(hipSetDevice(e->device));
  e->drop_graph();
  e->release_state();
  e->drop_slot_table();   // the table describes the slots of one allocation
  e->drop_sample_slots(); // and so do the per-slot sampling settings
  e->drop_action_mask();  // and the allowed-action sets
  const lram_config& c = e->cfg;
  const size_t D = c.d_model;
  e->st.resize(c.n_blocks);
  for (int i = 0; i < c.n_blocks; ++i) {
    BlockState& s = e->st[i];
    if (c.backbone == LRAM_BACKBONE_MAMBA) {
      s.s0.alloc((size_t)B * c.d_inner * c.d_state);
      s.conv.alloc((size_t)B * c.d_inner * c.d_conv);
    } else if (c.block_is_slstm[i]) {
      s.s0.alloc(4 * (size_t)B * D);
      s.conv.alloc((size_t)B * c.conv_k * D);
    } else {
      const size_t DH = e->dh();
      s.s0.alloc((size_t)B * c.n_heads * DH * DH);
      s.n.alloc((size_t)B * c.inner);
      s.m.alloc((size_t)B * c.n_heads);
      s.conv.alloc((size_t)B * c.conv_k * c.inner);
    }
    s.s0.zero();
    s.n.zero();
    s.m.zero();
    s.conv.zero();
  }
  e->B = B;
  e->n_live = B;
  e->ctx_rows = LRAM_CONTEXT_ROWS_ALL;
  alloc_workspace(e, kMaxTokens);
  e->lazy = lazy_choice(e);
  if (e->lazy) lazy_alloc(e);
  if (e->slot_segs_dev == nullptr) slot_segments_build(e);
  LRAM_HIP_CHECK(hipDeviceSynchronize());
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* lram_last_error(void) { return g_last_error.c_str(); }

int32_t lram_abi_version(void) { return LRAM_ABI_VERSION; }

int32_t lram_create(const lram_config* cfg, int32_t device, lram_engine** out) {
  return guarded([&] {
    LRAM_REQUIRE(cfg != nullptr && out != nullptr, "lram_create: null argument");
    validate_config(*cfg);
    int ndev = 0;
    LRAM_HIP_CHECK(hipGetDeviceCount(&ndev));
    LRAM_REQUIRE(device >= 0 && device < ndev, "lram_create: no such HIP device");
    LRAM_HIP_CHECK(hipSetDevice(device));
    auto e = std::make_unique<lram_engine>();
    e->cfg = *cfg;
    e->device = device;
    // Environment knobs (measurement / test switches; the table is in DESIGN.md section 5)
    e->gemm_knobs = gemm_knobs_from_env();   // the projection launchers' knobs: this engine's from here on
    for (const Knob& k : kKnobs)
      if (const char* v = std::getenv(k.name)) k.set(*e, v);
    *out = e.release();
  });
}

int32_t lram_destroy(lram_engine* e) {
  return guarded([&] {
    if (e) {
      (void)hipSetDevice(e->device);
      delete e;
    }
  });
}

int32_t lram_set_weight(lram_engine* e, const char* name, const float* host_data, size_t numel) {
  return guarded([&] {
    LRAM_REQUIRE(e && name && host_data && numel > 0, "lram_set_weight: bad argument");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    DevBuf& b = e->weights[name];
    b.alloc(numel);
    LRAM_HIP_CHECK(hipMemcpy(b.p, host_data, numel * sizeof(float), hipMemcpyHostToDevice));
    e->finalized = false;
    e->drop_graph();
  });
}

int32_t lram_finalize(lram_engine* e) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_finalize: null engine");
    finalize(e);
  });
}

int32_t lram_state_alloc(lram_engine* e, int32_t batch) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_state_alloc: null engine");
    state_alloc(e, batch);
  });
}

int64_t lram_state_bytes_per_env(const lram_engine* e) {
  if (!e) return 0;
  const lram_config& c = e->cfg;
  int64_t elems = 0;
  for (int i = 0; i < c.n_blocks; ++i) {
    if (c.backbone == LRAM_BACKBONE_MAMBA) {
      elems += (int64_t)c.d_inner * (c.d_state + c.d_conv);
    } else if (c.block_is_slstm[i]) {
      elems += (int64_t)c.d_model * (4 + c.conv_k);
    } else {
      const int64_t DH = c.inner / c.n_heads;
      elems += (int64_t)c.n_heads * DH * DH + c.inner + c.n_heads + (int64_t)c.conv_k * c.inner;
    }
  }
  return elems * 4;
}

int32_t lram_set_graph_mode(lram_engine* e, int32_t enable) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_set_graph_mode: null engine");
    if (e->prefold.pending || (enable != 0 && e->lazy_ready)) {  // graph replay bakes kernel arguments: it runs on the materialised state
      LRAM_HIP_CHECK(hipSetDevice(e->device));
      // steps may still be in flight on a non-blocking caller stream, which the null stream does not order against:
      // drain the device before the folds touch the windows and C
      LRAM_HIP_CHECK(hipDeviceSynchronize());
      if (enable != 0)
        lazy_materialize(e, nullptr);
      else
        lazy_finish_prefold(e, nullptr);
      LRAM_HIP_CHECK(hipDeviceSynchronize());
    }
    e->graph_mode = enable != 0;
    if (!e->graph_mode) e->drop_graph();
  });
}

int32_t lram_set_state_mode(lram_engine* e, int32_t mode, int32_t fold_period) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_set_state_mode: null engine");
    LRAM_REQUIRE(mode >= 0 && mode <= 2, "lram_set_state_mode: mode must be 0 (materialised), 1 (lazy) or 2 (auto)");
    LRAM_REQUIRE(fold_period == 0 || (fold_period >= 1 && fold_period * e->cfg.tokens_per_step + 4 <= kLazyWindow),
                 "lram_set_state_mode: fold_period out of range (the window holds 48 tokens)");
    LRAM_REQUIRE(mode != 1 || lazy_geometry_ok(e),
                 "lram_set_state_mode: lazy matrix memory needs an xLSTM head dim that is a multiple of 128 and at least one mLSTM block");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    if (e->lazy_ready) {  // leave the current mode with a materialised state
      LRAM_HIP_CHECK(hipDeviceSynchronize());  // pending steps on non-blocking streams first (see lram_set_graph_mode)
      lazy_materialize(e, nullptr);
      LRAM_HIP_CHECK(hipDeviceSynchronize());
    }
    e->lazy_mode = mode;
    if (fold_period > 0) e->lazy_period = fold_period;
    e->lazy_bound.clear();
    e->lazy = e->B > 0 && lazy_choice(e);
    if (e->lazy) lazy_alloc(e);
  });
}

int32_t lram_get_state_mode(const lram_engine* e) { return (e != nullptr && e->lazy && e->lazy_ready) ? 1 : 0; }

int32_t lram_set_micro_batches(lram_engine* e, int32_t n) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr && n >= 0 && n <= 8, "lram_set_micro_batches: n must be in 0..8 (0 = auto)");
    if (e->prefold.pending) {  // the tail fold belongs to the two-slice schedule: complete it (null stream: drain first, as in
      LRAM_HIP_CHECK(hipSetDevice(e->device));   // lram_set_graph_mode)
      LRAM_HIP_CHECK(hipDeviceSynchronize());
      lazy_finish_prefold(e, nullptr);
      LRAM_HIP_CHECK(hipDeviceSynchronize());
    }
    e->n_micro = n;
    e->drop_graph();
  });
}

int32_t lram_set_compat_mode(lram_engine* e, int32_t mamba_repeat, int32_t stale_state) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_set_compat_mode: null engine");
    LRAM_REQUIRE(mamba_repeat >= 1 && mamba_repeat <= 64, "lram_set_compat_mode: mamba_repeat must be in 1..64");
    LRAM_REQUIRE(e->cfg.backbone == LRAM_BACKBONE_MAMBA || (mamba_repeat == 1 && stale_state == 0),
                 "lram_set_compat_mode: the repeated-forward / stale-state quirks belong to the reference's Mamba agent "
                 "(src/algos/decision_mamba.py); the xLSTM agent does a single forward and drops the whole cache");
    if (e->compat_repeat != mamba_repeat || e->compat_stale != (stale_state != 0)) e->drop_graph();
    e->compat_repeat = mamba_repeat;
    e->compat_stale = stale_state != 0;
  });
}

int32_t lram_set_sampling(lram_engine* e, int32_t enable, double temperature, int32_t top_k, double top_p, uint64_t seed,
                          uint64_t slot_base) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_set_sampling: null engine");
    if (enable) {
      LRAM_REQUIRE(temperature > 0.0 && temperature < (double)INFINITY,
                   "lram_set_sampling: temperature must be finite and > 0 (it multiplies the logits)");
      LRAM_REQUIRE(top_p >= 0.0 && top_p <= 1.0, "lram_set_sampling: top_p must be in [0, 1]");
      LRAM_REQUIRE(top_k >= 0, "lram_set_sampling: top_k must be >= 0");
      LRAM_REQUIRE(top_k <= e->cfg.n_vocab, "lram_set_sampling: top_k exceeds the head's n_vocab logits");
      LRAM_REQUIRE(e->cfg.n_vocab <= kSampleMaxRow, "lram_set_sampling: the sampling kernel holds rows of up to 512 logits");
    }
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    LRAM_HIP_CHECK(hipDeviceSynchronize());  // steps in flight (non-blocking streams included) keep the mode they were launched in
    e->drop_graph();                         // the head kernel and its arguments are part of a captured step
    e->drop_sample_slots();                  // arming and disarming both start without per-slot settings
    if (enable) {
      if (!e->sample_draw) LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->sample_draw), sizeof(uint64_t)));
      LRAM_HIP_CHECK(hipMemset(e->sample_draw, 0, sizeof(uint64_t)));
      LRAM_HIP_CHECK(hipDeviceSynchronize());
      e->sample.temperature = temperature, e->sample.top_k = top_k, e->sample.top_p = top_p;
      e->sample.seed = seed, e->sample.slot0 = slot_base;
    }
    e->sampling = enable != 0;
  });
}

int32_t lram_get_sampling(lram_engine* e, int32_t* enable, double* temperature, int32_t* top_k, double* top_p, uint64_t* seed,
                          uint64_t* slot_base, uint64_t* draws) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_get_sampling: null engine");
    if (enable) *enable = e->sampling ? 1 : 0;
    if (temperature) *temperature = e->sample.temperature;
    if (top_k) *top_k = e->sample.top_k;
    if (top_p) *top_p = e->sample.top_p;
    if (seed) *seed = e->sample.seed;
    if (slot_base) *slot_base = e->sample.slot0;
    if (draws) {
      *draws = 0;
      if (e->sampling) {
        LRAM_HIP_CHECK(hipSetDevice(e->device));
        LRAM_HIP_CHECK(hipDeviceSynchronize());
        LRAM_HIP_CHECK(hipMemcpy(draws, e->sample_draw, sizeof(uint64_t), hipMemcpyDeviceToHost));
      }
    }
  });
}

int32_t lram_set_sampling_slots(lram_engine* e, const uint8_t* mode, const double* temperature, const int32_t* top_k,
                                const double* top_p) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_set_sampling_slots: null engine");
    LRAM_REQUIRE(e->B > 0, "lram_set_sampling_slots: state not allocated (call lram_state_alloc)");
    const bool clear = !mode && !temperature && !top_k && !top_p;
    LRAM_REQUIRE(clear || (mode && temperature && top_k && top_p),
                 "lram_set_sampling_slots: the four arrays go together (all NULL clears the table)");
    LRAM_REQUIRE(clear || e->sampling, "lram_set_sampling_slots: sampling is not armed (call lram_set_sampling first)");
    const int B = e->B;
    std::vector<SampleSlot> tab;
    if (!clear) {  // validate before anything changes: a refused table leaves the one in effect as it is
      tab.resize(B);
      for (int b = 0; b < B; ++b) {
        const std::string at = " (slot " + std::to_string(b) + ")";
        LRAM_REQUIRE(mode[b] <= 1, "lram_set_sampling_slots: mode must be 0 (greedy) or 1 (sample)" + at);
        LRAM_REQUIRE(temperature[b] > 0.0 && temperature[b] < (double)INFINITY,
                     "lram_set_sampling_slots: temperature must be finite and > 0 (it multiplies the logits)" + at);
        LRAM_REQUIRE(top_p[b] >= 0.0 && top_p[b] <= 1.0, "lram_set_sampling_slots: top_p must be in [0, 1]" + at);
        LRAM_REQUIRE(top_k[b] >= 0, "lram_set_sampling_slots: top_k must be >= 0" + at);
        LRAM_REQUIRE(top_k[b] <= e->cfg.n_vocab, "lram_set_sampling_slots: top_k exceeds the head's n_vocab logits" + at);
        tab[b].temperature = temperature[b], tab[b].top_p = top_p[b], tab[b].top_k = top_k[b], tab[b].mode = mode[b];
      }
    }
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    LRAM_HIP_CHECK(hipDeviceSynchronize());  // steps in flight read the table they were launched with
    e->drop_graph();                         // the head kernel and its table pointer are part of a captured step
    if (clear) {
      e->drop_sample_slots();
      return;
    }
    if (!e->sample_slots_dev)
      LRAM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->sample_slots_dev), sizeof(SampleSlot) * (size_t)B));
    LRAM_HIP_CHECK(hipMemcpy(e->sample_slots_dev, tab.data(), sizeof(SampleSlot) * (size_t)B, hipMemcpyHostToDevice));
    LRAM_HIP_CHECK(hipDeviceSynchronize());
    e->sample_slots.swap(tab);
    e->sample_slot_maxima();
  });
}

int32_t lram_get_sampling_slots(lram_engine* e, uint8_t* mode, double* temperature, int32_t* top_k, double* top_p, int32_t* set) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_get_sampling_slots: null engine");
    const bool on = !e->sample_slots.empty();
    if (set) *set = on ? 1 : 0;
    if (!on) return;
    for (size_t b = 0; b < e->sample_slots.size(); ++b) {
      const SampleSlot& t = e->sample_slots[b];
      if (mode) mode[b] = (uint8_t)t.mode;
      if (temperature) temperature[b] = t.temperature;
      if (top_k) top_k[b] = t.top_k;
      if (top_p) top_p[b] = t.top_p;
    }
  });
}

int32_t lram_get_compat_mode(const lram_engine* e, int32_t* mamba_repeat, int32_t* stale_state) {
  if (e == nullptr) return 1;
  if (mamba_repeat) *mamba_repeat = e->compat_repeat;
  if (stale_state) *stale_state = e->compat_stale ? 1 : 0;
  return 0;
}

}  // extern "C"
