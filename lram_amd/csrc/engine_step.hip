// One call from its inputs to its actions: the image and token front ends, the block stack, the action head; env-steps, repeated
// forwards, stored contexts in chunks (lram_step, lram_step_images, lram_step_slots, lram_prefill, lram_encoder_step), and the
// head at every timestep of a stored context (lram_score, lram_score_last, lram_score_tokens).
// Calls the stacks, gemm and the streams.
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

// uint8 frames [B, C, H, W] -> state-token embeddings [B, d_model] (reference: embed_image(x / 255),
// online_decision_transformer_model.py:523-526 + image_encoders.py:58-66)
// Floats one H x W frame takes in the image work buffers.  IMG_P holds the stage conv's output before its pool: 16 channels at
// H x W in stage 1, 32 channels at the pooled size in stages 2 and 3 (the larger of the two when H or W is 1 and the other
// is odd).  IMG_X0 / IMG_X1 / IMG_T hold pooled maps: at most 32 channels of (H-1)/2+1 x (W-1)/2+1.
struct ImageFrameFloats {
  size_t p, x;
};
ImageFrameFloats image_frame_floats(int H, int W) {
  const size_t hp = (H - 1) / 2 + 1, wp = (W - 1) / 2 + 1;
  const size_t x = 32 * hp * wp;
  return {std::max((size_t)16 * H * W, x), x};
}

// Checks the frame size against the uploaded weights: everything that refuses a call for its frames, nothing allocated.
void check_frame_size(const lram_engine* e, int C, int H, int W, const char* who) {
  const std::string wh(who);
  LRAM_REQUIRE(e->img_lin_w != nullptr, wh + ": no embed_image.* weights were uploaded");
  LRAM_REQUIRE(C == e->img_channels, wh + ": channel count " + std::to_string(C) +
                                         " does not match embed_image.cnn.0.conv.weight (" + std::to_string(e->img_channels) + ")");
  int h = H, w = W;
  for (int k = 0; k < 3; ++k) h = (h - 1) / 2 + 1, w = (w - 1) / 2 + 1;
  LRAM_REQUIRE((int64_t)32 * h * w == e->img_flat, wh + ": image size " + std::to_string(H) + " x " + std::to_string(W) +
                                              " (pooled " + std::to_string(h) + " x " + std::to_string(w) + ", " +
                                              std::to_string((int64_t)32 * h * w) + " features) does not match embed_image.linear.0.weight (" +
                                              std::to_string(e->img_flat) + " features)");
}

// ... then makes the image work buffers hold `frames` frames of H x W (an env-step: the batch; a frame list: the larger of the
// batch and its tile): every buffer by what it holds at this size, each grown on its own need (two sizes that feed the same
// linear layer can differ in which of them has the larger pooled map).  A region starts at a multiple of the per-frame size, so
// growing a buffer moves nobody's region.  Synchronises when it has to grow one: never called between a fork and a join.
void image_buffers(lram_engine* e, int C, int H, int W, const char* who, size_t frames = 0) {
  check_frame_size(e, C, H, W, who);
  const ImageFrameFloats f = image_frame_floats(H, W);
  const size_t B = std::max((size_t)e->B, frames), np = B * f.p, nx = B * f.x;
  if (np <= e->IMG_P.n && nx <= e->IMG_X0.n && nx <= e->IMG_X1.n && nx <= e->IMG_T.n) return;
  LRAM_HIP_CHECK(hipDeviceSynchronize());
  if (np > e->IMG_P.n) e->IMG_P.alloc(np);
  for (DevBuf* b : {&e->IMG_X0, &e->IMG_X1, &e->IMG_T})
    if (nx > b->n) b->alloc(nx);
}
// ... and the rows the frames of an env-step are embedded into (lram_step_images, lram_step_slots)
void step_image_buffers(lram_engine* e, int C, int H, int W, const char* who) {
  image_buffers(e, C, H, W, who);
  if (e->IMG_EMB.n < (size_t)e->B * e->cfg.d_model) {
    LRAM_HIP_CHECK(hipDeviceSynchronize());
    e->IMG_EMB.alloc((size_t)e->B * e->cfg.d_model);
  }
}

// The three conv stages over B frames, their maps in the work buffers from frame region r0 on (every env slice of a step keeps
// to its own fixed region, so slices at different stages of the CNN never touch each other's maps).  The last map -- act_flatten's
// ReLU applied, NCHW: a row of the Linear's operand -- goes to `flat` [B, img_flat].  With a frame list the first conv reads frame
// list[2 * k] of `images` as its k-th; without one, frame k.
void cnn_stages(lram_engine* e, const uint8_t* images, const int32_t* list, int H, int W, int B, size_t r0, float* flat, hipStream_t s) {
  const ImageFrameFloats f = image_frame_floats(H, W);
  const size_t end = r0 + (size_t)B;
  LRAM_REQUIRE(end * f.p <= e->IMG_P.n && end * f.x <= e->IMG_X0.n && end * f.x <= e->IMG_X1.n && end * f.x <= e->IMG_T.n,
               "image work buffers not allocated");
  float* const P = e->IMG_P.p + r0 * f.p;
  float* const X0 = e->IMG_X0.p + r0 * f.x;
  float* const X1 = e->IMG_X1.p + r0 * f.x;
  float* const Tb = e->IMG_T.p + r0 * f.x;
  const void* in = images;
  int in_u8 = 1;
  int h = H, w = W;
  for (int sidx = 0; sidx < 3; ++sidx) {
    const lram_engine::ImgConv* cv = e->img_conv[sidx];
    auto conv = [&](const lram_engine::ImgConv& c, const void* src, int u8, int relu_in, const float* res, float* dst,
                    int relu_out, const int32_t* frame_list = nullptr) {
      Conv3x3Args a;
      a.in = src, a.w = c.w, a.bias = c.b, a.residual = res, a.out = dst, a.src = frame_list;
      a.B = B, a.CIN = c.cin, a.COUT = c.cout, a.H = h, a.W = w, a.in_relu = relu_in, a.out_relu = relu_out, a.in_u8 = u8;
      launch_conv3x3(a, s);
    };
    conv(cv[0], in, in_u8, 0, nullptr, P, 0, sidx == 0 ? list : nullptr);
    launch_maxpool3s2(P, X0, (int64_t)B * cv[0].cout, h, w, s);
    h = (h - 1) / 2 + 1, w = (w - 1) / 2 + 1;
    conv(cv[1], X0, 0, 1, nullptr, Tb, 0);
    conv(cv[2], Tb, 0, 1, X0, X1, 0);
    conv(cv[3], X1, 0, 1, nullptr, Tb, 0);
    conv(cv[4], Tb, 0, 1, X1, sidx == 2 ? flat : X0, sidx == 2 ? 1 : 0);  // act_flatten's ReLU on the last map
    in = X0;
    in_u8 = 0;
  }
  // stage s > 0 reads X0 and writes P, then pools back into X0: no aliasing within a launch
}

// envs b0 .. b0 + nb - 1 of an env-step (`images` / `out` point at env b0's frame / row)
void embed_images(lram_engine* e, const uint8_t* images, int C, int H, int W, float* out, hipStream_t s, int b0 = 0, int nb = -1) {
  const int B = nb < 0 ? e->B : nb, D = e->cfg.d_model;
  // (image_buffers has checked C, H, W against the weights; the env slices of one call share its buffers)
  float* const X0 = e->IMG_X0.p + (size_t)b0 * image_frame_floats(H, W).x;
  cnn_stages(e, images, nullptr, H, W, B, (size_t)b0, X0, s);
  GemmArgs g;
  g.a = X0, g.lda = e->img_flat, g.w = e->img_lin_w, g.ldw = e->img_flat, g.c = out, g.ldc = D;
  g.bias = e->img_lin_b, g.m = B, g.n = D, g.k = e->img_flat;
  gemm(e, g, s);
  launch_relu(out, (int64_t)B * D, s);
}

// ---- stored contexts from frames: the frame list -------------------------------------------------------------------------
// Frames per tile at this size: the knob, capped so that one tile's maps in the four work buffers stay within 2 GiB and the
// conv's grid within kConvMaxFrames.
int64_t frame_tile(const lram_engine* e, int H, int W) {
  const ImageFrameFloats f = image_frame_floats(H, W);
  const int64_t cap = std::max<int64_t>(1, (int64_t)(((size_t)1 << 29) / (f.p + 3 * f.x)));
  return std::min<int64_t>({(int64_t)e->img_tile, cap, (int64_t)kConvMaxFrames});
}

// What a call of N listed frames needs beyond the work buffers: the list, the Linear's operand and its compact output rows.
// check: refused, with nothing allocated or launched, when the operand would exceed 2 GiB.
void check_frame_list(const lram_engine* e, int64_t N, const char* who) {
  LRAM_REQUIRE((size_t)N * (size_t)e->img_flat <= ((size_t)1 << 29) && (size_t)N * (size_t)e->cfg.d_model <= ((size_t)1 << 29),
               std::string(who) + ": the flattened maps of " + std::to_string(N) + " frames (" + std::to_string(e->img_flat) +
                   " features each) exceed 2 GiB: split the call");
}
void frame_list_buffers(lram_engine* e, int C, int H, int W, int64_t N, const char* who) {
  image_buffers(e, C, H, W, who, (size_t)std::min<int64_t>(N, frame_tile(e, H, W)));
  const size_t flat = (size_t)N * e->img_flat, rows = (size_t)N * e->cfg.d_model, list = (size_t)2 * N;
  if (e->IMG_FLAT.n >= flat && e->IMG_ROWS.n >= rows && e->IMG_LIST.n >= list) return;
  LRAM_HIP_CHECK(hipDeviceSynchronize());
  if (e->IMG_FLAT.n < flat) e->IMG_FLAT.alloc(flat);
  if (e->IMG_ROWS.n < rows) e->IMG_ROWS.alloc(rows);
  if (e->IMG_LIST.n < list) e->IMG_LIST.alloc(list);
}

// The N frames IMG_LIST names -> relu(Linear(cnn(frame src))) in row dst of `out` [., d_model]: the conv stages tile by tile,
// one Linear over all N rows (the result does not depend on the tile), ReLU + placement.  Buffers by frame_list_buffers.
void embed_frame_list(lram_engine* e, const uint8_t* frames, int H, int W, int64_t N, float* out, hipStream_t s) {
  const int D = e->cfg.d_model;
  const int64_t F = frame_tile(e, H, W);
  const int32_t* list = reinterpret_cast<const int32_t*>(e->IMG_LIST.p);
  for (int64_t t0 = 0; t0 < N; t0 += F) {
    cnn_stages(e, frames, list + 2 * t0, H, W, (int)std::min(F, N - t0), 0, e->IMG_FLAT.p + (size_t)t0 * e->img_flat, s);
    e->img_counts[1] += 1;
  }
  GemmArgs g;
  g.a = e->IMG_FLAT.p, g.lda = e->img_flat, g.w = e->img_lin_w, g.ldw = e->img_flat, g.c = e->IMG_ROWS.p, g.ldc = D;
  g.bias = e->img_lin_b, g.m = (int)N, g.n = D, g.k = e->img_flat;
  gemm(e, g, s);
  launch_relu_place_rows(e->IMG_ROWS.p, list, out, N, D, s);
  e->img_counts[0] += N, e->img_counts[2] += 1;
}

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
// starting at call-timestep L - n_b, and the chunks are cut so that every env starts on a chunk boundary (context_plan below).
// An env restarts at its own first timestep where its row of that chunk's mask says so; in an append call an env that has not
// started by a chunk is held in it (Pass::hold).  Device pointers into lram_engine::CTX, filled on the call's stream ahead of the
// first chunk.
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

// The frames of a stored-context call that count, and the envs that hand frames in: the image slots of a slot table (every env
// without one) among the call's rows (lram_engine::context_rows), each with its own length (null: all L).
struct FrameCount {
  int n_env;
  int64_t frames;
};
FrameCount count_frames(const lram_engine* e, int L, const int32_t* lengths) {
  FrameCount n{0, 0};
  for (int b = 0; b < e->context_rows(); ++b)
    if (!e->slot_table || (e->slot_flags[b] & LRAM_SLOT_IMAGE)) n.n_env += 1, n.frames += lengths ? lengths[b] : L;
  return n;
}

// Token front end of one env slice for the chunk of Lc timesteps that starts at timestep l: embeds the chunk's tokens into the
// slice's rows of X and applies embed_ln.  seq_emb: the state embeddings of a stored context, made ahead of the chunks.
void embed_tokens(lram_engine* e, const Pass& pass, const Inputs& in, const float* seq_emb, const Slice& x, int l, int Lc,
                  const ContextPlan* plan = nullptr) {
  const lram_config& c = e->cfg;
  const int D = c.d_model, T = c.tokens_per_step, Tc = T * Lc, L = in.L, emb = in.emb;
  const int64_t obs_w = emb ? D : c.state_dim;
  const float *obs = in.obs, *rtg = in.rtg, *rew = in.rew;
  const size_t r0 = (size_t)x.b0 * Tc, b0 = x.b0;
  float* X = e->X.p + r0 * D;
  if (plan != nullptr) {  // per-env lengths: every env's rows from its own (left-aligned) context, zeros ahead of it
    LRAM_REQUIRE(seq_emb != nullptr, "ragged context: no state embeddings");
    launch_embed_chunk_ragged(X, seq_emb + b0 * L * D, (int64_t)L * D, rtg + b0 * L, rew + b0 * L, L, plan->dev_start + b0, l,
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

// The engine's head geometry, and the slot table of a call as the slice from env slot b0 on sees it (none unless the call is
// per-slot).
HeadGeom head_geom(const lram_config& c) { return {c.act_dim, c.n_vocab, c.n_discrete, c.action_channels, c.tok_min, c.tok_max}; }
HeadSlots head_slots(const lram_engine* e, int discrete, size_t b0 = 0) {
  if (discrete != LRAM_HEAD_PER_SLOT) return {};
  return {e->slot_dev + b0, e->slot_dev + e->B + b0};
}

// The allowed-action sets as the slice from env slot b0 on sees them ({null, 0} without a mask: the unmasked kernels).
HeadMask head_mask(const lram_engine* e, size_t b0 = 0) {
  if (e->mask_dev == nullptr) return {};
  return {e->mask_dev + b0 * (size_t)e->mask_words, e->mask_words};
}
// A discrete = 1 call reads [0, n_discrete) on every slot: refused, before anything is launched, while some slot allows nothing there.
void check_head_mask(const lram_engine* e, int discrete, const std::string& w) {
  LRAM_REQUIRE(!(discrete == 1 && e->mask_no_discrete_at >= 0),
               w + ": the action mask (lram_set_action_mask) allows slot " + std::to_string(e->mask_no_discrete_at) +
                   " nothing below n_discrete: a discrete = 1 call would leave it an empty sub-row");
}

// What every score launch of a call shares: the head's geometry, the sink's tensors, the slot table of a per-slot call.
ScoreArgs score_args(const lram_engine* e, const ScoreSink& k, int discrete) {
  ScoreArgs a;
  a.geom = head_geom(e->cfg), a.slots = head_slots(e, discrete);
  a.discrete = discrete == LRAM_HEAD_PER_SLOT ? 0 : discrete;
  a.over = k.over, a.temperature = k.temperature;
  a.target_actions = k.target_actions, a.target_tokens = k.target_tokens, a.valid = k.valid;
  a.actions = k.actions, a.tokens = k.tokens, a.logp = k.logp, a.logits_out = k.logits;
  return a;
}

// The head at EVERY timestep of the chunk of Lc timesteps from l0 on that the slice has just run through the stack: the chunk's
// action-token rows of HID (row (b, l) at ((b * Lc + l) * T + pred) * D: one stride) against action_net, in blocks of at most
// `cap` rows into the region's scratch, each block scored into rows [b, l0 + l] of the sink.  The exact fp32 matrix-core kernel
// without split-K: a row's logits are one k-ordered fma chain whatever the block it falls into, so the outputs do not depend
// on the scratch bound.  (A last block of <= 8 rows would take the GEMV kernel, another summation order: it starts
// kScoreMinRows before the end instead and recomputes the rows it overlaps.)
void score_chunk(lram_engine* e, const ScoreSink& k, const Slice& x, float* scratch, int64_t cap, int l0, int Lc, int L,
                 int discrete, const int32_t* ctx_start = nullptr) {
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
    gh.m = (int)nr, gh.n = (int)nlog, gh.k = D;
    launch_gemm_f32(gh, x.s);
    count_gemm(e, 2, gh);
    ScoreArgs a = score_args(e, k, discrete);
    a.logits = scratch, a.ld = nlog, a.row0 = (int64_t)x.b0 * Lc + beg, a.rows = nr;
    a.inner = Lc, a.outer = L, a.off = l0, a.start = ctx_start;
    launch_action_score(a, x.s, head_mask(e));
  }
}

// Action head on the last timestep of the last chunk (Tc tokens per env, last_steps timesteps): logits per env slice, then
// argmax or a sampled draw.  What discrete = LRAM_HEAD_PER_SLOT needs was checked by the entry (check_head_mode).
// With a sink (lram_score over L timesteps) the same logits are scored into row [b, L - 1] of the sink's tensors instead: no draw.
void action_head(lram_engine* e, const Pass& pass, const std::vector<Slice>& sl, int Tc, int last_steps, int discrete,
                 float* actions, int32_t* tokens, const ScoreSink* sink = nullptr, int L = 1, const int32_t* ctx_start = nullptr) {
  const lram_config& c = e->cfg;
  const int D = c.d_model, T = c.tokens_per_step;
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
    if (sink != nullptr) {
      ScoreArgs a = score_args(e, *sink, discrete);
      a.logits = e->LOGITS.p + b0 * nlog, a.ld = nlog, a.row0 = (int64_t)b0, a.rows = x.nb;
      a.inner = 1, a.outer = L, a.off = L - 1, a.start = ctx_start;
      launch_action_score(a, x.s, head_mask(e));
      continue;
    }
    const float* logits = e->LOGITS.p + b0 * nlog;
    float* act = actions + b0 * c.act_dim;
    int32_t* tok = tokens ? tokens + b0 * c.act_dim : nullptr;
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

// L consecutive timesteps for every env slot (L = 1: one env-step).  The reset mask applies before the first timestep; the
// action head runs on the last timestep only (and only if an output buffer is given).  One fork / join of the slice streams
// brackets the whole call -- of repeated forwards (call.compat_passes > 1): one fork ahead of the first, one join behind the last.
// With a sink (lram_score; `actions` is then null) the head runs at every timestep: after the stack pass of every chunk, on
// that chunk's stream and workspace (score_chunk), and once more on the last timestep through the very launches a call without
// a sink makes for it (action_head) -- row [b, L - 1] of the sink is what lram_prefill computes, and LOGITS is left as it leaves it.
// With a plan (per-env lengths) the chunks are the plan's instead of the fixed stride, chunk c takes row c of the plan's reset
// masks instead of `reset` on the first chunk, and the front end and the sink place every env's rows by its own start.
// The rows of a stored context are R = lram_engine::context_rows() -- the batch, or the live prefix (lram_set_context_rows); an
// env-step's are the slices' (make_slices: the live prefix).  A plan with per-chunk rows clips every chunk's slices to them.
void timesteps_launches(lram_engine* e, const Pass& call, const Inputs& in, const uint8_t* reset, int discrete, float* actions,
                        int32_t* tokens, hipStream_t s, const ScoreSink* sink = nullptr, const ContextPlan* plan = nullptr) {
  const lram_config& c = e->cfg;
  const int D = c.d_model, T = c.tokens_per_step, L = in.L, R = e->context_rows();
  e->sync_used = 0, e->edge_used = 0;
  // Stored context is consumed in chunks: every block then reads and writes its recurrent state once per chunk
  // instead of once per timestep.  Up to 4 timesteps (12 tokens) per chunk through the token-sequential kernels,
  // up to 21 (63 tokens) through the chunkwise matrix-core kernels (mlstm_chunk.hip).
  const int kChunk = L > 1 ? prefill_chunk_steps(e, L) : 1;
  if (L > 1 || !lazy_active(e, T)) lazy_materialize(e, s);  // stored contexts go through the materialised kernels
  // Stored contexts: the state embeddings of ALL timesteps as one GEMM ahead of the chunks (rows b * L + l, as the input lies),
  // instead of one few-row GEMM per timestep (206M, 64 envs x 512 timesteps: 1024 launches of 12-26 us -> 1 + one per chunk)
  const float* seq_emb = nullptr;
  // (a call from frames has no other front end: its entry has refused what would not get here)
  if ((L > 1 || plan != nullptr || in.frames != nullptr) && T == 3 && D % 4 == 0 && !call.compat_shared) {
    if (in.emb) {
      seq_emb = in.obs;
    } else if ((size_t)R * L * D <= ((size_t)1 << 29)) {   // <= 2 GiB
      const FrameCount fc = in.frames ? count_frames(e, L, plan ? plan->lengths : nullptr) : FrameCount{0, 0};
      if (fc.frames > 0) frame_list_buffers(e, in.img_c, in.img_h, in.img_w, fc.frames, "stored context from frames");
      if (e->SEQ_EMB.n < (size_t)R * L * D) {
        LRAM_HIP_CHECK(hipDeviceSynchronize());
        e->SEQ_EMB.alloc((size_t)R * L * D);
      }
      if (in.obs != nullptr) {   // (from frames: the vector slots of a mixed table; the image slots' rows are overwritten below)
        GemmArgs ge;
        ge.a = in.obs, ge.lda = c.state_dim, ge.w = e->w_state, ge.ldw = c.state_dim, ge.c = e->SEQ_EMB.p, ge.ldc = D;
        ge.bias = e->b_state, ge.m = R * L, ge.n = D, ge.k = c.state_dim;
        gemm(e, ge, s);
      }
      // Frames: the third source.  The list of the frames that count is built on the device from the per-env starts and the
      // slot table's image list; the CNN embeds exactly those into their rows b * L + l -- a padded frame is never read.
      if (fc.frames > 0) {   // (0: a mixed table whose image slots all have length 0)
        launch_frame_list(reinterpret_cast<int32_t*>(e->IMG_LIST.p), plan ? plan->dev_start : nullptr,
                          e->slot_table ? e->slot_img_list : nullptr, fc.n_env, L, s);
        embed_frame_list(e, in.frames, in.img_h, in.img_w, fc.frames, e->SEQ_EMB.p, s);
      }
      seq_emb = e->SEQ_EMB.p;
    }
  }
  LRAM_REQUIRE(in.frames == nullptr || seq_emb != nullptr, "stored context from frames: no state embeddings");
  // chunk lanes (see lram_engine::chunk_lanes): the last chunk -- the one the action head reads -- is on lane 0 = the primary
  // workspace and the caller's stream.  Where they apply they replace the automatic env slices of large batches as well: whole-batch
  // launches, three chunks in flight (16M, 1024 envs x 252 timesteps: 224.4 -> 215.5 ms; 206M, 512 envs x 63: 295.3 -> 274.0 ms).
  std::vector<int> chunk_at;   // first timestep of every chunk, and L
  if (plan != nullptr)
    chunk_at = plan->starts;
  else
    for (int l = 0; l < L; l += kChunk) chunk_at.push_back(l);
  chunk_at.push_back(L);
  const int n_chunks = (int)chunk_at.size() - 1;
  const int32_t* ctx_start = plan ? plan->dev_start : nullptr;
  // (Mamba's stored contexts and the xLSTM geometries without a chunkwise form go through the token-sequential kernels in chunks
  // of 4 timesteps: the lanes apply to them as they are)
  const bool lanes = e->n_micro <= 1 && n_chunks >= 2 && e->chunk_lanes && !e->graph_mode && !call.compat_shared && twin_ready(e);
  hipStream_t hbm = s;
  const std::vector<Slice> sl = lanes ? std::vector<Slice>{Slice{0, R, s}} : make_slices(e, s, &hbm);
  const bool multi = sl.size() > 1;
  const int NL = lanes ? e->n_lanes : 1;
  // scratch of the per-timestep head: one region per lane / slice (a one-timestep call has its only timestep scored by action_head)
  const int64_t score_cap = std::max<int64_t>(lram_engine::kScoreMinRows, std::min<int64_t>(e->score_rows, (int64_t)R * kChunk));
  const size_t score_region = (size_t)score_cap * c.act_dim * c.n_vocab;
  if (sink != nullptr && L > 1) {
    const size_t want = score_region * (lanes ? (size_t)NL : sl.size());
    if (e->SCORE_LG.n < want) {
      LRAM_HIP_CHECK(hipDeviceSynchronize());
      e->SCORE_LG.alloc(want);
    }
  }
  if (multi && call.compat_pass == 0) fork_slices(e, sl, hbm, s);
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
    const int l = chunk_at[ci], Lc = chunk_at[ci + 1] - l;
    Tc = T * Lc;
    last_steps = Lc;
    const int lane = (n_chunks - 1 - ci) % NL;
    if (lanes)
      use.assign(1, Slice{0, started ? plan->rows[ci] : R, lane_s[lane]}), use_idx.assign(1, (size_t)lane);
    else if (started)
      clip_slices(plan->rows[ci]);
    else if (ci == 0)
      clip_slices(sl.back().b0 + sl.back().nb);
    if (call.context) e->ctx_counts[1] += 1, e->ctx_counts[2] += (int64_t)(use.back().b0 + use.back().nb) * Lc;
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
    if (plan != nullptr && multi && ci > 0 && Lc != l - chunk_at[ci - 1]) {
      for (const Slice& x : sl) stream_after(e, hbm, x.s);
      for (const Slice& x : sl) stream_after(e, x.s, hbm);
    }
    // (shared repeated forwards: the tokens of this env-step were embedded by pass 0 -- X0 / U0)
    if (!(call.compat_shared && call.compat_pass > 0))
      for (const Slice& x : use) embed_tokens(e, call, in, seq_emb, x, l, Lc, plan);
    Pass pass = call;
    if (lanes) pass.lane_wait = ci > 0 ? &e->lane_ev[(lane + 1) % NL] : nullptr, pass.lane_rec = &e->lane_ev[lane];
    const uint8_t* chunk_reset = l == 0 ? reset : nullptr;
    if (plan != nullptr) chunk_reset = plan->has_reset[ci] ? plan->dev_masks + (size_t)ci * R : nullptr;
    // (a chunk without a held env passes no hold pointer: it launches what a dense call launches)
    if (plan != nullptr && plan->has_hold[ci]) pass.hold = plan->dev_hold + (size_t)ci * R;
    run_stack(e, pass, Tc, chunk_reset, use, lanes ? lane_s[lane] : hbm);
    if (sink != nullptr && L > 1)
      for (size_t i = 0; i < use.size(); ++i)
        score_chunk(e, *sink, use[i], e->SCORE_LG.p + use_idx[i] * score_region, score_cap, l, Lc, L, discrete, ctx_start);
  }
  for (int k = 1; k < NL; ++k) stream_after(e, s, lane_s[k], true);
  // the head on the rows of the last chunk (with per-chunk rows: the envs with a context; the others' rows take the fill values)
  if (started || lanes) clip_slices(started ? plan->rows.back() : R);
  if (sink != nullptr)
    action_head(e, call, use, Tc, last_steps, discrete, nullptr, nullptr, sink, L, ctx_start);
  else if (actions != nullptr)
    action_head(e, call, use, Tc, last_steps, discrete, actions, tokens);
  if (multi && call.compat_pass == call.compat_passes - 1) join_slices(e, sl, hbm, s);
}

// Sampling mode: one draw per action-producing call.  Launched on the caller's stream behind the join of the env slices
// (and behind the last of the repeated forwards), so that every row of the call has read the same count; the next call's
// slices fork from this stream and see the new one.  In a captured step it is one more node on the graph's single chain.
void sample_draw_advance(lram_engine* e, hipStream_t s) {
  if (e->sampling) launch_sample_advance(e->sample_draw, s);
}

// Per-slot sampling settings: every sampling slot's top_k must fit the head the call gives that slot -- n_discrete logits
// on a discrete head, n_vocab otherwise (checked when the table was set).  Read from the host-side maxima: no per-step cost.
void check_sample_slots(const lram_engine* e, int discrete, const std::string& w) {
  if (!e->sampling || e->sample_slots.empty() || discrete == 0) return;
  const bool per_slot = discrete == LRAM_HEAD_PER_SLOT;
  const int k = per_slot ? e->sslot_kd_max : e->sslot_k_max, at = per_slot ? e->sslot_kd_at : e->sslot_k_at;
  LRAM_REQUIRE(k <= e->cfg.n_discrete, w + ": sampling top_k " + std::to_string(k) + " of slot " + std::to_string(at) +
                                           " exceeds the n_discrete = " + std::to_string(e->cfg.n_discrete) +
                                           " logits of the discrete head that slot gets");
}

// discrete = LRAM_HEAD_PER_SLOT: what the call needs, checked before anything is launched (the recurrent state is untouched
// by a refused call).
void check_head_mode(const lram_engine* e, int discrete, const char* who) {
  // (n_discrete = 0 is a legal geometry -- the reference's dmcontrol head -- but an argmax over no logits is no action)
  LRAM_REQUIRE(discrete != 1 || e->cfg.n_discrete >= 1, std::string(who) + ": a discrete head needs n_discrete >= 1");
  check_sample_slots(e, discrete, who);
  check_head_mask(e, discrete, who);
  if (discrete != LRAM_HEAD_PER_SLOT) return;
  const std::string w(who);
  LRAM_REQUIRE(e->slot_table, w + ": LRAM_HEAD_PER_SLOT needs a slot table (lram_set_slot_table)");
  LRAM_REQUIRE(e->compat_repeat <= 1, w + ": LRAM_HEAD_PER_SLOT cannot be combined with the Mamba repeated-forward mode "
                                          "(mamba_repeat > 1 advances the state once per action dim of the env, which differs per slot)");
  LRAM_REQUIRE(!(e->sampling && e->sample_slots.empty() && e->slot_has_discrete && e->sample.top_k > e->cfg.n_discrete),
               w + ": sampling top_k exceeds n_discrete and the slot table holds a discrete slot");
}

// Do the repeated forwards of the Mamba reference-trajectory mode share the token front end and layer 0's in_proj?
bool compat_shares(const lram_engine* e, int discrete) {
  const int passes = discrete ? 1 : std::max(1, std::min(e->compat_repeat, e->cfg.act_dim));
  return passes > 1 && e->cfg.backbone == LRAM_BACKBONE_MAMBA && e->compat_share && e->cfg.n_blocks >= 2;
}
// ... then pass 0 keeps them in X0 / U0.  Called by lram_step BEFORE any stream capture begins: hipMalloc on a thread with
// an active capture fails with hipErrorStreamCaptureUnsupported and invalidates the capture (graph mode + repeated forwards).
void compat_prepare(lram_engine* e, int discrete) {
  if (e->B <= 0 || !compat_shares(e, discrete)) return;
  const size_t bt = (size_t)e->B * e->cfg.tokens_per_step;
  if (e->X0.n < bt * e->cfg.d_model) e->X0.alloc(bt * e->cfg.d_model);
  if (e->U0.n < bt * 2 * e->cfg.d_inner) e->U0.alloc(bt * 2 * e->cfg.d_inner);
}

void step_launches(lram_engine* e, Pass pass, const Inputs& in, const uint8_t* reset, int discrete, float* actions,
                   int32_t* tokens, hipStream_t s) {
  // compat_repeat (reference DiscreteDecisionMamba.get_action_pred, src/algos/decision_mamba.py:107-122): the same
  // (state, rtg, reward) tokens go through the stack once per action dim with the cache on, and action dim i is the
  // prediction of forward i.  Forward p writes action columns >= p, so column i keeps forward min(i, repeat - 1).
  pass.compat_passes = discrete ? 1 : std::max(1, std::min(e->compat_repeat, e->cfg.act_dim));
  pass.compat_shared = compat_shares(e, discrete);
  if (pass.compat_shared) {  // (allocated by compat_prepare ahead of this call: never inside a stream capture)
    const size_t bt = (size_t)e->n_live * e->cfg.tokens_per_step;   // (the rows of this call; compat_prepare allocates for the batch)
    LRAM_REQUIRE(e->X0.n >= bt * e->cfg.d_model && e->U0.n >= bt * 2 * e->cfg.d_inner,
                 "shared repeated forwards: workspace not prepared");
  }
  // every forward runs on the same slice streams: a slice's forward p + 1 follows its forward p in stream order (state, X0 / U0,
  // logits are per slice), so the slices are forked once and joined once instead of draining the two-slice pipeline per forward
  // (Mamba-48M at 2048 slots, 4 forwards per env-step, same box: 140.35k -> 141.0k env-steps/s)
  for (pass.compat_pass = 0; pass.compat_pass < pass.compat_passes; ++pass.compat_pass)
    timesteps_launches(e, pass, in, pass.compat_pass == 0 ? reset : nullptr, discrete, actions, tokens, s);
  sample_draw_advance(e, s);
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


// The refusals of the score entries for the sink they were handed (before anything is launched, the recurrent state untouched);
// `who` names the entry.
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
  LRAM_REQUIRE(discrete == 0 || discrete == 1 || discrete == LRAM_HEAD_PER_SLOT, w + ": discrete must be 0, 1 or LRAM_HEAD_PER_SLOT");
  LRAM_REQUIRE(discrete != LRAM_HEAD_PER_SLOT || e->slot_table, w + ": LRAM_HEAD_PER_SLOT needs a slot table (lram_set_slot_table)");
  LRAM_REQUIRE(discrete != 1 || e->cfg.n_discrete >= 1, w + ": a discrete head needs n_discrete >= 1");
  check_head_mask(e, discrete, w);
}

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

// The per-env lengths of a stored-context call (the ragged and append entries).  check(): everything that refuses the call for its
// lengths, before anything is launched or allocated.  run(): the plan and its device tables, then the chunks (`launch` runs
// timesteps_launches with the plan).  A call whose lengths all equal `timesteps` never gets to run(): it is the dense entry's.
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
  ContextPlan plan;   // (made by run())
  bool append = false;

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
    if (e->KEEP.n < need) {
      LRAM_HIP_CHECK(hipDeviceSynchronize());
      size_t free_b = 0, total_b = 0;
      LRAM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
      LRAM_REQUIRE(need * sizeof(float) + ((size_t)2 << 30) <= free_b + e->KEEP.n * sizeof(float),
                   w + ": the records of the " + std::to_string(kept.size()) + " slots of length 0 (" +
                       std::to_string(need * sizeof(float)) + " bytes) would leave less than 2 GiB of device memory free");
      e->KEEP.alloc(need);
    }
    plan.starts = context_plan(L, L > 1 ? prefill_chunk_steps(e, L) : 1, lengths, B, w.c_str());
    const int n_chunks = (int)plan.starts.size();
    // CTX: int32 start[B] | int32 chunk_start[L] | uint8 masks[L, B] | uint8 hold[L, B], as floats of one allocation
    const size_t want = (size_t)B + L + ((size_t)2 * L * B + 3) / 4;
    if (e->CTX.n < want) {
      LRAM_HIP_CHECK(hipDeviceSynchronize());
      e->CTX.alloc(want);
    }
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

// What the entries from frames refuse beyond the others (lram_prefill_frames / lram_score_frames), before anything is launched or
// allocated: no image encoder, a frame size that does not fit it, a geometry or mode without the state-embedding front end, state
// embeddings or flattened maps beyond 2 GiB.  (The entry itself has checked the slot table against dev_obs_seq.)
void check_frames_call(const lram_engine* e, const char* who, const Inputs& in, const int32_t* lengths) {
  const std::string w(who);
  const lram_config& c = e->cfg;
  LRAM_REQUIRE(in.img_c > 0 && in.img_h > 0 && in.img_w > 0, w + ": channels, height and width must be >= 1");
  check_frame_size(e, in.img_c, in.img_h, in.img_w, who);
  LRAM_REQUIRE(c.d_model % 4 == 0, w + ": stored contexts from frames need d_model to be a multiple of 4 (the chunk front end moves float4)");
  LRAM_REQUIRE(e->compat_repeat <= 1 && !e->compat_stale && !compat_shares(e, 0),
               w + ": a Mamba reference-trajectory mode is on (lram_set_compat_mode): its calls do not take their state "
                   "embeddings from one pass ahead of the chunks, which is where the frames are embedded");
  LRAM_REQUIRE((size_t)e->context_rows() * in.L * c.d_model <= ((size_t)1 << 29),
               w + ": the [batch, timesteps, d_model] state embeddings of the frames exceed 2 GiB");
  check_frame_list(e, count_frames(e, in.L, lengths).frames, who);
}

// What the six stored-context entries share, in this order: the refusals (the recurrent state is untouched by a refused call), the
// launches, the draw count.  `who` names the entry in every message.  rc: the per-env lengths of the ragged and append entries,
// null for the dense pair.  With a sink (the score entries) the head runs at every timestep and nothing is drawn; without one
// `actions` / `tokens` (nullable) take the action at every env's own last timestep.
void stored_context_call(lram_engine* e, const char* who, RaggedCall* rc, const Inputs& in, const uint8_t* reset, int discrete,
                         float* actions, int32_t* tokens, const ScoreSink* sink, hipStream_t s) {
  const std::string w(who);
  step_entry(e, who);
  require_all_live(e, who);
  LRAM_REQUIRE((in.obs || in.frames) && in.rtg && in.rew, w + ": null device pointer");
  LRAM_REQUIRE(in.L >= 1, w + ": timesteps must be >= 1");
  if (rc != nullptr) rc->check(in.emb);
  if (in.frames != nullptr) check_frames_call(e, who, in, rc ? rc->lengths : nullptr);
  if (sink != nullptr)
    check_score_sink(e, who, discrete, *sink);
  else if (actions != nullptr)
    check_head_mode(e, discrete, who);
  e->ctx_counts[0] += 1;
  Pass pass;
  pass.context = true;
  const int R = e->context_rows();
  if (rc == nullptr || rc->dense()) {   // every context of full length: the dense entry's own launches
    lazy_finish_prefold(e, s);          // (only an env-step takes a tail fold over)
    timesteps_launches(e, pass, in, reset, discrete, actions, tokens, s, sink);
  } else {
    rc->run(reset, s, [&](const ContextPlan& plan) {
      // the call-timesteps ahead of the first chunk are padding for every env: their rows of the sink take the fill values here
      // (per-chunk rows: an env is in no chunk ahead of its start, so the fill covers every call-timestep -- for env b the
      // kernel keeps to its padded rows [n_b, timesteps))
      if (sink != nullptr)
        launch_score_fill_ragged(sink->actions, sink->tokens, sink->logp, plan.dev_start, R, in.L,
                                 plan.rows.empty() ? plan.starts[0] : in.L, e->cfg.act_dim, s);
      timesteps_launches(e, pass, in, nullptr, discrete, actions, tokens, s, sink, &plan);
      if (sink == nullptr && actions != nullptr)   // slots without a context: 0 / -1 in place of the head's answer to the padding
        launch_action_fill_kept(actions, tokens, plan.dev_start, R, in.L, e->cfg.act_dim, s);
    });
  }
  // (a score is never a draw: the sampling mode and its counter are left alone)
  if (sink == nullptr && actions != nullptr) sample_draw_advance(e, s);
}
// The inputs of the entries from frames (lram_prefill_frames / lram_score_frames): the frames are a third source of the state
// embeddings (timesteps_launches); per-env lengths, where given, make it a ragged or an append call.
struct FramesCall {
  Inputs in;
  std::unique_ptr<RaggedCall> rc;
};
FramesCall frames_call(lram_engine* e, const char* who, const uint8_t* dev_frames, int32_t channels, int32_t height, int32_t width,
                       const float* dev_obs_seq, const float* dev_rtg_seq, const float* dev_reward_seq, int32_t timesteps,
                       const int32_t* host_lengths, int32_t append) {
  const std::string w(who);
  LRAM_REQUIRE(e != nullptr, w + ": null engine");
  LRAM_REQUIRE(dev_frames != nullptr, w + ": dev_frames is NULL");
  LRAM_REQUIRE(append == 0 || append == 1, w + ": append must be 0 (replace) or 1 (append)");
  // the vector slots of a mixed table hand in observations; nobody else's dev_obs_seq is ever read
  // (judged on the rows of the call: the image slots of the live prefix where lram_set_context_rows says so, as lram_step_slots)
  const int R = e->context_rows(), n_image = e->slot_table && R > 0 ? e->slot_img_prefix[R] : 0;
  const bool mixed = e->slot_table && n_image < R;
  LRAM_REQUIRE(!e->slot_table || n_image > 0, w + ": the slot table holds no image slot: there is no frame to take");
  LRAM_REQUIRE(!mixed || dev_obs_seq != nullptr, w + ": dev_obs_seq is NULL and the slot table holds vector slots");
  FramesCall fc;
  fc.in = Inputs{mixed ? dev_obs_seq : nullptr, 0, dev_rtg_seq, dev_reward_seq, timesteps};
  fc.in.frames = dev_frames, fc.in.img_c = channels, fc.in.img_h = height, fc.in.img_w = width;
  if (host_lengths != nullptr) fc.rc.reset(new RaggedCall{e, w, timesteps, host_lengths, {}, append != 0});
  return fc;
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

}  // namespace

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
    const Inputs in{dev_obs, obs_is_embedding, dev_rtg, dev_reward, 1};
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
          step_launches(e, Pass{}, in, dev_reset_mask, discrete, dev_actions, dev_tokens, cs);
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
      step_launches(e, Pass{}, in, dev_reset_mask, discrete, dev_actions, dev_tokens, s);
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
    step_launches(e, pass, Inputs{e->IMG_EMB.p, 1, dev_rtg, dev_reward, 1}, dev_reset_mask, discrete, dev_actions, dev_tokens,
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
    step_launches(e, pass, Inputs{dev_obs, 0, dev_rtg, dev_reward, 1}, dev_reset_mask, LRAM_HEAD_PER_SLOT, dev_actions, dev_tokens,
                  static_cast<hipStream_t>(stream));
  });
}

// The six stored-context entries: dense / ragged (replace) / append, each as prefill and as score -- one body (stored_context_call).
int32_t lram_prefill(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                     const float* dev_reward_seq, int32_t timesteps, const uint8_t* dev_reset_mask, int32_t discrete,
                     float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    stored_context_call(e, "lram_prefill", nullptr, Inputs{dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps},
                        dev_reset_mask, discrete, dev_actions, dev_tokens, nullptr, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_score(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                   const float* dev_reward_seq, int32_t timesteps, const uint8_t* dev_reset_mask, int32_t discrete,
                   const float* dev_target_actions, const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over,
                   double temperature, float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits, void* stream) {
  return guarded([&] {
    const ScoreSink sink{dev_actions, dev_tokens, dev_logp, dev_logits, dev_target_actions, dev_target_tokens, dev_valid, over, temperature};
    stored_context_call(e, "lram_score", nullptr, Inputs{dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps},
                        dev_reset_mask, discrete, nullptr, nullptr, &sink, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_prefill_ragged(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                            const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                            const uint8_t* dev_reset_mask, int32_t discrete, float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    RaggedCall rc{e, "lram_prefill_ragged", timesteps, host_lengths, {}, false};
    stored_context_call(e, rc.w.c_str(), &rc, Inputs{dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps},
                        dev_reset_mask, discrete, dev_actions, dev_tokens, nullptr, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_score_ragged(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                          const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                          const uint8_t* dev_reset_mask, int32_t discrete, const float* dev_target_actions,
                          const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over, double temperature,
                          float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits, void* stream) {
  return guarded([&] {
    RaggedCall rc{e, "lram_score_ragged", timesteps, host_lengths, {}, false};
    const ScoreSink sink{dev_actions, dev_tokens, dev_logp, dev_logits, dev_target_actions, dev_target_tokens, dev_valid, over, temperature};
    stored_context_call(e, rc.w.c_str(), &rc, Inputs{dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps},
                        dev_reset_mask, discrete, nullptr, nullptr, &sink, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_prefill_append(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                            const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                            const uint8_t* dev_reset_mask, int32_t discrete, float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_prefill_append: null engine");
    RaggedCall rc{e, "lram_prefill_append", timesteps, host_lengths, {}, true};
    stored_context_call(e, rc.w.c_str(), &rc, Inputs{dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps},
                        dev_reset_mask, discrete, dev_actions, dev_tokens, nullptr, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_score_append(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                          const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                          const uint8_t* dev_reset_mask, int32_t discrete, const float* dev_target_actions,
                          const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over, double temperature,
                          float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_score_append: null engine");
    RaggedCall rc{e, "lram_score_append", timesteps, host_lengths, {}, true};
    const ScoreSink sink{dev_actions, dev_tokens, dev_logp, dev_logits, dev_target_actions, dev_target_tokens, dev_valid, over, temperature};
    stored_context_call(e, rc.w.c_str(), &rc, Inputs{dev_obs_seq, obs_is_embedding, dev_rtg_seq, dev_reward_seq, timesteps},
                        dev_reset_mask, discrete, nullptr, nullptr, &sink, static_cast<hipStream_t>(stream));
  });
}

// Stored contexts from uint8 frames: the same body (frames_call above builds its inputs).
int32_t lram_prefill_frames(lram_engine* e, const uint8_t* dev_frames, int32_t channels, int32_t height, int32_t width,
                            const float* dev_obs_seq, const float* dev_rtg_seq, const float* dev_reward_seq, int32_t timesteps,
                            const int32_t* host_lengths, int32_t append, const uint8_t* dev_reset_mask, int32_t discrete,
                            float* dev_actions, int32_t* dev_tokens, void* stream) {
  return guarded([&] {
    FramesCall fc = frames_call(e, "lram_prefill_frames", dev_frames, channels, height, width, dev_obs_seq, dev_rtg_seq,
                                dev_reward_seq, timesteps, host_lengths, append);
    stored_context_call(e, "lram_prefill_frames", fc.rc.get(), fc.in, dev_reset_mask, discrete, dev_actions, dev_tokens, nullptr,
                        static_cast<hipStream_t>(stream));
  });
}

int32_t lram_score_frames(lram_engine* e, const uint8_t* dev_frames, int32_t channels, int32_t height, int32_t width,
                          const float* dev_obs_seq, const float* dev_rtg_seq, const float* dev_reward_seq, int32_t timesteps,
                          const int32_t* host_lengths, int32_t append, const uint8_t* dev_reset_mask, int32_t discrete,
                          const float* dev_target_actions, const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over,
                          double temperature, float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits,
                          void* stream) {
  return guarded([&] {
    FramesCall fc = frames_call(e, "lram_score_frames", dev_frames, channels, height, width, dev_obs_seq, dev_rtg_seq,
                                dev_reward_seq, timesteps, host_lengths, append);
    const ScoreSink sink{dev_actions, dev_tokens, dev_logp, dev_logits, dev_target_actions, dev_target_tokens, dev_valid, over, temperature};
    stored_context_call(e, "lram_score_frames", fc.rc.get(), fc.in, dev_reset_mask, discrete, nullptr, nullptr, &sink,
                        static_cast<hipStream_t>(stream));
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

int32_t lram_score_last(lram_engine* e, const int32_t* dev_tokens, int32_t over, double temperature, float* dev_logp,
                        void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_score_last: state not allocated (call lram_state_alloc)");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    prof_tick(e);
    LRAM_REQUIRE(dev_tokens && dev_logp, "lram_score_last: null device pointer");
    LRAM_REQUIRE(e->last_head >= 0, "lram_score_last: no action-producing call since lram_state_alloc: there are no logits to score");
    LRAM_REQUIRE(e->last_head != LRAM_HEAD_PER_SLOT || e->slot_table,
                 "lram_score_last: the last call was per-slot and the slot table has been cleared since");
    ScoreSink sink;
    sink.logp = dev_logp, sink.target_tokens = dev_tokens, sink.over = over, sink.temperature = temperature;
    check_head_mask(e, e->last_head, "lram_score_last");
    ScoreArgs a = score_args(e, sink, e->last_head);
    a.logits = e->LOGITS.p, a.ld = (int64_t)e->cfg.act_dim * e->cfg.n_vocab, a.rows = e->n_live;
    launch_action_score(a, static_cast<hipStream_t>(stream), head_mask(e));
  });
}

int32_t lram_score_last_sampled(lram_engine* e, const int32_t* dev_tokens, float* dev_logp, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr, "lram_score_last_sampled: null engine");
    LRAM_REQUIRE(e->B > 0, "lram_score_last_sampled: state not allocated (call lram_state_alloc)");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    prof_tick(e);
    LRAM_REQUIRE(dev_tokens && dev_logp, "lram_score_last_sampled: null device pointer");
    LRAM_REQUIRE(e->last_head >= 0,
                 "lram_score_last_sampled: no action-producing call since lram_state_alloc: there are no logits to score");
    LRAM_REQUIRE(e->sampling, "lram_score_last_sampled: sampling is not armed (lram_set_sampling): there is no drawn distribution");
    const int head = e->last_head;
    LRAM_REQUIRE(head != LRAM_HEAD_PER_SLOT || e->slot_table,
                 "lram_score_last_sampled: the last call was per-slot and the slot table has been cleared since");
    LRAM_REQUIRE(head != 1 || e->cfg.n_discrete >= 1, "lram_score_last_sampled: a discrete head needs n_discrete >= 1");
    check_sample_slots(e, head, "lram_score_last_sampled");
    LRAM_REQUIRE(!(head == LRAM_HEAD_PER_SLOT && e->sample_slots.empty() && e->slot_has_discrete &&
                   e->sample.top_k > e->cfg.n_discrete),
                 "lram_score_last_sampled: sampling top_k exceeds n_discrete and the slot table holds a discrete slot");
    check_head_mask(e, head, "lram_score_last_sampled");
    // (deterministic: no uniform is read, the draw counter is neither read nor advanced)
    launch_action_logp(e->LOGITS.p, dev_tokens, dev_logp, e->n_live, head_geom(e->cfg), head_slots(e, head), head, e->sample,
                       e->sample_slots_dev, static_cast<hipStream_t>(stream), head_mask(e));
  });
}

int32_t lram_sample_rows(const float* dev_logits, int64_t rows, int32_t n, int64_t ld, const uint8_t* dev_mode,
                         const double* dev_temperature, const int32_t* dev_top_k, const double* dev_top_p,
                         const double* dev_uniform, const int32_t* dev_tokens_in, int32_t* dev_tokens_out, float* dev_logp_out,
                         void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(dev_logits && dev_mode && dev_temperature && dev_top_k && dev_top_p, "lram_sample_rows: null device pointer");
    LRAM_REQUIRE((dev_uniform == nullptr) == (dev_tokens_out == nullptr), "lram_sample_rows: dev_uniform and dev_tokens_out go together");
    LRAM_REQUIRE((dev_tokens_in == nullptr) == (dev_logp_out == nullptr), "lram_sample_rows: dev_tokens_in and dev_logp_out go together");
    LRAM_REQUIRE(dev_tokens_out || dev_logp_out, "lram_sample_rows: neither a draw (dev_uniform, dev_tokens_out) nor a score "
                                                 "(dev_tokens_in, dev_logp_out) is asked for");
    LRAM_REQUIRE(ld == 0 || ld >= n, "lram_sample_rows: ld must be 0 (one shared row) or >= n");
    launch_sample_rows(dev_logits, rows, n, ld, dev_mode, dev_temperature, dev_top_k, dev_top_p, dev_uniform, dev_tokens_in,
                       dev_tokens_out, dev_logp_out, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_sample_rows_masked(const float* dev_logits, int64_t rows, int32_t n, int64_t ld, const uint8_t* dev_mode,
                                const double* dev_temperature, const int32_t* dev_top_k, const double* dev_top_p,
                                const double* dev_uniform, const int32_t* dev_tokens_in, int32_t* dev_tokens_out,
                                float* dev_logp_out, const uint32_t* dev_mask, int32_t words, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(dev_logits && dev_mode && dev_temperature && dev_top_k && dev_top_p && dev_mask,
                 "lram_sample_rows_masked: null device pointer");
    LRAM_REQUIRE((dev_uniform == nullptr) == (dev_tokens_out == nullptr),
                 "lram_sample_rows_masked: dev_uniform and dev_tokens_out go together");
    LRAM_REQUIRE((dev_tokens_in == nullptr) == (dev_logp_out == nullptr),
                 "lram_sample_rows_masked: dev_tokens_in and dev_logp_out go together");
    LRAM_REQUIRE(dev_tokens_out || dev_logp_out, "lram_sample_rows_masked: neither a draw nor a score is asked for");
    LRAM_REQUIRE(ld == 0 || ld >= n, "lram_sample_rows_masked: ld must be 0 (one shared row) or >= n");
    LRAM_REQUIRE(n >= 1 && words == (n + 31) / 32, "lram_sample_rows_masked: words must be ceil(n / 32)");
    launch_sample_rows(dev_logits, rows, n, ld, dev_mode, dev_temperature, dev_top_k, dev_top_p, dev_uniform, dev_tokens_in,
                       dev_tokens_out, dev_logp_out, static_cast<hipStream_t>(stream), HeadMask{dev_mask, words});
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

int32_t lram_embed_images(lram_engine* e, const uint8_t* dev_images, int32_t channels, int32_t height, int32_t width,
                          float* dev_embeddings, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_embed_images: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(dev_images && dev_embeddings && channels > 0 && height > 0 && width > 0, "lram_embed_images: bad argument");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    image_buffers(e, channels, height, width, "lram_embed_images");
    embed_images(e, dev_images, channels, height, width, dev_embeddings, static_cast<hipStream_t>(stream));
  });
}

int32_t lram_embed_frames(lram_engine* e, const uint8_t* dev_frames, int64_t n_frames, int32_t channels, int32_t height,
                          int32_t width, float* dev_embeddings, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_embed_frames: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(dev_frames && dev_embeddings && n_frames >= 1 && channels > 0 && height > 0 && width > 0,
                 "lram_embed_frames: bad argument");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    check_frame_size(e, channels, height, width, "lram_embed_frames");
    check_frame_list(e, n_frames, "lram_embed_frames");
    frame_list_buffers(e, channels, height, width, n_frames, "lram_embed_frames");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (the identity list: one "env" of n_frames timesteps)
    launch_frame_list(reinterpret_cast<int32_t*>(e->IMG_LIST.p), nullptr, nullptr, 1, (int)n_frames, s);
    embed_frame_list(e, dev_frames, height, width, n_frames, dev_embeddings, s);
  });
}

int32_t lram_image_counts(lram_engine* e, int64_t* out, int32_t reset) {
  return guarded([&] {
    LRAM_REQUIRE(e != nullptr && out != nullptr, "lram_image_counts: null argument");
    std::copy(e->img_counts, e->img_counts + 3, out);
    if (reset) std::fill(e->img_counts, e->img_counts + 3, (int64_t)0);
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
