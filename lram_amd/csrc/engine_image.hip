// The IMPALA-CNN image front end and its buffers: the frames of an env-step (lram_step_images, lram_step_slots, lram_embed_images)
// and the frame list of a stored context (lram_prefill_frames, lram_score_frames, lram_embed_frames).
// Calls gemm.
#include "engine.h"

namespace {

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

// check_frame_size, then makes the image work buffers hold `frames` frames of H x W (an env-step: the batch; a frame list: the
// larger of the batch and its tile): every buffer by what it holds at this size, each grown on its own need (two sizes that feed
// the same linear layer can differ in which of them has the larger pooled map).  A region starts at a multiple of the per-frame
// size, so growing a buffer moves nobody's region.  Synchronises when it has to grow one: never called between a fork and a join.
void image_buffers(lram_engine* e, int C, int H, int W, const char* who, size_t frames) {
  check_frame_size(e, C, H, W, who);
  const ImageFrameFloats f = image_frame_floats(H, W);
  const size_t B = std::max((size_t)e->B, frames), np = B * f.p, nx = B * f.x;
  grow({{&e->IMG_P, np}, {&e->IMG_X0, nx}, {&e->IMG_X1, nx}, {&e->IMG_T, nx}});
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
                    int relu_out, const int32_t* frame_list) {
      Conv3x3Args a;
      a.in = src, a.w = c.w, a.bias = c.b, a.residual = res, a.out = dst, a.src = frame_list;
      a.B = B, a.CIN = c.cin, a.COUT = c.cout, a.H = h, a.W = w, a.in_relu = relu_in, a.out_relu = relu_out, a.in_u8 = u8;
      launch_conv3x3(a, s);
    };
    conv(cv[0], in, in_u8, 0, nullptr, P, 0, sidx == 0 ? list : nullptr);
    launch_maxpool3s2(P, X0, (int64_t)B * cv[0].cout, h, w, s);
    h = (h - 1) / 2 + 1, w = (w - 1) / 2 + 1;
    conv(cv[1], X0, 0, 1, nullptr, Tb, 0, nullptr);
    conv(cv[2], Tb, 0, 1, X0, X1, 0, nullptr);
    conv(cv[3], X1, 0, 1, nullptr, Tb, 0, nullptr);
    conv(cv[4], Tb, 0, 1, X1, sidx == 2 ? flat : X0, sidx == 2 ? 1 : 0, nullptr);  // act_flatten's ReLU on the last map
    in = X0;
    in_u8 = 0;
  }
  // stage s > 0 reads X0 and writes P, then pools back into X0: no aliasing within a launch
}

// ---- stored contexts from frames: the frame list -------------------------------------------------------------------------
// Frames per tile at this size: the knob, capped so that one tile's maps in the four work buffers stay within 2 GiB and the
// conv's grid within kConvMaxFrames.
int64_t frame_tile(const lram_engine* e, int H, int W) {
  const ImageFrameFloats f = image_frame_floats(H, W);
  const int64_t cap = std::max<int64_t>(1, (int64_t)(((size_t)1 << 29) / (f.p + 3 * f.x)));
  return std::min<int64_t>({(int64_t)e->img_tile, cap, (int64_t)kConvMaxFrames});
}

}  // namespace

namespace lram::host {

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

// The work buffers of an env-step's frames and the rows they are embedded into (lram_step_images, lram_step_slots)
void step_image_buffers(lram_engine* e, int C, int H, int W, const char* who) {
  image_buffers(e, C, H, W, who, 0);
  grow(e->IMG_EMB, (size_t)e->B * e->cfg.d_model);
}

// envs b0 .. b0 + nb - 1 of an env-step (`images` / `out` point at env b0's frame / row)
void embed_images(lram_engine* e, const uint8_t* images, int C, int H, int W, float* out, hipStream_t s, int b0, int nb) {
  const int D = e->cfg.d_model;
  // (image_buffers has checked C, H, W against the weights; the env slices of one call share its buffers)
  float* const X0 = e->IMG_X0.p + (size_t)b0 * image_frame_floats(H, W).x;
  cnn_stages(e, images, nullptr, H, W, nb, (size_t)b0, X0, s);
  GemmArgs g;
  g.a = X0, g.lda = e->img_flat, g.w = e->img_lin_w, g.ldw = e->img_flat, g.c = out, g.ldc = D;
  g.bias = e->img_lin_b, g.m = nb, g.n = D, g.k = e->img_flat;
  gemm(e, g, s);
  launch_relu(out, (int64_t)nb * D, s);
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
  grow({{&e->IMG_FLAT, (size_t)N * e->img_flat}, {&e->IMG_ROWS, (size_t)N * e->cfg.d_model}, {&e->IMG_LIST, (size_t)2 * N}});
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

}  // namespace lram::host

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int32_t lram_embed_images(lram_engine* e, const uint8_t* dev_images, int32_t channels, int32_t height, int32_t width,
                          float* dev_embeddings, void* stream) {
  return guarded([&] {
    LRAM_REQUIRE(e && e->B > 0, "lram_embed_images: state not allocated (call lram_state_alloc)");
    LRAM_REQUIRE(dev_images && dev_embeddings && channels > 0 && height > 0 && width > 0, "lram_embed_images: bad argument");
    LRAM_HIP_CHECK(hipSetDevice(e->device));
    image_buffers(e, channels, height, width, "lram_embed_images", 0);
    embed_images(e, dev_images, channels, height, width, dev_embeddings, static_cast<hipStream_t>(stream), 0, e->B);
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

}  // extern "C"
