// IMPALA-CNN image front end for gfx950 (Atari / Procgen / vision observations).
//
// Replaces the reference's `embed_image` module (src/algos/models/image_encoders.py:10-131 ImpalaCNN, built at
// multi_domain_discrete_dt_model.py:43-46; the uint8 -> x/255 cast is online_decision_transformer_model.py:523-526):
//   3 x [ conv3x3(pad 1) -> maxpool(3, stride 2, pad 1) -> 2 x residual( x + conv(relu(conv(relu(x)))) ) ]
//   with 16 / 32 / 32 channels -> ReLU -> flatten (NCHW order) -> Linear -> ReLU.
// Activations are NCHW fp32 like the reference's; weights keep nn.Conv2d's [cout][cin][3][3] layout.
//
// conv3x3: one workgroup = one spatial tile of one image x all output channels.  The input tile (with its halo,
// zero padding, the optional ReLU / uint8 scaling applied while staging) sits in LDS; every thread owns one output
// pixel and a contiguous group of output channels in registers, so an input value read from LDS feeds CPT fused
// multiply-adds whose weight operand is wave-uniform (scalar loads).  Direct fp32 FMA arithmetic: ~65 MFLOP per
// image, i.e. ~33 GFLOP per env-step at 512 envs per GPU -- small beside the recurrent stack.
#include "common.h"
#include "device_math.h"

namespace lram {
namespace {

// TS x TS output pixels per workgroup, G = 256 / TS^2 channel groups, CPT output channels per thread.
// INDEXED (the first conv of a stored context's frame list): input frame k is a.src[2 * k] of the caller's frame tensor; the
// output stays compact.  Every other launch takes the instances without it.
template <int TS, int CPT, bool INDEXED>
__global__ __launch_bounds__(256) void conv3x3_kernel(Conv3x3Args a) {
  extern __shared__ float tile[];  // [CIN][TS + 2][TS + 3]
  constexpr int TP = TS + 3;       // padded row pitch
  constexpr int PIX = TS * TS;
  const int tid = threadIdx.x;
  const int H = a.H, W = a.W, CIN = a.CIN, COUT = a.COUT;
  const int tiles_x = (W + TS - 1) / TS;
  const int ty0 = (blockIdx.x / tiles_x) * TS, tx0 = (blockIdx.x % tiles_x) * TS;
  const int b = blockIdx.y;
  int b_in = b;
  if constexpr (INDEXED) b_in = a.src[2 * b];
  // ---- stage the input tile with a one-pixel halo ----
  const int halo = (TS + 2) * (TS + 2);
  for (int idx = tid; idx < CIN * halo; idx += 256) {
    const int ci = idx / halo, r = idx - ci * halo;
    const int yy = r / (TS + 2), xx = r - yy * (TS + 2);
    const int y = ty0 + yy - 1, x = tx0 + xx - 1;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const int64_t off = (((int64_t)b_in * CIN + ci) * H + y) * W + x;
      v = a.in_u8 ? (float)reinterpret_cast<const uint8_t*>(a.in)[off] / 255.0f
                  : reinterpret_cast<const float*>(a.in)[off];
      if (a.in_relu) v = fmaxf(v, 0.f);
    }
    tile[(ci * (TS + 2) + yy) * TP + xx] = v;
  }
  __syncthreads();
  const int pix = tid % PIX;
  const int g = __builtin_amdgcn_readfirstlane(tid / PIX);  // channel group: uniform within a wave (PIX >= 64)
  const int py = pix / TS, px = pix - py * TS;
  const int co0 = g * CPT;
  float acc[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) acc[c] = a.bias[co0 + c];
  for (int ci = 0; ci < CIN; ++ci) {
    float v[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) v[3 * ky + kx] = tile[(ci * (TS + 2) + py + ky) * TP + px + kx];
    const float* wp = a.w + ((int64_t)co0 * CIN + ci) * 9;
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const float* wc = wp + (int64_t)c * CIN * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[c] += v[t] * wc[t];
    }
  }
  const int y = ty0 + py, x = tx0 + px;
  if (y < H && x < W) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int64_t off = (((int64_t)b * COUT + co0 + c) * H + y) * W + x;
      float o = acc[c];
      if (a.residual != nullptr) o += a.residual[off];
      if (a.out_relu) o = fmaxf(o, 0.f);
      a.out[off] = o;
    }
  }
}

// nn.MaxPool2d(3, stride 2, padding 1): out[y][x] = max over in[2y-1 .. 2y+1][2x-1 .. 2x+1] (window clipped)
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* in, float* out, int64_t planes, int H, int W,
                                                         int Ho, int Wo) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= planes * Ho * Wo) return;
  const int x = (int)(gid % Wo), y = (int)((gid / Wo) % Ho);
  const int64_t p = gid / ((int64_t)Wo * Ho);
  const float* src = in + p * H * W;
  float m = -INFINITY;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = 2 * y + dy, xx = 2 * x + dx;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) m = fmaxf(m, src[(int64_t)yy * W + xx]);
    }
  out[gid] = m;
}

__global__ __launch_bounds__(256) void relu_kernel(float* x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = fmaxf(x[i], 0.f);
}

// The frame list of a stored context: one {src, dst} entry per frame that counts, env by env (blockIdx.y = k, the k-th env that
// hands in frames: slot slots[k], or k without a slot table), timestep by timestep.  src = k * L + l indexes the caller's frame
// tensor, dst = b * L + l the rows of the state embeddings.  Env b's context is its first L - start[b] timesteps (start: the
// call-timestep at which its end-aligned context begins; null: every context has all L), so the entries of the envs ahead of
// it number the sum of their lengths: every workgroup sums them for itself.
__global__ __launch_bounds__(256) void frame_list_kernel(int32_t* list, const int32_t* start, const int32_t* slots, int L) {
  __shared__ int part[256];
  const int k = blockIdx.y, tid = threadIdx.x;
  int before = k * L;
  if (start != nullptr) {   // (uniform over the launch)
    int sum = 0;
    for (int j = tid; j < k; j += 256) sum += L - start[slots != nullptr ? slots[j] : j];
    part[tid] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) part[tid] += part[tid + w];
      __syncthreads();
    }
    before = part[0];
  }
  const int b = slots != nullptr ? slots[k] : k;
  const int n = start != nullptr ? L - start[b] : L;
  const int l = blockIdx.x * 256 + tid;
  if (l < n) {
    list[2 * (before + l)] = k * L + l;
    list[2 * (before + l) + 1] = b * L + l;
  }
}

// act_linear's ReLU over the compact rows of the frame list's Linear, each placed at its row list[2 * i + 1] of `out`; V
// channels per thread (4: float4 moves)
template <int V>
__global__ __launch_bounds__(256) void relu_place_rows_kernel(const float* rows, const int32_t* list, float* out, int64_t N, int D) {
  const int dv = D / V;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= N * dv) return;
  const int64_t i = gid / dv;
  const int d = (int)(gid - i * dv) * V;
  const float* src = rows + i * D + d;
  float* dst = out + (int64_t)list[2 * i + 1] * D + d;
  if constexpr (V == 4) {
    const float4 v = *reinterpret_cast<const float4*>(src);
    *reinterpret_cast<float4*>(dst) = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
  } else {
    *dst = fmaxf(*src, 0.f);
  }
}

}  // namespace

void launch_conv3x3(const Conv3x3Args& a, hipStream_t stream) {
  LRAM_REQUIRE(a.B > 0 && a.CIN > 0 && a.H > 0 && a.W > 0, "conv3x3: empty problem");
  LRAM_REQUIRE(a.COUT == 16 || a.COUT == 32, "conv3x3: 16 or 32 output channels (IMPALA model_size 1)");
  // 32-channel maps of at most 16 x 16 pixels: 8 x 8 tiles with the output channels split over four waves give
  // four times the workgroups of a 16 x 16 tile (one image = one tile would leave half the chip idle at 512 envs)
  const bool small = a.COUT == 32 && a.H * a.W <= 256;
  const int TS = small ? 8 : 16;
  dim3 grid(((a.H + TS - 1) / TS) * ((a.W + TS - 1) / TS), a.B), block(256);
  const size_t shmem = sizeof(float) * (size_t)a.CIN * (TS + 2) * (TS + 3);
  LRAM_REQUIRE(shmem <= 64 * 1024, "conv3x3: too many input channels for the LDS tile");
  LRAM_REQUIRE(a.B <= kConvMaxFrames, "conv3x3: too many frames for one launch (the grid's y extent)");
  if (a.src != nullptr) {
    LRAM_REQUIRE(a.COUT == 16 && a.in_u8, "conv3x3: a frame list goes with the first conv of stage 1 only");
    hipLaunchKernelGGL((conv3x3_kernel<16, 16, true>), grid, block, shmem, stream, a);
  } else if (small)
    hipLaunchKernelGGL((conv3x3_kernel<8, 8, false>), grid, block, shmem, stream, a);
  else if (a.COUT == 16)
    hipLaunchKernelGGL((conv3x3_kernel<16, 16, false>), grid, block, shmem, stream, a);
  else
    hipLaunchKernelGGL((conv3x3_kernel<16, 32, false>), grid, block, shmem, stream, a);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_frame_list(int32_t* list, const int32_t* start, const int32_t* slots, int n_env, int L, hipStream_t stream) {
  LRAM_REQUIRE(list != nullptr && n_env >= 1 && n_env <= 65535 && L >= 1, "frame list: bad argument");
  hipLaunchKernelGGL(frame_list_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)n_env), dim3(256), 0, stream, list, start, slots, L);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_relu_place_rows(const float* rows, const int32_t* list, float* out, int64_t N, int D, hipStream_t stream) {
  LRAM_REQUIRE(rows && list && out && N >= 1 && D >= 1, "relu + place: bad argument");
  const bool vec = D % 4 == 0 && ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t n = N * (vec ? D / 4 : D);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (vec)
    hipLaunchKernelGGL((relu_place_rows_kernel<4>), grid, block, 0, stream, rows, list, out, N, D);
  else
    hipLaunchKernelGGL((relu_place_rows_kernel<1>), grid, block, 0, stream, rows, list, out, N, D);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_maxpool3s2(const float* in, float* out, int64_t planes, int H, int W, hipStream_t stream) {
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const int64_t n = planes * Ho * Wo;
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, out, planes, H, W,
                     Ho, Wo);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_relu(float* x, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(relu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, n);
  LRAM_HIP_CHECK(hipGetLastError());
}

}  // namespace lram
