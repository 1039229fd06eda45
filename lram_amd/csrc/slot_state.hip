// Recurrent state of individual env slots on gfx950: copy slot -> slot (fork), swap slot <-> slot, save slots -> records, load
// records -> slots.
//
// The engine keeps every state tensor batch-major, one allocation per block and tensor; an env's state is therefore ~5 pieces
// per block scattered over as many allocations (16M: 9 MB in 8 blocks, 206M: 112 MB in 20).  The engine describes them once in
// a device-resident segment table (common.h: SlotSeg; one entry per contiguous per-env piece, the sLSTM [4, B, D] tensor is
// four) and a chunk table that cuts every piece into runs of kSlotChunk floats, so that ONE launch over
// (chunk, listed slot) moves every block and tensor: no per-tensor copy loops, no launch per block.
//
// Access shape: a lane moves 16 bytes, consecutive lanes consecutive 16-byte pieces (a wave instruction touches 1 KiB), four
// pieces in flight per lane, non-temporal loads and stores as the materialised cell kernel uses for C -- the data is touched
// once and must not evict the step's working set from L2.  Pieces whose per-env size, stride or record offset is not a multiple
// of 16 bytes (the stabiliser m with 1 or 2 heads, the count word) take a scalar path.
//
// Lazy matrix memory (mlstm_lazy.hip): a COPY moves the representation as it is -- C_base, the window rows, and the live
// ping-pong side of coefficients, scale and count word -- so the source is not folded and not written.  A SAVE computes
// C = g C_base + sum_j c_j khat_j v_j^T on the fly into the record (slot_lazy_save_kernel) and writes no engine state.  A LOAD
// writes C_base = C and marks the slot's window empty on the live side (count 0, zero bit clear, g = 1).
// A SWAP moves what a copy moves, both ways: two chunks loaded, then stored crosswise.
// The per-step score buffer `pw` of the lazy path is scratch (written and read inside one step) and is not moved.
#include "common.h"

namespace lram {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kPieces = kSlotChunk / (256 * 4);  // 16-byte pieces per lane and chunk

// `len` floats src -> dst by one workgroup of 256 lanes.  vec: both sides 16-byte aligned and len a multiple of 4.
__device__ __forceinline__ void move_chunk(const float* __restrict__ src, float* __restrict__ dst, int len, bool vec) {
  const int tid = threadIdx.x;
  if (vec) {
    const v4f* s4 = reinterpret_cast<const v4f*>(src);
    v4f* d4 = reinterpret_cast<v4f*>(dst);
    const int n4 = len >> 2;
    v4f v[kPieces];
#pragma unroll
    for (int u = 0; u < kPieces; ++u) {
      const int i = tid + 256 * u;
      if (i < n4) v[u] = __builtin_nontemporal_load(s4 + i);
    }
#pragma unroll
    for (int u = 0; u < kPieces; ++u) {
      const int i = tid + 256 * u;
      if (i < n4) __builtin_nontemporal_store(v[u], d4 + i);
    }
  } else {  // bit patterns, not values: the count word travels through here
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d1 = reinterpret_cast<uint32_t*>(dst);
    for (int i = tid; i < len; i += 256) d1[i] = s1[i];
  }
}

// a pointer every lane of the wave holds the same value of, moved to scalar registers
__device__ __forceinline__ float* uniform_ptr(float* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<float*>(((uint64_t)hi << 32) | lo);
}

// `len` floats at p <-> `len` floats at q by one workgroup of 256 lanes (p and q never overlap: the slots of a swap are distinct).
// Both chunks are loaded before either is stored: 2 x kPieces 16-byte pieces in flight per lane.
__device__ __forceinline__ void swap_chunk(float* __restrict__ p, float* __restrict__ q, int len, bool vec) {
  const int tid = threadIdx.x;
  if (vec) {
    // (both chunk bases are the same for every lane: held in scalar registers, a lane's address is base + one 32-bit offset --
    // eight 64-bit lane addresses would take the kernel past 64 VGPRs)
    v4f* p4 = reinterpret_cast<v4f*>(uniform_ptr(p));
    v4f* q4 = reinterpret_cast<v4f*>(uniform_ptr(q));
    const int n4 = len >> 2;
    if (n4 == kPieces * 256) {   // a whole chunk (all but a segment's last): no lane is idle, nothing is predicated
      v4f vp[kPieces], vq[kPieces];
#pragma unroll
      for (int u = 0; u < kPieces; ++u) vp[u] = __builtin_nontemporal_load(p4 + tid + 256 * u);
#pragma unroll
      for (int u = 0; u < kPieces; ++u) vq[u] = __builtin_nontemporal_load(q4 + tid + 256 * u);
#pragma unroll
      for (int u = 0; u < kPieces; ++u) __builtin_nontemporal_store(vq[u], p4 + tid + 256 * u);
#pragma unroll
      for (int u = 0; u < kPieces; ++u) __builtin_nontemporal_store(vp[u], q4 + tid + 256 * u);
    } else {                     // a segment's tail (i < n4 <= 1024: inside the chunk): piece by piece
      for (int i = tid; i < n4; i += 256) {
        const v4f x = __builtin_nontemporal_load(p4 + i), y = __builtin_nontemporal_load(q4 + i);
        __builtin_nontemporal_store(y, p4 + i), __builtin_nontemporal_store(x, q4 + i);
      }
    }
  } else {  // bit patterns, not values: the count word travels through here
    uint32_t* p1 = reinterpret_cast<uint32_t*>(p);
    uint32_t* q1 = reinterpret_cast<uint32_t*>(q);
    for (int i = tid; i < len; i += 256) {
      const uint32_t x = p1[i], y = q1[i];
      p1[i] = y, q1[i] = x;
    }
  }
}

__device__ __forceinline__ bool seg_live(const SlotSeg& sg, const SlotStateArgs& a) {
  if (sg.kind >= kSlotSegWindow && !a.lazy) return false;
  return sg.parity < 0 || sg.parity == a.parity;
}

}  // namespace

// grid (chunk, pair): slot dst[pair] <- slot src[pair], every live segment
__global__ __launch_bounds__(256) void slot_copy_kernel(SlotStateArgs a) {
  const SlotChunk ch = a.chunks[blockIdx.x];
  const SlotSeg sg = a.segs[ch.seg];
  if (!seg_live(sg, a)) return;
  const int64_t sb = a.src[blockIdx.y], db = a.dst[blockIdx.y];
  const int len = min(kSlotChunk, sg.numel - ch.off);
  move_chunk(sg.base + sb * sg.stride + ch.off, sg.base + db * sg.stride + ch.off, len, (sg.vec & 1) != 0);
}

// grid (chunk, pair): slot src[pair] <-> slot dst[pair], every live segment.  The host has checked that all 2n indices are
// distinct and in range, so no two workgroups touch the same floats.
__global__ __launch_bounds__(256) void slot_swap_kernel(SlotStateArgs a) {
  const SlotChunk ch = a.chunks[blockIdx.x];
  const SlotSeg sg = a.segs[ch.seg];
  if (!seg_live(sg, a)) return;
  const int64_t sb = a.src[blockIdx.y], db = a.dst[blockIdx.y];
  const int len = min(kSlotChunk, sg.numel - ch.off);
  swap_chunk(sg.base + sb * sg.stride + ch.off, sg.base + db * sg.stride + ch.off, len, (sg.vec & 1) != 0);
}

// grid (record chunk, listed slot): record[pair] <- slot src[pair]; in lazy mode C is left to slot_lazy_save_kernel
__global__ __launch_bounds__(256) void slot_save_kernel(SlotStateArgs a) {
  const SlotChunk ch = a.chunks[blockIdx.x];
  const SlotSeg sg = a.segs[ch.seg];
  if (sg.rec_off < 0 || (a.lazy && sg.kind == kSlotSegC)) return;
  const int64_t sb = a.src[blockIdx.y];
  const int len = min(kSlotChunk, sg.numel - ch.off);
  move_chunk(sg.base + sb * sg.stride + ch.off, a.records + (int64_t)blockIdx.y * a.rec_numel + sg.rec_off + ch.off, len,
             sg.vec == 3 && a.rec_vec != 0);
}

// grid (record chunk, listed slot): slot src[pair] <- record[pair]; lazy mode: workgroup 0 of every slot also empties the
// slot's window on the live ping-pong side (no other workgroup of a load touches the bookkeeping)
__global__ __launch_bounds__(256) void slot_load_kernel(SlotStateArgs a) {
  const SlotChunk ch = a.chunks[blockIdx.x];
  const SlotSeg sg = a.segs[ch.seg];
  const int64_t sb = a.src[blockIdx.y];
  if (a.lazy && blockIdx.x == 0) {
    for (int k = 0; k < a.n_segs; ++k) {
      const SlotSeg bk = a.segs[k];
      if (bk.parity != a.parity) continue;
      if (bk.kind == kSlotSegG)
        for (int i = threadIdx.x; i < bk.numel; i += 256) bk.base[sb * bk.stride + i] = 1.f;
      else if (bk.kind == kSlotSegCount && threadIdx.x == 0)
        *reinterpret_cast<int32_t*>(bk.base + sb * bk.stride) = 0;   // no pending tokens, zero bit clear
    }
  }
  if (sg.rec_off < 0) return;
  const int len = min(kSlotChunk, sg.numel - ch.off);
  move_chunk(a.records + (int64_t)blockIdx.y * a.rec_numel + sg.rec_off + ch.off, sg.base + sb * sg.stride + ch.off, len,
             sg.vec == 3 && a.rec_vec != 0);
}

// grid (segment, record): the sLSTM hidden planes of the listed records must lie inside (-limit, limit)
__global__ __launch_bounds__(256) void slot_y_range_kernel(SlotStateArgs a, float limit, int* flag) {
  const SlotSeg sg = a.segs[blockIdx.x];
  if (sg.kind != kSlotSegSlstmY) return;
  const float* y = a.records + (int64_t)blockIdx.y * a.rec_numel + sg.rec_off;
  bool bad = false;
  for (int i = threadIdx.x; i < sg.numel; i += 256) bad |= !(fabsf(y[i]) < limit);
  if (bad) atomicOr(flag, 1);
}

// Lazy save: one workgroup per (32 rows x 128 columns of C, head, listed slot).
//   record C[r][c] = g C_base[r][c] + sum_{j < n} (coef_j khat_j[r]) v_j[c]          (g = 0 under the zero bit: C_base is stale)
// The scaled khat tile and the v rows are staged in LDS; a lane owns 4 columns (16 bytes) of 4 rows, consecutive lanes
// consecutive columns.  Plain fp32 FMAs in window order: at most 48 terms per element, not a per-step path.
constexpr int kLsR = 32, kLsC = 128, kLsW = kLazyWindow;
__global__ __launch_bounds__(256) void slot_lazy_save_kernel(SlotLazySaveArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[kLsW * kLsR];
  __shared__ __attribute__((aligned(16))) float Vs[kLsW * kLsC];
  const int DH = a.DH, NH = a.NH;
  const int rtiles = DH / kLsR;
  const int row0 = (blockIdx.x % rtiles) * kLsR, col0 = (blockIdx.x / rtiles) * kLsC;
  const int h = blockIdx.y;
  const int64_t b = a.slots[blockIdx.z];
  const int tid = threadIdx.x;
  const int word = a.count[b];
  const int n = min(word & 0xFFFF, kLsW);
  const bool zero = (word & (1 << 16)) != 0;
  const int64_t bh = b * NH + h;
  const float g = a.g[bh];
  const float* wk = a.wk + bh * kLsW * DH + row0;
  const float* wv = a.wv + bh * kLsW * DH + col0;
  const float* coef = a.coef + bh * kLsW;
  for (int idx = tid; idx < n * (kLsR / 4); idx += 256) {
    const int j = idx / (kLsR / 4), r4 = (idx % (kLsR / 4)) * 4;
    const v4f k4 = *reinterpret_cast<const v4f*>(wk + (int64_t)j * DH + r4);
    *reinterpret_cast<v4f*>(Ks + j * kLsR + r4) = coef[j] * k4;
  }
  for (int idx = tid; idx < n * (kLsC / 4); idx += 256) {
    const int j = idx / (kLsC / 4), c4 = (idx % (kLsC / 4)) * 4;
    *reinterpret_cast<v4f*>(Vs + j * kLsC + c4) = *reinterpret_cast<const v4f*>(wv + (int64_t)j * DH + c4);
  }
  const int cg = tid & 31, rl = tid >> 5;
  const float* Cb = a.C + (bh * DH + row0) * DH + col0 + 4 * cg;
  v4f acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const v4f c = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(Cb + (int64_t)(rl + 8 * i) * DH));
    acc[i] = zero ? (v4f)(0.f) : g * c;
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const v4f v = *reinterpret_cast<const v4f*>(Vs + j * kLsC + 4 * cg);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float k = Ks[j * kLsR + rl + 8 * i];
      acc[i].x = fmaf(k, v.x, acc[i].x);
      acc[i].y = fmaf(k, v.y, acc[i].y);
      acc[i].z = fmaf(k, v.z, acc[i].z);
      acc[i].w = fmaf(k, v.w, acc[i].w);
    }
  }
  float* out = a.records + (int64_t)blockIdx.z * a.rec_numel + a.rec_off + ((int64_t)h * DH + row0) * DH + col0 + 4 * cg;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float* o = out + (int64_t)(rl + 8 * i) * DH;
    if (a.rec_vec) {
      __builtin_nontemporal_store(acc[i], reinterpret_cast<v4f*>(o));
    } else {
      o[0] = acc[i].x, o[1] = acc[i].y, o[2] = acc[i].z, o[3] = acc[i].w;
    }
  }
}

namespace {
dim3 slot_grid(int chunks, int n) { return dim3((unsigned)chunks, (unsigned)n); }
}  // namespace

void launch_slot_copy(const SlotStateArgs& a, hipStream_t stream) {
  if (a.n <= 0 || a.n_chunks <= 0) return;
  LRAM_REQUIRE(a.n <= 65535, "slot copy: at most 65535 pairs per call");
  hipLaunchKernelGGL(slot_copy_kernel, slot_grid(a.n_chunks, a.n), dim3(256), 0, stream, a);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_slot_swap(const SlotStateArgs& a, hipStream_t stream) {
  if (a.n <= 0 || a.n_chunks <= 0) return;
  LRAM_REQUIRE(a.n <= 65535, "slot swap: at most 65535 pairs per call");
  hipLaunchKernelGGL(slot_swap_kernel, slot_grid(a.n_chunks, a.n), dim3(256), 0, stream, a);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_slot_save(const SlotStateArgs& a, hipStream_t stream) {
  if (a.n <= 0 || a.n_chunks <= 0) return;
  LRAM_REQUIRE(a.n <= 65535, "slot save: at most 65535 slots per call");
  hipLaunchKernelGGL(slot_save_kernel, slot_grid(a.n_chunks, a.n), dim3(256), 0, stream, a);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_slot_load(const SlotStateArgs& a, hipStream_t stream) {
  if (a.n <= 0 || a.n_chunks <= 0) return;
  LRAM_REQUIRE(a.n <= 65535, "slot load: at most 65535 slots per call");
  hipLaunchKernelGGL(slot_load_kernel, slot_grid(a.n_chunks, a.n), dim3(256), 0, stream, a);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_slot_y_range(const SlotStateArgs& a, float limit, int* flag, hipStream_t stream) {
  if (a.n <= 0 || a.n_segs <= 0) return;
  hipLaunchKernelGGL(slot_y_range_kernel, dim3((unsigned)a.n_segs, (unsigned)a.n), dim3(256), 0, stream, a, limit, flag);
  LRAM_HIP_CHECK(hipGetLastError());
}

void launch_slot_lazy_save(const SlotLazySaveArgs& a, hipStream_t stream) {
  if (a.n <= 0) return;
  LRAM_REQUIRE(a.DH % kLsC == 0 && a.n <= 65535, "lazy slot save: head dim must be a multiple of 128");
  const unsigned tiles = (unsigned)((a.DH / kLsR) * (a.DH / kLsC));
  hipLaunchKernelGGL(slot_lazy_save_kernel, dim3(tiles, (unsigned)a.NH, (unsigned)a.n), dim3(256), 0, stream, a);
  LRAM_HIP_CHECK(hipGetLastError());
}

}  // namespace lram
