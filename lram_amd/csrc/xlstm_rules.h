// The xLSTM token rules, once: what one token does to the mLSTM front-end scalars and to an sLSTM cell is the same in every
// kernel that applies it (xlstm_kernels.hip, mlstm_chunk.hip, mlstm_front.hip, slstm_seq.hip), so a state reaches the same
// bits whichever of them carried it there.  Values in, values out: no memory access, no LDS, no state, nothing of a kernel's
// layout or of the order in which it requests its operands.  The order of operations inside each rule is the oracle's
// (device_math.h); division by sqrt(DH) is a division, not a multiplication by a reciprocal.
//
// Reference functions replaced: conv1d_step + SiLU, LinearHeadwiseExpand q / k / v, mLSTMCell igate / fgate,
// recurrent_step_stabilized_simple's gate and normaliser part, [3P] slstm_pointwise.
#pragma once
#include "device_math.h"

namespace lram {

// ---- mLSTM token rules ----

// Depthwise 4-tap conv + SiLU on 4 adjacent channels: p0 .. p3 are the taps, oldest first; cw[c] holds channel c's 4 weights.
__device__ __forceinline__ float4 conv4_silu(const float4& p0, const float4& p1, const float4& p2, const float4& p3, const float4* cw,
                                             const float4& cb) {
  float4 y;
  y.x = p0.x * cw[0].x + p1.x * cw[0].y + p2.x * cw[0].z + p3.x * cw[0].w + cb.x;
  y.y = p0.y * cw[1].x + p1.y * cw[1].y + p2.y * cw[1].z + p3.y * cw[1].w + cb.y;
  y.z = p0.z * cw[2].x + p1.z * cw[2].y + p2.z * cw[2].z + p3.z * cw[2].w + cb.z;
  y.w = p0.w * cw[3].x + p1.w * cw[3].y + p2.w * cw[3].z + p3.w * cw[3].w + cb.w;
  return make_float4(silu_f(y.x), silu_f(y.y), silu_f(y.z), silu_f(y.w));
}

// One 4 x 4 block of the block-diagonal q / k / v projections: row o of the block is w[o].
__device__ __forceinline__ float4 block4x4(const float4* w, const float4& x) {
  return make_float4(dot4(w[0], x), dot4(w[1], x), dot4(w[2], x), dot4(w[3], x));
}

// A thread's 4-channel share of a gate pre-activation W . [q, k, v].
__device__ __forceinline__ float gate_partial(const float4& wq, const float4& wk, const float4& wv, const float4& q, const float4& k,
                                              const float4& v) {
  return dot4(wq, q) + dot4(wk, k) + dot4(wv, v);
}

// The stabilised gate step  lf = logsigmoid(f~); m' = max(lf + m, i~); f = exp(lf + m - m'); i = exp(i~ - m')  in the halves
// the chunk scan needs (it runs the m chain over the tokens first and exponentiates per lane afterwards); the step kernels'
// mlstm_gate_step is made of the same halves.
struct MlstmGate {
  float f, i, m;
};
__device__ __forceinline__ float mlstm_log_f(float gf) { return log_sigmoid(gf); }
__device__ __forceinline__ float mlstm_m_next(float lf, float m, float gi) { return fmaxf(lf + m, gi); }
__device__ __forceinline__ MlstmGate mlstm_gate_fi(float lf, float m, float mn, float gi) { return {expf(lf + m - mn), expf(gi - mn), mn}; }
__device__ __forceinline__ MlstmGate mlstm_gate_step(float gi, float gf, float m) {
  const float lf = mlstm_log_f(gf);
  return mlstm_gate_fi(lf, m, mlstm_m_next(lf, m, gi), gi);
}

// khat = k / sqrt(DH)
__device__ __forceinline__ float khat(float k, float sqrt_dh) { return k / sqrt_dh; }
__device__ __forceinline__ float4 khat(const float4& k, float sqrt_dh) {
  return make_float4(k.x / sqrt_dh, k.y / sqrt_dh, k.z / sqrt_dh, k.w / sqrt_dh);
}

// Normaliser state  n_t = f_t n_{t-1} + i_t khat_t.  (The statement stays as it is written: hipcc contracts the sum into one FMA,
// and with khat held in a temporary it takes f n for the addend in some kernels and i khat in others -- 1 ulp apart.)
__device__ __forceinline__ float4 mlstm_n_step(float4 n, float f, float i, const float4& k, float sqrt_dh) {
  n.x = f * n.x + i * khat(k.x, sqrt_dh);
  n.y = f * n.y + i * khat(k.y, sqrt_dh);
  n.z = f * n.z + i * khat(k.z, sqrt_dh);
  n.w = f * n.w + i * khat(k.w, sqrt_dh);
  return n;
}

// h_t's denominator from qn = q_t . n_t
__device__ __forceinline__ float mlstm_denominator(float qn, float m) { return fmaxf(fabsf(qn), expf(-m)) + 1e-6f; }

// ---- sLSTM cell rule ([3P] slstm_pointwise: per-element n == 0 first-step rule) ----
// One token of one (env, channel) cell from its four gate pre-activations: c, n, m are updated in place, the return value is
// y = h_t.
__device__ __forceinline__ float slstm_cell(float iraw, float fraw, float zraw, float oraw, float& c, float& n, float& m) {
  const float logfplusm = m + log_sigmoid(fraw);
  const float mnew = (n == 0.f) ? iraw : fmaxf(iraw, logfplusm);
  const float ogate = sigmoid_f(oraw);
  const float igate = fminf(expf(iraw - mnew), 1.f);
  const float fgate = fminf(expf(logfplusm - mnew), 1.f);
  const float cnew = fgate * c + igate * tanhf(zraw);
  const float nnew = fgate * n + igate;
  c = cnew, n = nnew, m = mnew;
  return ogate * cnew / nnew;
}

}  // namespace lram
