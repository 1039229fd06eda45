// The Mamba stack of one pass: a block cut at its projections into three stages, and the staggered schedule of the env slices.
// Calls gemm and the streams.
#include "engine.h"

namespace {

// ---- Mamba block, cut at its projections ---------------------------------------------------------------
// stage 0: add + RMSNorm | in_proj      stage 1: conv | x_proj, dt_proj      stage 2: selective state update | out_proj
void mamba_stage(lram_engine* e, const Pass& pass, int i, int stage, int T, const uint8_t* reset, const Slice& sl) {
  const lram_config& c = e->cfg;
  const int D = c.d_model, di = c.d_inner, N = c.d_state, R = c.dt_rank, rows = sl.nb * T, ldx = R + 2 * N;
  const size_t r0 = (size_t)sl.b0 * T, b0 = sl.b0;
  const BlockWeights& w = e->bw[i];
  BlockState& st = e->st[i];
  float* X = e->X.p + r0 * D;
  float* RES = e->RES.p + r0 * D;
  float* XN = e->XN.p + r0 * D;
  // shared repeated forwards (step_launches): layer 0's residual input and in_proj output are the same in every pass
  const bool share = pass.compat_shared;
  if (share && i == 0 && stage == 0 && pass.compat_pass > 0) return;
  float* U = (share && i == 0) ? e->U0.p + r0 * 2 * di : e->U.p + r0 * 2 * di;
  float* RES_out = (share && i == 0) ? e->X0.p + r0 * D : RES;   // layer 0: RES = the embedded tokens, kept in X0
  const float* RES_in = i == 0 ? nullptr : ((share && i == 1) ? e->X0.p + r0 * D : RES);
  float* XA = e->XA.p + r0 * di;
  float* Q = e->Q.p + r0 * ldx;
  float* DTP = e->DTP.p + r0 * di;
  float* H = e->H.p + r0 * di;
  // compat_stale (reference InferenceParams.reset(), decision_mamba.py:20-25 + models/decision_mamba.py:130-149):
  // only layer 0 starts the episode from an empty state
  const uint8_t* rs = (reset && !(e->compat_stale && i > 0)) ? reset + b0 : nullptr;
  hipStream_t gs = sl.s;
  // f16x2 projections: the kernels that produce their operands hand the row maxima over -- the norm writes XN's (one
  // wave per row), the conv and the state-update kernels one partial maximum per wave (d_inner / 64 per row, plain
  // stores; the GEMM's prologue takes their maximum).  Atomic maxima were measured first: +20 us on the conv launch,
  // +13 us on the state update (147k single-lane atomics per launch), as much as the row-maximum launches they replaced.
  // dt_proj (K = dt_rank) inside the state-update kernel instead of a GEMM launch + its [rows, d_inner] round trip
  const bool dt_fused = e->mamba_dt_fuse && mamba_ssm_dt_fusable(N, R) && e->dt_wt[i].p != nullptr;
  const bool amx = e->use_f16x2 && di % 64 == 0 && N == 16 && T <= 4;
  const int parts = di / 64;
  float* amx_xn = amx ? e->AMX_XN.p + r0 : nullptr;
  float* amx_xa = amx ? e->AMX_XA.p + r0 * parts : nullptr;
  float* amx_h = amx ? e->AMX_H.p + r0 * parts : nullptr;
  // in_proj with both operands pre-split: the norm writes XN as two f16 planes + inverse row scales (see mlstm_front)
  const bool ps_in = amx && presplit_for(e, w.in_proj, rows, 2 * di, D);
  uint16_t* xn2 = reinterpret_cast<uint16_t*>(e->XN2.p) + r0 * 32;  // K-tile-major planes: [D / 32][B * T][32]
  const int64_t xn2_kt = ps_in ? (int64_t)(e->XN2.n / D) * 32 : 0;
  // x_proj's operand row maxima are not needed, and not written, where gemm() runs it in the exact-fp32 form of the narrow-output kernel
  const bool xp_narrow32 = stage == 1 && narrow32_for(e, w.x_proj, rows, ldx, di);
  if (stage == 0) {
    launch_add_rms_norm(X, RES_in, RES_out, ps_in ? nullptr : XN, w.norm_g, rows, D, c.norm_eps, sl.s, ps_in ? nullptr : amx_xn,
                        ps_in ? xn2 : nullptr, (int64_t)e->XN2.n, ps_in ? amx_xn : nullptr, xn2_kt);
  } else if (stage == 1) {
    MambaConvArgs ca;
    ca.xz = U, ca.conv_state = st.conv.p + b0 * di * c.d_conv, ca.conv_w = w.conv_w, ca.conv_b = w.conv_b, ca.xc = XA;
    ca.reset = rs, ca.B = sl.nb, ca.T = T, ca.d_inner = di, ca.K = c.d_conv, ca.amax = xp_narrow32 ? nullptr : amx_xa;
    ca.hold = pass.hold ? pass.hold + b0 : nullptr;   // (a stored-context chunk with a held env)
    launch_mamba_conv(ca, sl.s);
  } else {
    MambaSsmArgs sa;
    sa.ssm_state = st.s0.p + b0 * di * N, sa.xc = XA, sa.dtp = DTP, sa.dt_bias = w.dt_bias, sa.xdb = Q;
    sa.A_log = w.A_log, sa.Dp = w.Dp, sa.xz = U, sa.y = H, sa.reset = rs;
    sa.B = sl.nb, sa.T = T, sa.d_inner = di, sa.N = N, sa.R = R, sa.amax = amx_h;
    sa.hold = pass.hold ? pass.hold + b0 : nullptr;
    if (dt_fused) sa.dt_wt = e->dt_wt[i].p, sa.dtp = nullptr;
    prof_record(e, sl.s, true);
    launch_mamba_ssm(sa, sl.s);
    prof_record(e, sl.s, false);
  }
  if (stage == 0) {
    GemmArgs in;
    in.a = XN, in.lda = D, in.w = w.in_proj, in.ldw = D, in.c = U, in.ldc = 2 * di, in.bias = w.in_proj_b;
    in.m = rows, in.n = 2 * di, in.k = D, in.a_amax = amx_xn;
    if (ps_in) in.a = nullptr, in.a_amax = nullptr, in.a2 = xn2, in.a2_plane = (int64_t)e->XN2.n, in.a2_kt = xn2_kt, in.a2_inv = amx_xn;
    in.beside_memory_bound = (pass.n_slices > 1 || pass.lane_rec != nullptr) ? 1 : 0;   // (the other slice's conv / state update / norm run beside it)
    gemm(e, in, gs);
  } else if (stage == 1) {
    GemmArgs xp;
    xp.a = XA, xp.lda = di, xp.w = w.x_proj, xp.ldw = di, xp.c = Q, xp.ldc = ldx;
    xp.m = rows, xp.n = ldx, xp.k = di, xp.a_amax = xp_narrow32 ? nullptr : amx_xa, xp.amax_parts = amx ? parts : 1;
    gemm(e, xp, gs);
    if (!dt_fused && mamba_dt_proj_needs_plain_kernel(N, R)) {
      // (K = dt_rank or the row pitch dt_rank + 2 * d_state not a multiple of 4: the GEMM kernels' 16-byte operand loads do not apply)
      launch_mamba_dt_proj(Q, ldx, w.dt_proj, R, DTP, rows, di, gs);
    } else if (!dt_fused) {
      GemmArgs dp;
      dp.a = Q, dp.lda = ldx, dp.w = w.dt_proj, dp.ldw = R, dp.c = DTP, dp.ldc = di;
      dp.m = rows, dp.n = di, dp.k = R;
      gemm(e, dp, gs);
    }
  } else {
    GemmArgs op;
    op.a = H, op.lda = di, op.w = w.out_proj, op.ldw = di, op.c = X, op.ldc = D, op.bias = w.out_proj_b;
    op.m = rows, op.n = D, op.k = di, op.a_amax = amx_h, op.amax_parts = amx ? parts : 1;
    gemm(e, op, gs);
  }
}

}  // namespace

namespace lram::host {

// Mamba is projection-bound.  With two env slices on their own streams the memory-bound kernels
// of one slice (norm, conv, the selective state update) overlap the projections of the other; slice 1 is enqueued
// one stage behind slice 0 so the two do not start in lockstep.  No cross-stream events between fork and join:
// serialising the projections on a third stream costs more in event hand-offs than it gains (measured: 250k vs
// 298k single-stream vs 320k free-running env-steps/s at B = 2048, Mamba-48M).
void run_mamba_stack(lram_engine* e, const Pass& pass, int T, const uint8_t* reset, const std::vector<Slice>& sl) {
  const lram_config& c = e->cfg;
  const int D = c.d_model;
  const int n_stages = 3 * c.n_blocks;
  const int ns = (int)sl.size();
  for (int k = 0; k < n_stages + ns - 1; ++k)   // slice j is enqueued j stages behind slice 0
    for (int j = 0; j < ns; ++j)
      if (k - j >= 0 && k - j < n_stages) {
        const int layer = (k - j) / 3, stage = (k - j) % 3;
        // chunk lanes of lram_prefill (one slice): layer i of this chunk after layer i of the chunk before it (conv + SSM state)
        if (stage == 0 && pass.lane_wait) LRAM_HIP_CHECK(hipStreamWaitEvent(sl[j].s, (*pass.lane_wait)[layer], 0));
        mamba_stage(e, pass, layer, stage, T, reset, sl[j]);
        if (stage == 2 && pass.lane_rec) LRAM_HIP_CHECK(hipEventRecord((*pass.lane_rec)[layer], sl[j].s));
      }
  for (const Slice& x : sl) {
    const size_t r0 = (size_t)x.b0 * T;
    launch_add_rms_norm(e->X.p + r0 * D, e->RES.p + r0 * D, nullptr, e->HID.p + r0 * D, e->post_g, x.nb * T, D,
                        c.norm_eps, x.s);
  }
}

}  // namespace lram::host
