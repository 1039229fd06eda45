// The xLSTM stack of one pass: mLSTM block (front end | state pass | back end), sLSTM block, the schedule of the lazy matrix
// memory's folds and read passes over the env slices, and the lazy representation's host side.  Calls gemm and the streams.
#include "engine.h"

namespace {

// ---- lazy matrix memory plumbing ------------------------------------------------------------------------
// step_off = 1: the arguments the NEXT step's launches get (the tail fold: its "in" side is the side this step's read passes write)
MlstmLazyArgs lazy_args(lram_engine* e, int i, int T, const uint8_t* reset, int b0, int nb, int step_off = 0) {
  const lram_config& c = e->cfg;
  const size_t NH = c.n_heads, DH = e->dh(), B = e->B;
  const int64_t step = e->lazy_step + step_off;
  const int in = (int)(step & 1), out = 1 - in;
  BlockState& st = e->st[i];
  MlstmLazyArgs a{};
  a.C = st.s0.p + (size_t)b0 * NH * DH * DH;
  a.wk = st.wk.p + (size_t)b0 * NH * kLazyWindow * DH;
  a.wv = st.wv.p + (size_t)b0 * NH * kLazyWindow * DH;
  a.coef_in = st.coef.p + (in * B + b0) * NH * kLazyWindow;
  a.coef_out = st.coef.p + (out * B + b0) * NH * kLazyWindow;
  a.g_in = st.gsc.p + (in * B + b0) * NH;
  a.g_out = st.gsc.p + (out * B + b0) * NH;
  a.count_in = reinterpret_cast<const int32_t*>(e->LZ_COUNT.p) + in * B + b0;
  a.count_out = reinterpret_cast<int32_t*>(e->LZ_COUNT.p) + out * B + b0;
  a.pw = st.pw.p ? st.pw.p + (size_t)b0 * NH * T * kLazyWT : nullptr;
  a.reset = reset ? reset + b0 : nullptr;
  a.B = nb, a.T = T, a.NH = (int)NH, a.DH = (int)DH;
  // the fold phase is taken relative to the env's global index, so slices fold the same envs as the whole batch
  a.phase = (int)((step + b0) % e->lazy_period), a.period = e->lazy_period, a.force = 0;
  return a;
}

// Would a step of T tokens taken at lazy_step == `step` use the compact fold grid (no class but the due one can overflow)?
bool lazy_bound_compact(const lram_engine* e, int64_t step, int T) {
  const int P = e->lazy_period;
  if ((int)e->lazy_bound.size() != P) return false;
  const int c_due = lazy_due_class(step, P);
  for (int cls = 0; cls < P; ++cls)
    if (cls != c_due && e->lazy_bound[cls] + T > kLazyWindow) return false;
  return true;
}

// The fold of one block over all env slots, for the step at lazy_step + step_off: the live range, then the parked range.  (A step's
// reset mask holds the live rows only: parked slots [n_live, B) fold in a launch of their own, without a mask -- a step never resets
// them -- so every class's fold still covers all its slots and the host-side bounds stay true.  The parked launch of a compact fold
// takes the compact grid view first, compact == 2 -- most parked windows are empty -- or is not launched at all.)
void fold_block(lram_engine* e, int i, int T, const uint8_t* reset, bool compact, int step_off, hipStream_t s) {
  MlstmLazyArgs la = lazy_args(e, i, T, reset, 0, e->n_live, step_off);
  la.compact = compact ? 1 : 0;
  prof_record(e, s, true, true);
  launch_mlstm_lazy_fold(la, s);
  if (e->n_live < e->B && !e->parked_windows_empty(e->lazy_step + step_off)) {
    MlstmLazyArgs lp = lazy_args(e, i, T, nullptr, e->n_live, e->B - e->n_live, step_off);
    lp.compact = compact ? 2 : 0;
    launch_mlstm_lazy_fold(lp, s);
  }
  prof_record(e, s, false, true);
}

}  // namespace

namespace lram::host {

// Fold every pending window into C_base and empty the bookkeeping: afterwards the state is the materialised
// reference layout again (export / import, prefill, long encoder calls, leaving lazy mode).
void lazy_materialize(lram_engine* e, hipStream_t s) {
  lazy_finish_prefold(e, s);
  if (!e->lazy_ready || !e->lazy_dirty) return;
  const lram_config& c = e->cfg;
  const size_t B = e->B, NH = c.n_heads;
  for (int i = 0; i < c.n_blocks; ++i) {
    if (c.block_is_slstm[i]) continue;
    MlstmLazyArgs a = lazy_args(e, i, 1, nullptr, 0, e->B);
    a.force = 1;
    launch_mlstm_lazy_fold(a, s);
  }
  for (int i = 0; i < c.n_blocks; ++i) {
    if (c.block_is_slstm[i]) continue;
    for (int p = 0; p < 2; ++p)
      launch_mlstm_lazy_clear(reinterpret_cast<int32_t*>(e->LZ_COUNT.p) + p * B, e->st[i].gsc.p + p * B * NH, nullptr,
                              (int)B, (int)NH, s);
  }
  e->lazy_bound.assign(e->lazy_period, 0);
  e->lazy_dirty = false;
}

// Completes a pending tail fold outside the step it was launched for: the due class's fold in the blocks the tail did not cover
// (compact grid, the phase of the step that would have come next), then the bookkeeping that fold step would have left -- for the
// envs of that class with pending tokens the shared count 0 with the zero bit cleared and g = 1 in every mLSTM block, on the
// side the next step reads.  LZ_COUNT is per env and shared by all blocks, so "block 0 is folded, the others are not" cannot be
// written into it; afterwards the state is what the normal schedule leaves behind that class's fold, and later steps find nothing
// pending there.  Called first thing by every entry that reads or edits the lazy representation and is not the matching step.
void lazy_finish_prefold(lram_engine* e, hipStream_t s) {
  if (!e->prefold.pending) return;
  const lram_engine::Prefold pf = e->prefold;
  e->prefold = lram_engine::Prefold{};
  LRAM_REQUIRE(e->lazy_ready && pf.B == e->B && pf.period == e->lazy_period && pf.step == e->lazy_step,
               "lazy mLSTM: a tail fold is pending for another state than the engine holds");
  const lram_config& c = e->cfg;
  const int B = e->B, NH = c.n_heads, P = e->lazy_period;
  const int side = (int)(e->lazy_step & 1);             // what the next step reads = what the last one wrote
  const int first = lazy_due_class(e->lazy_step, P);
  int k = 0;
  for (int i = 0; i < c.n_blocks; ++i) {
    if (c.block_is_slstm[i] || k++ < pf.blocks) continue;
    MlstmLazyArgs a = lazy_args(e, i, 1, nullptr, 0, B);
    a.compact = 1;
    launch_mlstm_lazy_fold(a, s);
  }
  int32_t* count = reinterpret_cast<int32_t*>(e->LZ_COUNT.p) + (size_t)side * B;
  for (int i = 0; i < c.n_blocks; ++i)
    if (!c.block_is_slstm[i]) launch_mlstm_lazy_folded(count, e->st[i].gsc.p + (size_t)side * B * NH, B, NH, first, P, s);
  launch_mlstm_lazy_folded(count, nullptr, B, NH, first, P, s);
  if ((int)e->lazy_bound.size() == P) e->lazy_bound[first] = 0;
}

}  // namespace lram::host

namespace {

// ---- mLSTM block, split at the cell kernel -----------------------------------------------------------
// proj_up in two halves pays from 2048 env slots (measured at 16M: 4096 slots 370k -> 374k env-steps/s, 1024 slots 292k
// -> 287k, 32 slots 45.4k -> 40.0k: below that the extra launch costs more than the shorter critical path gives)
// lean front end: the lazy read pass of the fused-score geometries rebuilds q, k, v itself (no q / k / v round trip through HBM)
bool lean_front(const lram_engine* e, int T) {
  return lazy_active(e, T) && mlstm_lazy_fused_scores(e->cfg.inner / e->cfg.n_heads);
}

bool split_up_now(const lram_engine* e) { return e->n_live >= 2048 && !e->graph_mode; }

// Output group norm + learnable skip inside the lazy read pass's epilogue (its workgroup holds a head's whole output
// row), silu(z) written by proj_up's epilogue and multiplied onto proj_down's operand while that GEMM stages it: no
// group-norm launch on the slice's chain, no [rows, inner] round trip for h.
// (Measured and removed, profiles/EXPERIMENTS.md: the output gate and proj_down's row maxima in that epilogue too -- the
// row-maximum launches and 0.7 GB of chain reads went, the step got 1.8 % SLOWER because the read pass, the critical queue,
// got 14 us longer; proj_down's row scales from a Cauchy-Schwarz bound instead of a row-maximum launch: -1.5 %; the gated
// operand pre-split by a row kernel: -0.5 %.)
bool gn_fused(const lram_engine* e, int T) {
  const int dh = e->cfg.inner / e->cfg.n_heads;
  return (e->gn_fuse == 1 || (e->gn_fuse == 2 && e->n_live >= 2048)) && lean_front(e, T) && e->use_bf16x3 && (dh == 256 || dh == 128) && T <= 4 &&
         e->cfg.inner % 8 == 0 && e->cfg.d_model % 8 == 0 && e->n_live >= 64;  // (fewer rows take the GEMV path)
}

void mlstm_front(lram_engine* e, const Pass& pass, int i, int T, const uint8_t* reset, const Slice& sl) {
  const lram_config& c = e->cfg;
  const int D = c.d_model, inner = c.inner, NH = c.n_heads, rows = sl.nb * T;
  const size_t r0 = (size_t)sl.b0 * T, b0 = sl.b0;
  const BlockWeights& w = e->bw[i];
  BlockState& st = e->st[i];
  float* amx = e->use_f16x2 ? e->AMX_XN.p + r0 : nullptr;  // the norm hands proj_up's operand row maxima over
  // proj_up in two halves: the x_m half feeds the conv / q / k / v front end and is on the block's critical path; the
  // z half is only needed by the output gate after the state pass and is issued beside it (mlstm_up_z)
  GemmArgs up;
  up.a = e->XN.p + r0 * D, up.lda = D, up.w = w.proj_up, up.ldw = D, up.c = e->U.p + r0 * e->ucols, up.ldc = 2 * inner;
  up.m = rows, up.n = split_up_now(e) ? inner : 2 * inner, up.k = D;
  if (gn_fused(e, T) && !split_up_now(e)) up.act_silu_from = inner;  // the z half is stored as silu(z)
  if (!split_up_now(e) && takes_skinny_with_norm(e, up)) {
    // few rows: the norm runs in the projection's prologue (each workgroup normalises its 32 rows in registers)
    up.a = e->X.p + r0 * D, up.norm_g = w.norm_g, up.norm_b = w.norm_b, up.norm_eps = c.ln_eps, up.norm_rms = c.norm_is_rms;
    launch_gemm_skinny(up, sl.s);
    count_gemm(e, 3, up);
  } else {
    // f16x2 with both operands pre-split: the norm writes the two operand planes (into XN's memory: 2 x 2 bytes per
    // element) and the rows' inverse scales (into AMX_XN) instead of fp32 + row maxima; both halves of proj_up read them
    const bool ps = presplit_for(e, w.proj_up, rows, inner, D);
    uint16_t* xn2 = reinterpret_cast<uint16_t*>(e->XN2.p) + r0 * 32;  // K-tile-major planes: [D / 32][B * T][32]
    const int64_t xn2_kt = ps ? (int64_t)(e->XN2.n / D) * 32 : 0;
    launch_row_norm(e->X.p + r0 * D, D, ps ? nullptr : e->XN.p + r0 * D, D, w.norm_g, w.norm_b, rows, D, c.ln_eps,
                    c.norm_is_rms, sl.s, nullptr, ps ? nullptr : amx, nullptr, ps ? xn2 : nullptr, (int64_t)e->XN2.n,
                    ps ? amx : nullptr, xn2_kt);
    up.a_amax = amx;
    if (ps) up.a = nullptr, up.a_amax = nullptr, up.a2 = xn2, up.a2_plane = (int64_t)e->XN2.n, up.a2_kt = xn2_kt, up.a2_inv = amx;
    if (pass.lane_rec != nullptr) up.beside_memory_bound = 2;   // a chunk lane of lram_prefill
    gemm(e, up, sl.s);
  }
  if (e->front_multi && lean_front(e, T) && sl.nb >= e->front_min_envs && e->gate_coef[i].p != nullptr &&
      mlstm_front_supported(inner, NH, c.conv_k, T)) {
    // large launches of the lean path: several env slots per workgroup, weights in registers (mlstm_front.hip)
    MlstmFrontArgs fa;
    fa.u = e->U.p + r0 * e->ucols, fa.ldu = 2 * inner, fa.conv_state = st.conv.p + b0 * c.conv_k * inner;
    fa.n_state = st.n.p + b0 * inner, fa.m_state = st.m.p + b0 * NH;
    fa.conv_w = w.conv_w, fa.conv_b = w.conv_b, fa.wq = w.wq, fa.wk = w.wk, fa.gc = e->gate_coef[i].p, fa.bi = w.bi, fa.bf = w.bf;
    fa.xa = e->XA.p + r0 * e->icols, fa.scal = e->SCAL.p + r0 * NH * 4, fa.reset = reset ? reset + b0 : nullptr;
    fa.B = sl.nb, fa.T = T, fa.inner = inner, fa.NH = NH, fa.K = c.conv_k, fa.epw = e->front_epw;
    // (the lean path belongs to the lazy read pass; stored contexts run materialised, so a held env never gets here)
    LRAM_REQUIRE(pass.hold == nullptr, "mLSTM front end: the multi-env kernel has no hold rule (stored contexts run materialised)");
    launch_mlstm_front(fa, sl.s);
    return;
  }
  MlstmPreArgs pa;
  pa.u = e->U.p + r0 * e->ucols, pa.conv_state = st.conv.p + b0 * c.conv_k * inner, pa.n_state = st.n.p + b0 * inner;
  pa.m_state = st.m.p + b0 * NH;
  pa.conv_w = w.conv_w, pa.conv_b = w.conv_b, pa.wq = w.wq, pa.wk = w.wk, pa.wv = w.wv;
  pa.wi = w.wi, pa.bi = w.bi, pa.wf = w.wf, pa.bf = w.bf;
  pa.q = e->Q.p + r0 * e->icols, pa.k = e->K.p + r0 * e->icols, pa.v = e->V.p + r0 * e->icols;
  pa.xa = e->XA.p + r0 * e->icols;
  pa.scal = e->SCAL.p + r0 * NH * 4, pa.reset = reset ? reset + b0 : nullptr;
  pa.hold = pass.hold ? pass.hold + b0 : nullptr;
  pa.B = sl.nb, pa.T = T, pa.inner = inner, pa.NH = NH, pa.K = c.conv_k;
  pa.lean = lean_front(e, T) ? 1 : 0;
  if (T > kMaxTokens) {
    LRAM_REQUIRE(T <= e->tok_cap && e->AMAT.p != nullptr, "chunkwise prefill workspace not allocated");
    pa.gates = e->GATES.p + r0 * NH * 2;
    pa.amat = e->AMAT.p + b0 * NH * kChunkMaxTokens * kChunkMaxTokens;
    pa.vec = e->VEC.p + b0 * NH * 3 * kChunkMaxTokens;
  }
  launch_mlstm_pre(pa, sl.s);
}

void mlstm_up_z(lram_engine* e, int i, int T, const Slice& sl) {
  if (!split_up_now(e)) return;
  const lram_config& c = e->cfg;
  const int D = c.d_model, inner = c.inner, rows = sl.nb * T;
  const size_t r0 = (size_t)sl.b0 * T;
  GemmArgs up;
  up.a = e->XN.p + r0 * D, up.lda = D, up.w = e->bw[i].proj_up + (size_t)inner * D, up.ldw = D;
  up.c = e->U.p + r0 * e->ucols + inner, up.ldc = 2 * inner, up.m = rows, up.n = inner, up.k = D;
  if (e->use_f16x2) up.a_amax = e->AMX_XN.p + r0;  // written by this block's norm launch (mlstm_front)
  if (presplit_for(e, e->bw[i].proj_up, rows, inner, D)) {  // (same decision as mlstm_front: XN2 holds operand planes)
    up.a = nullptr, up.a_amax = nullptr;
    up.a2 = reinterpret_cast<uint16_t*>(e->XN2.p) + r0 * 32, up.a2_plane = (int64_t)e->XN2.n, up.a2_kt = (int64_t)(e->XN2.n / D) * 32;
    up.a2_inv = e->AMX_XN.p + r0;
  }
  if (gn_fused(e, T)) up.act_silu_from = 0;
  up.beside_memory_bound = e->upz_beside ? 1 : 0;   // (issued beside this slice's own state pass)
  gemm(e, up, sl.s);
}

void mlstm_cell(lram_engine* e, const Pass& pass, int i, int T, const uint8_t* reset, const Slice& sl, hipStream_t s) {
  const lram_config& c = e->cfg;
  const int inner = c.inner, NH = c.n_heads, DH = e->dh();
  const size_t r0 = (size_t)sl.b0 * T, b0 = sl.b0;
  MlstmCellArgs ca;
  ca.C = e->st[i].s0.p + b0 * NH * DH * DH, ca.q = e->Q.p + r0 * e->icols, ca.k = e->K.p + r0 * e->icols;
  ca.v = e->V.p + r0 * e->icols, ca.scal = e->SCAL.p + r0 * NH * 4, ca.h = e->H.p + r0 * e->icols;
  ca.reset = reset ? reset + b0 : nullptr, ca.B = sl.nb, ca.T = T, ca.NH = NH, ca.DH = DH;
  ca.hold = pass.hold ? pass.hold + b0 : nullptr;
  // Large launches: one cell workgroup per CU (84 KB of LDS each; a second one does not fit, two 37 KB GEMM
  // workgroups of the other slice do).  Measured on MI355X at B=4096/16M: 1.61 ms -> 1.47 ms per launch
  // (5.5 -> 6.0 TB/s) standalone; see DESIGN.md section 6.
  const long wgs = (long)sl.nb * NH * ((DH % 256 == 0) ? DH / 256 : (DH % 128 == 0) ? DH / 128 : DH / 64);
  ca.min_lds_bytes = wgs >= 1024 ? 84 * 1024 : 0;
  ca.unroll = e->cell_unroll;
  if (T > kMaxTokens) {
    ca.amat = e->AMAT.p + b0 * NH * kChunkMaxTokens * kChunkMaxTokens;
    ca.vec = e->VEC.p + b0 * NH * 3 * kChunkMaxTokens;
    ca.chunk_exact_fp32 = e->chunk_exact_fp32 ? 1 : 0;
  }
  prof_record(e, s, true);
  launch_mlstm_cell(ca, s);
  prof_record(e, s, false);
}

void mlstm_back(lram_engine* e, const Pass& pass, int i, int T, const Slice& sl) {
  const lram_config& c = e->cfg;
  const int D = c.d_model, inner = c.inner, NH = c.n_heads, DH = e->dh(), rows = sl.nb * T;
  const size_t r0 = (size_t)sl.b0 * T;
  const BlockWeights& w = e->bw[i];
  float* X = e->X.p + r0 * D;
  if (gn_fused(e, T)) {  // H holds GN(h) + skip * xa, U's z half silu(z)
    GemmArgs dn;
    dn.a = e->H.p + r0 * e->icols, dn.lda = inner, dn.w = w.proj_down, dn.ldw = inner, dn.c = X, dn.ldc = D, dn.residual = X;
    dn.m = rows, dn.n = D, dn.k = inner;
    dn.gate = e->U.p + r0 * e->ucols + inner, dn.ldg = 2 * inner;
    gemm(e, dn, sl.s);
    return;
  }
  GroupNormArgs ga;
  ga.h = e->H.p + r0 * e->icols, ga.gamma = w.on_g, ga.beta = w.on_b, ga.skip = w.skip, ga.xa = e->XA.p + r0 * e->icols;
  ga.u = e->U.p + r0 * e->ucols, ga.out = e->G.p + r0 * e->icols, ga.rows = rows, ga.NH = NH, ga.DH = DH, ga.mode = 0;
  ga.eps = c.ln_eps;
  // the norm's waves (one per row and head) hand proj_down's operand row maxima over as NH partial maxima per row: the
  // row_amax launch between the two (8-11 us on every block of a chain-bound slice's chain) goes
  // (LRAM_GN_AMAX=0, test switch: the standalone row-maximum launch instead; bit-identical by construction -- a maximum of
  // partial maxima is exact -- and tests/test_gpu_realbatch.py holds it to that)
  const bool hand_over = e->gn_amax_handover && e->AMX_H.p != nullptr && f16x2_rows(e, rows, D, inner);
  GemmArgs dn;
  dn.a = e->G.p + r0 * e->icols, dn.lda = inner, dn.w = w.proj_down, dn.ldw = inner, dn.c = X, dn.ldc = D, dn.residual = X;
  dn.m = rows, dn.n = D, dn.k = inner;
  // ... or (round 6; one env slice: stored contexts, small and mid-size batches) the norm writes proj_down's operand itself: the two
  // f16 planes of the row scaled by its maximum over all heads -- the same 4 bytes per element as the fp32 row, into G's memory --
  // and the projection runs on the pre-split kernel (LDS-DMA staging, no conversion in its loop: 15-28 % faster on every
  // down-projection shape alone, profiles/r06_gemm_durations.txt).  Bit-identical to the hand-over path.  Same box, hand-over vs
  // planes: C5's prefill 297.9 -> 292.0 ms, 206M at 64 envs 14.98k -> 15.18k env-steps/s; NOT inside the two-slice pipelines, where
  // the pre-split kernel's 48 KB workgroups wait for the other slice's read pass to leave a CU: 16M at 1024 slots 378.6k -> 368.8k,
  // 206M at 512 slots +-0.
  const int64_t bt = (int64_t)(e->G.n / e->icols);   // rows the workspace holds
  GemmArgs probe;
  const bool planes = hand_over && e->gn_planes && pass.n_slices == 1 && e->gemm_presplit && NH <= 8 && (inner & 31) == 0 && bt * inner * 4 < (1ll << 31) &&
                      f16x2_weight(e, w.proj_down, inner, &probe) && 4 * probe.w2_plane < (1ll << 31);
  if (planes) {
    ga.out = nullptr;
    ga.h2 = reinterpret_cast<uint16_t*>(e->G.p) + r0 * 32, ga.h2_plane = bt * inner, ga.h2_kt = bt * 32, ga.h2_inv = e->AMX_H.p + r0;
    dn.a = nullptr, dn.a2 = ga.h2, dn.a2_plane = ga.h2_plane, dn.a2_kt = ga.h2_kt, dn.a2_inv = ga.h2_inv;
  } else {
    ga.amax = hand_over ? e->AMX_H.p + r0 * NH : nullptr;
    if (hand_over) dn.a_amax = ga.amax, dn.amax_parts = NH;
  }
  launch_group_norm(ga, sl.s);
  gemm(e, dn, sl.s);
}

// Fills g4's operand tables for the four sLSTM gate projections as one bf16x3 launch; false where that kernel cannot serve it.
bool slstm_gates_one_bf16x3(const lram_engine* e, GemmArgs& g4, const BlockWeights& w, const float* XC, const float* XN, float* gates,
                            int Hs) {
  if (!e->use_bf16x3 || !e->slstm_gates_one) return false;
  int64_t plane = -1;
  for (int g = 0; g < 4; ++g) {
    auto it = e->split.find(w.gate_w[g]);
    if (it == e->split.end() || (plane >= 0 && (int64_t)it->second.n != plane)) return false;
    plane = (int64_t)it->second.n;
    g4.a_tab[g] = (g < 2) ? XC : XN, g4.w_tab[g] = w.gate_w[g], g4.c_tab[g] = gates + (int64_t)g * Hs;
    g4.w3_tab[g] = it->second.p;
  }
  g4.w3 = g4.w3_tab[0], g4.w3_plane = plane;
  return gemm_bf16x3_supported(g4) && !gemm_small_m(g4);
}

void slstm_block(lram_engine* e, const Pass& pass, int i, int T, const uint8_t* reset, const Slice& sl) {
  const lram_config& c = e->cfg;
  const int D = c.d_model, NH = c.n_heads, SDH = e->sdh(), F = c.ffn_dim, Hs = D, rows = sl.nb * T;
  const size_t r0 = (size_t)sl.b0 * T, b0 = sl.b0;
  const BlockWeights& w = e->bw[i];
  BlockState& st = e->st[i];
  hipStream_t s = sl.s;
  float* X = e->X.p + r0 * D;
  float* XN = e->XN.p + r0 * D;
  float* XC = e->Q.p + r0 * e->icols;          // silu(conv(xn))
  float* gates = e->U.p + r0 * e->ucols;  // [rows, 4, H]
  float* RY = e->RY.p + b0 * 4 * Hs;     // [nb, 4, H]
  float* Y = e->H.p + r0 * e->icols;          // [rows, H]
  float* Ubuf = e->U.p + r0 * e->ucols;
  float* Gbuf = e->G.p + r0 * e->icols;
  float* state = st.s0.p + b0 * Hs;      // [4, B, H] viewed from env b0 (leading-axis stride e->B * H)
  const uint8_t* hold = pass.hold ? pass.hold + b0 : nullptr;   // (a stored-context chunk with a held env)
  launch_row_norm(X, D, XN, D, w.norm_g, w.norm_b, rows, D, c.ln_eps, c.norm_is_rms, s);
  SlstmConvArgs sa;
  sa.xn = XN, sa.conv_state = st.conv.p + b0 * c.conv_k * D, sa.slstm_state = state, sa.conv_w = w.conv_w;
  sa.conv_b = w.conv_b, sa.xc = XC, sa.reset = reset ? reset + b0 : nullptr, sa.B = sl.nb, sa.T = T, sa.D = D;
  sa.K = c.conv_k, sa.state_B = e->B, sa.hold = hold;
  launch_slstm_conv(sa, s);
  GemmArgs g4;  // few rows: the four gate projections (per-head blocks, i / f on the conv branch, z / o on the norm) as ONE launch
  g4.a = XC, g4.lda = D, g4.sA1 = SDH, g4.w = w.gate_w[0], g4.ldw = SDH, g4.sW1 = (int64_t)SDH * SDH;
  g4.c = gates, g4.ldc = 4 * Hs, g4.sC1 = SDH, g4.m = rows, g4.n = SDH, g4.k = SDH, g4.nb1 = NH, g4.nb2 = 4;
  // (head dim <= 128: up to 768 rows as well -- 16M at 256 envs +2.6 %; at 6144 rows -1.5 %, 206M's 320-wide heads at 768 rows -1 %)
  const bool gates_big = rows <= e->slstm_gates_rows && gemm_skinny_supported(g4) && g4.k <= 128;
  // (every table entry must meet the few-row kernel's 16-byte alignment, not only entry 0 that g4.a / g4.w stand for: a
  // misaligned later entry falls back to the four separate launches instead of failing inside launch_gemm_skinny)
  bool tab_aligned = true;
  for (int g = 0; g < 4; ++g)
    tab_aligned = tab_aligned && ((reinterpret_cast<uintptr_t>((g < 2) ? XC : XN) | reinterpret_cast<uintptr_t>(w.gate_w[g])) & 15) == 0;
  if (tab_aligned && (takes_skinny(e, g4) || gates_big)) {
    for (int g = 0; g < 4; ++g)
      g4.a_tab[g] = (g < 2) ? XC : XN, g4.w_tab[g] = w.gate_w[g], g4.c_tab[g] = gates + (int64_t)g * Hs;
    launch_gemm_skinny(g4, s);
    count_gemm(e, 3, g4);
  } else if (slstm_gates_one_bf16x3(e, g4, w, XC, XN, gates, Hs)) {
    // larger slices: the same ONE launch on the bf16x3 kernel (operand tables; every gate's tiles in one grid instead of four
    // short launches of 48-144 workgroups each on the slice's chain) -- bit-identical to the four launches
    g4.knobs = e->gemm_knobs;   // (a tile launcher without gemm())
    launch_gemm_bf16x3(g4, s);
    count_gemm(e, 1, g4);
  } else {
    for (int g = 0; g < 4; ++g) {
      GemmArgs ga;
      ga.a = (g < 2) ? XC : XN, ga.lda = D, ga.sA1 = SDH;
      ga.w = w.gate_w[g], ga.ldw = SDH, ga.sW1 = (int64_t)SDH * SDH;
      ga.c = gates + (int64_t)g * Hs, ga.ldc = 4 * Hs, ga.sC1 = SDH;
      ga.m = rows, ga.n = SDH, ga.k = SDH, ga.nb1 = NH;
      gemm(e, ga, s);
    }
  }
  // few env rows (up to slstm_fused_rows): recurrent projection + pointwise cell as ONE lean launch per token instead of a
  // batched matrix-core GEMM (fixed latency of a 128-row tile) and the pointwise kernel
  // (measured, same box each: 16M 1 env +1.9 %, 8 +4.2 %, 12 +6.6 %, 32 +6.0 %, 128 +3.3 %, 512-env slices +1.6 %, 1024-env
  // slices +-0; 206M 16 envs +6.1 %, 64 +2.9 %, 256-env slices -1.4 %: the row limit scales with 128 / head dim)
  const bool tok_fused = e->slstm_fused_rows > 0 &&
                         (int64_t)sl.nb * std::max(SDH, 128) <= (int64_t)e->slstm_fused_rows * 128 && slstm_token_supported(Hs, NH);
  for (int t = 0; tok_fused && t < T; ++t) {
    SlstmTokenArgs ta;
    ta.gates = gates, ta.rt = w.rt, ta.bias = w.rbias, ta.state = state, ta.yout = Y;
    ta.hprev = t == 0 ? state : Y + (int64_t)(t - 1) * Hs, ta.hprev_ld = t == 0 ? Hs : (int64_t)T * Hs;
    ta.B = sl.nb, ta.T = T, ta.t = t, ta.H = Hs, ta.NH = NH, ta.state_B = e->B, ta.write_h = (t == T - 1 && t > 0) ? 1 : 0;
    ta.hold = hold;
    launch_slstm_token(ta, s);
    ++e->slstm_counts[0];
  }
  // (a one-token pass copies the h plane of every env: a stored-context chunk, the only pass with held envs, holds whole timesteps)
  LRAM_REQUIRE(hold == nullptr || T >= 3, "sLSTM block: held envs need whole timesteps of three tokens");
  if (tok_fused && T == 1)  // the single launch read the state's h plane: it is refreshed from the output rows afterwards
    LRAM_HIP_CHECK(hipMemcpyAsync(state, Y, (size_t)sl.nb * Hs * sizeof(float), hipMemcpyDeviceToDevice, s));
  // slices beyond the token kernel's: the whole step's recurrence as ONE launch (head dim 128; slstm_seq.hip)
  const bool seq = !tok_fused && e->slstm_seq && e->slstm_rt2[i].p != nullptr && slstm_seq_supported(Hs, NH, T);
  if (seq) {
    SlstmSeqArgs qa;
    qa.gates = gates, qa.bias = w.rbias, qa.state = state, qa.yout = Y;
    if (e->slstm_rinv[i].p != nullptr)
      qa.rt2h = reinterpret_cast<const uint16_t*>(e->slstm_rt2[i].p), qa.rinv = e->slstm_rinv[i].p;
    else
      qa.rt2 = e->slstm_rt2[i].p;
    qa.B = sl.nb, qa.T = T, qa.H = Hs, qa.NH = NH, qa.state_B = e->B, qa.hold = hold;
    launch_slstm_seq(qa, s);
    ++e->slstm_counts[1];
  }
  for (int t = 0; !tok_fused && !seq && t < T; ++t) {
    GemmArgs ra;
    ra.a = state, ra.lda = Hs, ra.sA1 = SDH, ra.sA2 = 0;
    ra.w = w.rt, ra.ldw = SDH, ra.sW1 = 4 * (int64_t)SDH * SDH, ra.sW2 = (int64_t)SDH * SDH;
    ra.c = RY, ra.ldc = 4 * Hs, ra.sC1 = SDH, ra.sC2 = Hs;
    ra.m = sl.nb, ra.n = SDH, ra.k = SDH, ra.nb1 = NH, ra.nb2 = 4;
    gemm(e, ra, s);
    SlstmPointwiseArgs pw;
    pw.gates = gates, pw.ry = RY, pw.bias = w.rbias, pw.state = state, pw.yout = Y;
    pw.B = sl.nb, pw.T = T, pw.t = t, pw.H = Hs, pw.state_B = e->B, pw.hold = hold;
    launch_slstm_pointwise(pw, s);
    ++e->slstm_counts[2];
  }
  GroupNormArgs gn;
  gn.h = Y, gn.gamma = w.gn_g, gn.beta = w.gn_b, gn.out = X, gn.rows = rows, gn.NH = NH, gn.DH = SDH;
  gn.mode = 1, gn.eps = c.ln_eps, gn.skip = nullptr, gn.xa = nullptr, gn.u = nullptr;
  launch_group_norm(gn, s);
  float* amx = e->use_f16x2 ? e->AMX_XN.p + r0 : nullptr;
  GemmArgs up;
  up.a = XN, up.lda = D, up.w = w.ffn_up, up.ldw = D, up.c = Ubuf, up.ldc = 2 * F;
  up.m = rows, up.n = 2 * F, up.k = D;
  if (takes_skinny_with_norm(e, up)) {  // few rows: the FFN's norm inside the projection's prologue
    up.a = X, up.norm_g = w.ffn_norm_g, up.norm_b = w.ffn_norm_b, up.norm_eps = c.ln_eps, up.norm_rms = c.norm_is_rms;
    launch_gemm_skinny(up, s);
    count_gemm(e, 3, up);
  } else {
    launch_row_norm(X, D, XN, D, w.ffn_norm_g, w.ffn_norm_b, rows, D, c.ln_eps, c.norm_is_rms, s, nullptr, amx);
    up.a_amax = amx;
    gemm(e, up, s);
  }
  launch_gelu_gate(Ubuf, Gbuf, rows, F, s);
  GemmArgs dn;
  dn.a = Gbuf, dn.lda = F, dn.w = w.ffn_down, dn.ldw = F, dn.c = X, dn.ldc = D, dn.residual = X;
  dn.m = rows, dn.n = D, dn.k = F;
  gemm(e, dn, s);
}

}  // namespace

namespace lram::host {

// Block stack on X [B*T, D] (in-place residual stream) -> HID.  With more than one slice the HBM-bound cell
// kernels of all slices are serialised on `hbm` while each slice's projections / norms run on its own stream:
// while slice A's matrix memory streams through HBM, slice B's fp32-MFMA GEMMs use the otherwise idle matrix
// cores (and vice versa one half-layer later).
void run_xlstm_stack(lram_engine* e, const Pass& pass, int T, const uint8_t* reset, const std::vector<Slice>& sl, hipStream_t hbm) {
  const lram_config& c = e->cfg;
  const int D = c.d_model;
  const bool lazy = lazy_active(e, T);
  LRAM_REQUIRE(!(lazy && pass.hold != nullptr), "xLSTM stack: the lazy kernels have no hold rule (stored contexts run materialised)");
  // Tail fold of the step before (lram_engine::prefold): this step is the one it was launched for when nothing came in between (every
  // other entry completes it), the period and the batch are the same, there are still two slices and this step's folds take the
  // compact grid.  Then the pre-folded blocks count as folded: their read passes see the due envs as lazy_view_of reports them --
  // fold, n = 0, g0 = 1 -- which is what they are.  Otherwise the fold is completed here, ahead of everything the slices launch.
  int n_prefolded = 0;
  if (e->prefold.pending) {
    const lram_engine::Prefold& pf = e->prefold;
    if (lazy && sl.size() > 1 && pass.lane_rec == nullptr && pf.step == e->lazy_step && pf.period == e->lazy_period && pf.B == e->B &&
        lazy_bound_compact(e, e->lazy_step, T)) {
      n_prefolded = pf.blocks;
      e->prefold = lram_engine::Prefold{};
    } else {
      lazy_finish_prefold(e, hbm);
      for (const Slice& x : sl) stream_after(e, x.s, hbm);
    }
  }
  bool lazy_compact = false;   // this step's fold launches may use the compact grid (no window can overflow)
  if (lazy) {
    // Upper bound of pending tokens per fold class (env index mod period), tracked on the host: while no class can
    // overflow its window before its turn, the fold launch only covers the envs whose turn it is.
    const int P = e->lazy_period;
    lazy_compact = true;
    if ((int)e->lazy_bound.size() != P) {
      e->lazy_bound.assign(P, kLazyWindow);
      lazy_compact = false;
    }
    const int c_due = lazy_due_class(e->lazy_step, P);
    for (int cls = 0; cls < P; ++cls) {
      if (cls == c_due)
        e->lazy_bound[cls] = 0;
      else if (e->lazy_bound[cls] + T > kLazyWindow)
        lazy_compact = false;
      e->lazy_bound[cls] = std::min(e->lazy_bound[cls] + T, 4 * kLazyWindow);
    }
  }
  // This step's folds depend on nothing this step computes (window rows, coefficients and counts are last step's).
  // Two slices: they go onto the state-pass stream itself, into the two stretches of a step where that stream has nothing to
  // run -- fold_bubbles of them before the first read pass (the step's front end and block 0's projections are still under
  // way), the rest while both slices are inside an sLSTM block -- instead of beside the read passes, which they slow down.
  // One slice (everything on the caller's stream): fold(i) right ahead of block i.
  // (Measured and removed, profiles/EXPERIMENTS.md: folds on their own stream one block ahead of the cells, every fold queued
  // at the step start, folds fused with the readout of the envs they rewrite, gaps / staggered front ends.)
  const bool bubbles = lazy && sl.size() > 1;
  // One slice (everything else on the caller's stream): ALL of the step's folds go to a side stream at the step's start -- they
  // depend on nothing this step computes -- and the read pass of block i waits for fold i alone, instead of every fold sitting
  // on the one stream ahead of its block (206M at 64 envs: 17 folds of ~21 us each = 8 % of the step).
  // From 256 MiB of matrix memory per block (16M: 256 envs, 206M: 41); below, the extra stream's events cost more than the folds.
  // Same box, folds on the one stream vs on the side stream, env-steps/s: 206M at 32 / 64 envs 10.56k vs 10.56k / 15.18k vs 15.67k;
  // 16M at 128 / 256 / 448 envs 155.6k vs 149.5k / 224.2k vs 226.7k / 287.4k vs 297.2k.
  // (Only where the ONE slice is the automatic choice: a forced single slice -- lram_set_micro_batches(1), bench.py's "chip to
  // itself" measurement of the state pass -- keeps every kernel of the pass alone on the chip.)
  const bool side_folds = lazy && sl.size() == 1 && e->n_micro == 0 && mlstm_live_bytes(e) >= 256.0 * 1024 * 1024;
  hipStream_t fold_stream = hbm;
  std::vector<hipEvent_t> fold_done(side_folds ? c.n_blocks : 0, nullptr);
  if (side_folds) {
    if (!e->hbm_stream) LRAM_HIP_CHECK(hipStreamCreateWithFlags(&e->hbm_stream, hipStreamNonBlocking));
    fold_stream = e->hbm_stream;
    stream_after(e, fold_stream, sl[0].s);
  }
  std::vector<char> folded(c.n_blocks, 0);
  auto launch_folds = [&](int i) {  // one fold per block over all env slots: folds do not care about the slices
    fold_block(e, i, T, reset, lazy_compact, 0, fold_stream);
    folded[i] = 1;
  };
  auto next_mlstm = [&](int i) {
    for (int k = i + 1; k < c.n_blocks; ++k)
      if (!c.block_is_slstm[k]) return k;
    return -1;
  };
  for (int i = next_mlstm(-1), k = 0; i >= 0 && k < n_prefolded; i = next_mlstm(i), ++k) folded[i] = 1;   // (by the step before)
  if (bubbles) {
    int k = 0;
    const int ahead = pass.images != nullptr ? e->fold_bubbles_images : lram_engine::fold_bubbles;
    for (int i = next_mlstm(-1); i >= 0 && k < ahead; i = next_mlstm(i))
      if (!folded[i]) launch_folds(i), ++k;
  }
  // the last mLSTM block: the tail fold goes behind its read passes
  int last_mlstm = -1;
  for (int i = next_mlstm(-1); i >= 0; i = next_mlstm(i)) last_mlstm = i;
  // ... where the next step can take it over as it stands: the compact grid, judged by the bounds this step leaves
  const bool tail = bubbles && e->fold_tail && lazy_compact && pass.lane_rec == nullptr && lazy_bound_compact(e, e->lazy_step + 1, T);
  if (side_folds)
    for (int i = next_mlstm(-1); i >= 0; i = next_mlstm(i)) {
      launch_folds(i);
      fold_done[i] = ring_event(e);
      LRAM_HIP_CHECK(hipEventRecord(fold_done[i], fold_stream));
    }
  for (int i = 0; i < c.n_blocks; ++i) {
    if (i > 0 && pass.lane_rec) LRAM_HIP_CHECK(hipEventRecord((*pass.lane_rec)[i - 1], sl[0].s));   // (chunk lanes: one slice, one stream)
    if (pass.lane_wait) LRAM_HIP_CHECK(hipStreamWaitEvent(sl[0].s, (*pass.lane_wait)[i], 0));
    if (c.block_is_slstm[i]) {
      // (enqueued BEFORE the sLSTM block's ~50 launches: with short kernels the host is only just ahead of the device
      // there, and folds queued behind them reached the state-pass stream 0.26 ms after it had gone idle -- 206M, 512 slots)
      if (bubbles) {
        // the folds still outstanding run behind the previous block's read passes, shared out over this and the later sLSTM
        // blocks of the stack (206M: three stretches, five folds each, instead of fifteen in the first and none in the
        // other two); at least the blocks whose read passes come before the next sLSTM block
        int left = 0, stretches = 0, must = 0;
        for (int k = next_mlstm(i); k >= 0; k = next_mlstm(k)) left += folded[k] ? 0 : 1;
        for (int k = i; k < c.n_blocks; ++k) stretches += c.block_is_slstm[k] ? 1 : 0;
        for (int k = i + 1; k < c.n_blocks && !c.block_is_slstm[k]; ++k) must += folded[k] ? 0 : 1;
        int take = left;
        if (stretches > 1) take = std::max((take + stretches - 1) / stretches, std::min(must, take));
        for (int k = next_mlstm(i); k >= 0 && take > 0; k = next_mlstm(k))
          if (!folded[k]) launch_folds(k), --take;
      }
      for (const Slice& x : sl) slstm_block(e, pass, i, T, reset, x);
      continue;
    }
    if (lazy && !folded[i]) launch_folds(i);  // (one slice, or a stack without an sLSTM block: the fold ahead of its read passes)
    if (lazy && e->n_live < e->B) {
      // Parked slots take no token, but the bookkeeping is ping-ponged by step parity: what a read pass leaves on the "out" side
      // for a slot that received nothing -- coefficients, scale and count carried over; count 0 and g = 1 where the slot's fold
      // ran this step -- is written for slots [n_live, B) here.  It reads the "in" side only, as the folds do, and sits on the
      // first slice's stream ahead of that slice's read pass: the state-pass stream, and with it the tail fold, comes behind it.
      MlstmLazyArgs lp = lazy_args(e, i, T, nullptr, e->n_live, e->B - e->n_live);
      // (no fold was launched over the parked range: nothing there is due, whatever a window holds -- a phase no slot index meets)
      if (e->parked_windows_empty(e->lazy_step)) lp.phase = 1, lp.period = 1 << 30;
      launch_mlstm_lazy_parked(lp, sl[0].s);
    }
    for (const Slice& x : sl) {
      mlstm_front(e, pass, i, T, reset, x);
      if (lazy) {
        // lazy matrix memory: on the HBM stream the read-only pass with the window scores, the window attention and the
        // step's bookkeeping
        MlstmLazyArgs la = lazy_args(e, i, T, reset, x.b0, x.nb);
        const size_t r0 = (size_t)x.b0 * T;
        la.q = e->Q.p + r0 * e->icols, la.k = e->K.p + r0 * e->icols, la.v = e->V.p + r0 * e->icols;
        la.scal = e->SCAL.p + r0 * c.n_heads * 4, la.h = e->H.p + r0 * e->icols;
        // the read-only pass's occupancy cap (LDS per workgroup; 0 = the launcher's default of three workgroups per CU, 41 KB,
        // at 256-wide heads).  Slices below ~900 envs are CHAIN-bound -- the slice's projections / front end take longer than the
        // other slice's read pass -- and two read-pass workgroups per CU (54 KB) leave room for the two-stage projection
        // workgroups (155 VGPRs, 48 KB) to start beside them: 16M at 640 / 768 / 896 / 1024 / 1152 / 1280 / 1408 slots +1.5 / +2.6 /
        // +4.0 / +2.5 / +4.6 / +3.8 / +1.1 %, 1536-1792 +0.3-1 %, 2048 -1.3 %, 4096 -1.3 % (profiles/r05_ab_read_pass_lds_cap.txt)
        la.min_lds_bytes = (sl.size() >= 2 && x.nb <= e->lazy_cap2_envs && la.DH == 256) ? 54 * 1024 : 0;
        if (!mlstm_lazy_fused_scores(la.DH)) launch_mlstm_lazy_book(la, x.s);  // scores beside the front end
        if (lean_front(e, T)) {
          const BlockWeights& w = e->bw[i];
          la.lean_xa = e->XA.p + r0 * e->icols, la.lean_u = e->U.p + r0 * e->ucols;
          la.lean_wq = w.wq, la.lean_wk = w.wk, la.lean_wv = w.wv;
          if (gn_fused(e, T)) la.gn_g = w.on_g, la.gn_b = w.on_b, la.gn_skip = w.skip, la.gn_eps = c.ln_eps;
        }
        stream_after(e, hbm, x.s);
        if (side_folds) LRAM_HIP_CHECK(hipStreamWaitEvent(hbm, fold_done[i], 0));
        prof_record(e, hbm, true);
        launch_mlstm_lazy_cell(la, hbm);
        prof_record(e, hbm, false);
        mlstm_up_z(e, i, T, x);  // on the slice's stream, beside its own state pass
        stream_after(e, x.s, hbm);
        continue;
      }
      stream_after(e, hbm, x.s);
      mlstm_cell(e, pass, i, T, reset, x, hbm);
      mlstm_up_z(e, i, T, x);
      stream_after(e, x.s, hbm);
    }
    if (tail && i == last_mlstm) {
      // Next step's folds of the first fold_tail_blocks blocks, now: their window rows, coefficients, scales and counts are final
      // (this step's read passes of those blocks are done, in stream order), and the state-pass stream has nothing else to run
      // until the step ends.  No reset mask: it is next step's, not known yet -- an env that turns out to restart then has been
      // folded for nothing (its view sets `zero`, C_base is not read).  Enqueued ahead of the slices' join: the call leaves no
      // work behind on an engine stream.
      e->prefold.step = e->lazy_step + 1, e->prefold.period = e->lazy_period, e->prefold.B = e->B, e->prefold.blocks = 0;
      e->prefold.pending = true;
      for (int k = next_mlstm(-1); k >= 0 && e->prefold.blocks < lram_engine::fold_tail_blocks; k = next_mlstm(k)) {
        fold_block(e, k, T, nullptr, true, 1, hbm);
        ++e->prefold.blocks;
      }
    }
    for (const Slice& x : sl) mlstm_back(e, pass, i, T, x);
  }
  if (pass.lane_rec) LRAM_HIP_CHECK(hipEventRecord((*pass.lane_rec)[c.n_blocks - 1], sl[0].s));
  if (lazy) {
    ++e->lazy_step;
    e->lazy_dirty = true;
  }
  for (const Slice& x : sl) {
    const size_t r0 = (size_t)x.b0 * T;
    launch_row_norm(e->X.p + r0 * D, D, e->HID.p + r0 * D, D, e->post_g, e->post_b, x.nb * T, D, c.ln_eps,
                    c.norm_is_rms, x.s);
  }
}

}  // namespace lram::host
