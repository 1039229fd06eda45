"""GPU: every published model size of the reference (README.md:186-240) at full depth against the CPU oracle, on the paths
the engine takes for it in production.

  xLSTM-48M   [7:1] and [1:0]: mLSTM head dim 384 (lazy read pass with the separate score kernel), sLSTM head dim 192
  xLSTM-110M  [7:1] and [1:0]: head dim 512 (the read pass's 64-column instance), sLSTM head dim 256
  Mamba-16M / 110M / 206M:     dt_rank 32 / 64 / 80 -- the generic state-update kernel with dt_proj fused (the lane kernel is
                               for dt_rank 48 only); x_proj N = 64 / 96 on the narrow kernel, 112 on the tile GEMM path

Three kinds of runs, all on the weight distributions "exercise" and "reference" (lram_amd/weights.py::init_state_dict):

  few envs     4 (xLSTM) or 6 (Mamba) env slots, 30 env-steps with random restarts, lazy and materialised state (xLSTM),
  planted      the same envs planted at both ends of every env slice among random traffic, at the slot counts where the
               engine switches to f16x2 projections, lazy state, side-stream folds and two env slices; each run proves it
               reached the regime its name claims (state mode, f16x2 launches, bit-identity to the explicit slice count),
  stored       lram_prefill of a context whose balanced chunk split is uneven (43 = 15 + 15 + 13 timesteps) and of 4k + 1
  contexts     timesteps through the token-sequential chunks (a one-timestep last chunk through the chunk lanes), then lazy
               decoding.

Oracle bars (few envs and planted): 0 action ties, hidden states and the final recurrent state per row within 2e-4 of the
fp32 oracle or as close to the float64 evaluation as the fp32 oracle is (tests/helpers.py, escape hatch for at most 5 % of
the rows), C and n of every mLSTM block per element within ELEM_STATE_TOL (or, where the fp32 oracle itself is that far from
float64, see ELEM_FP64_CAP).  The oracle runs the sampled envs only, once per
(model, weight distribution): the cases of one model follow each other and share it."""
import os

import pytest
import torch

from lram_amd import init_state_dict, preset
from oracle.dt_ref import OraclePolicy
from tests.helpers import (ELEM_STATE_TOL, Fp64Oracle, assert_actions_match, assert_close_or_as_close_as_fp32_oracle,
                           elem_rel_err, make_inputs, rel_err, relaxed_rows_fraction, relaxed_rows_reset, sampled_state,
                           state_vs_oracle)

pytestmark = pytest.mark.gpu

STEPS, PERIOD, RESET_PROB = 30, 13, 0.05
SCHEMES = ("exercise", "reference")


def _n_env(spec):
    return 4 if spec.backbone == "xlstm" else 6


def _spec_sd(name, scheme):
    spec = preset(name)
    return spec, init_state_dict(spec, seed=0, scheme=scheme)


_ORACLE = {}


def _oracle(name, scheme):
    """fp32 and float64 oracle over the sampled envs' 30 steps: per-step actions / logits / hidden, final states.  One entry
    is kept (the cases of one model and weight distribution are consecutive)."""
    key = (name, scheme)
    if key not in _ORACLE:
        _ORACLE.clear()
        spec, sd = _spec_sd(name, scheme)
        n = _n_env(spec)
        seq = make_inputs(spec, n, STEPS, seed=4321, reset_prob=RESET_PROB)
        o32, o64 = OraclePolicy(spec, sd), Fp64Oracle(spec, sd)
        steps = []
        for obs, rtg, rew, mask in seq:
            a, d = o32.step(obs, rtg, rew, mask, return_debug=True)
            _, d64 = o64.step(obs, rtg, rew, mask, return_debug=True)
            steps.append({"actions": a, "logits": d["logits"], "hidden": d["hidden"], "hidden64": d64["hidden"]})
        _ORACLE[key] = {"spec": spec, "sd": sd, "seq": seq, "steps": steps, "state": o32.state, "state64": o64.ora.state}
    return _ORACLE[key]


def _folds(where, seq):
    """Folds per planted env under the engine's rule (mlstm_lazy.hip::lazy_view: due where (slot + step) % period == 0 with a
    non-empty window, not on a restart)."""
    slot = torch.as_tensor(where)
    folds, pending = torch.zeros(len(where), dtype=torch.long), torch.zeros(len(where), dtype=torch.long)
    for t, (_, _, _, mask) in enumerate(seq):
        due = ((slot + t) % PERIOD == 0) & (pending > 0) & ~mask.bool()
        folds += due.long()
        pending = torch.where(mask.bool() | due, torch.zeros_like(pending), pending) + 3
    return folds


def _drive(o, slots, where, mode=None, micro=None, keep=False):
    """One engine over the oracle's 30 steps with the sampled envs at `where` and random traffic everywhere else.  Returns the
    engine (open) and, with keep, every step's actions of all slots, the last step's taps and a few state tensors."""
    from lram_amd.engine import Engine
    spec, sd, seq = o["spec"], o["sd"], o["seq"]
    eng = Engine(spec, sd, slots, device="cuda:0")
    if mode is not None:
        eng.set_state_mode(mode)
    if micro is not None:
        eng.set_micro_batches(micro)
    eng.gemm_counts(reset=True)
    idx = torch.as_tensor(where, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(slots)
    d_obs = torch.zeros(slots, spec.state_dim, device="cuda")
    d_rtg = torch.full((slots,), 4.5, device="cuda")
    d_rew = torch.zeros(slots, device="cuda")
    d_mask = torch.ones(slots, dtype=torch.uint8, device="cuda")
    out = {"acts": [], "hidden": [], "a_where": []}
    for t, (obs, rtg, rew, mask) in enumerate(seq):
        if slots > len(where):
            d_obs[:, : spec.state_dim * 3 // 4] = torch.rand(slots, spec.state_dim * 3 // 4, generator=g, device="cuda") * 2 - 1
            if t > 0:
                d_mask.copy_((torch.rand(slots, generator=g, device="cuda") < 0.02).to(torch.uint8))
            d_rtg.copy_(torch.where(d_mask.bool(), torch.full_like(d_rtg, 4.5), d_rtg - 0.01))
        d_obs[idx], d_rtg[idx], d_rew[idx], d_mask[idx] = obs.cuda(), rtg.cuda(), rew.cuda(), mask.cuda()
        a, _ = eng.step(d_obs, d_rtg, d_rew, d_mask)
        torch.cuda.synchronize()
        _, hidden, logits = eng.taps()
        out["a_where"].append(a[idx].cpu())
        out["hidden"].append(hidden[idx].cpu())
        if keep:
            out["acts"].append(a.cpu().clone())
    if keep:
        _, hidden, logits = eng.taps()
        out["taps"] = (hidden.cpu(), logits.cpu())
        blocks = sorted({0, spec.n_blocks - 1, *spec.slstm_at[:1]})
        out["state"] = {(i, w): eng.export_state_tensor(i, w) for i in blocks for w in (0, 3)}   # (kept on the device: 1 GiB at 110M x 256)
    return eng, out


def _state_pairs(eng, o, where):
    """(what, engine tensor, fp32 oracle, float64 oracle, per-element check) for every state tensor of the sampled envs, env-major."""
    spec = o["spec"]
    idx = torch.as_tensor(where, device="cuda")
    for i in range(spec.n_blocks):
        if spec.backbone == "mamba":
            for w, j in ((3, 0), (0, 1)):   # (conv, ssm) = state[i]
                yield f"layer {i} {('conv', 'ssm')[j]}", eng.export_state_tensor(i, w)[idx].cpu(), o["state"][i][j], o["state64"][i][j], False
            continue
        ref, r64 = o["state"][f"block_{i}"], o["state64"][f"block_{i}"]
        yield f"block {i} conv", eng.export_state_tensor(i, 3)[idx].cpu(), ref["conv_state"][0], r64["conv_state"][0], False
        if i in spec.slstm_at:
            yield (f"block {i} sLSTM", eng.export_state_tensor(i, 0)[:, idx].cpu().transpose(0, 1),
                   ref["slstm_state"].transpose(0, 1), r64["slstm_state"].transpose(0, 1), False)
        else:
            for w, what in enumerate(("C", "n", "m")):
                yield f"block {i} {what}", eng.export_state_tensor(i, w)[idx].cpu(), ref["mlstm_state"][w], r64["mlstm_state"][w], w < 2


# Per-element bar on C and n: ELEM_STATE_TOL against the fp32 oracle; beyond it, the tensor's worst element against the float64
# evaluation within 8 x the fp32 oracle's own per-element distance from it, and never beyond this cap.  The [1:0] stacks of 12 and
# 16 mLSTM blocks on the "exercise" weights need it in their deepest blocks: there the fp32 oracle itself is up to 7.8e-3 per
# element from float64 (48M block 11) -- small entries (1e-5 ... 1e-4 of the tensor's largest) that follow the ~1e-5 relative
# rounding the block's inputs carry after 10+ blocks; measured engine vs float64 on those tensors: 3.1e-3 ... 7.6e-3.
ELEM_FP64_CAP = 1e-2


def _check_oracle(eng, out, o, where, name):
    """Actions (0 ties), hidden states at every step and the final state against the oracle; returns the report line."""
    spec = o["spec"]
    relaxed_rows_reset()
    ties = 0
    for t, st in enumerate(o["steps"]):
        assert_close_or_as_close_as_fp32_oracle(out["hidden"][t], st["hidden"], st["hidden64"], what=f"{name} step {t}: hidden")
        ties += assert_actions_match(out["a_where"][t], st["actions"], st["logits"], spec, what=f"{name} step {t}")
    worst, relaxed_elem = 0.0, 0
    n = len(where)
    for what, got, want, want64, elem in _state_pairs(eng, o, where):
        assert_close_or_as_close_as_fp32_oracle(got.reshape(n, 1, -1), want.reshape(n, 1, -1), want64.reshape(n, 1, -1),
                                                what=f"{name} final {what}")
        if elem:   # C and n entries span orders of magnitude: each one relative to itself
            e = elem_rel_err(got, want)
            worst = max(worst, e)
            if e >= ELEM_STATE_TOL:   # (see ELEM_FP64_CAP)
                e64, o64 = elem_rel_err(got, want64), elem_rel_err(want, want64)
                relaxed_elem += 1
                assert e64 <= min(8.0 * o64, ELEM_FP64_CAP), \
                    f"{name} final {what}: per-element relative error {e:.2e}; vs float64 {e64:.2e}, fp32 oracle vs float64 {o64:.2e}"
    frac = relaxed_rows_fraction()
    assert ties == 0, f"{name}: {ties} action ties"
    assert frac <= 0.05, f"{name}: {frac:.1%} of the rows needed the float64 rule"
    if os.environ.get("LRAM_TEST_REPORT"):
        print(f"[report] {name}: mode {eng.state_mode}, ties {ties}, float64-rule rows {frac:.2%}, worst C/n element {worst:.2e}, "
              f"C/n tensors on the float64 rule {relaxed_elem}")


def _assert_bit_identical(a, b, what):
    assert all(torch.equal(x, y) for x, y in zip(a["acts"], b["acts"])), f"{what}: actions"
    assert torch.equal(a["taps"][0], b["taps"][0]) and torch.equal(a["taps"][1], b["taps"][1]), f"{what}: hidden / logits"
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), f"{what}: state {k}"


# (model, regime name, slots, state mode, env slices, f16x2 projections).  The thresholds these slot counts sit beside
# (csrc/engine.hip, engine_xlstm.hip, engine_streams.hip, engine_gemm.hip): lazy from 128 MiB of one block's matrix memory over the batch, side-stream folds from 256 MiB, two env
# slices from 512 MiB (xLSTM) / 1024 slots (Mamba); f16x2 below 256 operand rows from 96 rows for weights of >= 1.1 M elements
# and from 48 rows for >= 2.5 M (48M: proj_up 3072 x 768 at 32 envs; 110M: proj_up 4096 x 1024 at 16 envs).
REGIMES = {
    "xlstm_48m": [("f16x2_materialised_one_slice", 32, "materialised", 1, True),
                  ("lazy_one_slice_side_stream_folds", 160, "lazy", 1, False),
                  ("lazy_two_slices", 256, "lazy", 2, False)],
    "xlstm_110m": [("f16x2_materialised_one_slice", 16, "materialised", 1, True),
                   ("lazy_one_slice_side_stream_folds", 96, "lazy", 1, False),
                   ("lazy_two_slices", 256, "lazy", 2, False)],
    **{m: [("one_slice_generic_state_update", 128, "materialised", 1, False),
           ("two_slices", 1024, "materialised", 2, False)] for m in ("mamba_16m", "mamba_110m", "mamba_206m")},
}
MODELS = ("xlstm_48m", "xlstm_48m_mlstm", "xlstm_110m", "xlstm_110m_mlstm", "mamba_16m", "mamba_110m", "mamba_206m")
CASES = [(m, s, r) for m in MODELS for s in SCHEMES
         for r in [("few_envs_lazy_and_materialised" if m.startswith("xlstm") else "few_envs_materialised", 0, None, 0, False)]
         + REGIMES.get(m, [])]


def _planted(slots, slices, n):
    """Sampled envs at both ends of every slice (n = 4: first two and last two slots of one slice; 4 or 6 ends of two)."""
    if slices == 1:
        return [0, 1, slots - 2, slots - 1][:n] if n == 4 else [0, 1, 2, slots - 3, slots - 2, slots - 1]
    h = slots // 2
    return [0, h - 1, h, slots - 1] if n == 4 else [0, 1, h - 1, h, slots - 2, slots - 1]


@pytest.mark.parametrize("name,scheme,regime", CASES, ids=[f"{m}-{s}-{r[0]}" for m, s, r in CASES])
def test_published_model_against_the_oracle(hip_lib, name, scheme, regime):
    o = _oracle(name, scheme)
    spec = o["spec"]
    n = _n_env(spec)
    label, slots, mode, slices, f16 = regime
    if spec.backbone == "mamba":
        assert spec.dt_rank != 48   # not the lane kernel's geometry: the generic selective-state-update kernel
    if slots == 0:   # few envs: the sampled envs alone
        modes = ("lazy", "eager") if spec.backbone == "xlstm" else ("eager",)
        if spec.backbone == "mamba":
            from lram_amd.engine import Engine, LramError
            eng = Engine(spec, o["sd"], n, device="cuda:0")
            with pytest.raises(LramError):   # no lazy form of a Mamba state
                eng.set_state_mode("lazy")
            eng.close()
        for m in modes:
            where = list(range(n))
            if m == "lazy":
                assert int(_folds(where, o["seq"]).min()) >= 2
            eng, out = _drive(o, n, where, mode=m)
            assert eng.state_mode == ("lazy" if m == "lazy" else "materialised")
            _check_oracle(eng, out, o, where, f"{name} {scheme} {n} envs {m}")
            eng.close()
        return
    where = _planted(slots, slices, n)
    if mode == "lazy":
        assert int(_folds(where, o["seq"]).min()) >= 2
    eng, out = _drive(o, slots, where, keep=True)
    what = f"{name} {scheme} {slots} slots"
    assert eng.state_mode == mode, what
    if f16:
        assert eng.gemm_counts()["f16x2"]["launches"] > 0, what
    _check_oracle(eng, out, o, where, what)
    eng.close()
    torch.cuda.empty_cache()
    # the automatic slice count is the one the regime claims: the same run with it set explicitly is the same computation, bit
    # for bit (a forced single slice keeps the folds on the step's stream: the side-stream folds must not change a bit either)
    eng2, out2 = _drive(o, slots, where, micro=slices, keep=True)
    eng2.close()
    torch.cuda.empty_cache()
    _assert_bit_identical(out, out2, f"{what}: automatic vs {slices} slice(s)")


# ---- stored contexts ------------------------------------------------------------------------------------------------------
def _seq_tensors(seq, L):
    return [torch.stack([x[k] for x in seq[:L]], 1).contiguous().cuda() for k in range(3)]


def _all_states_equal(a, b, spec, what):
    for blk in range(spec.n_blocks):
        kinds = (0, 3) if (spec.backbone == "mamba" or blk in spec.slstm_at) else (0, 1, 2, 3)
        for w in kinds:
            assert torch.equal(a.export_state_tensor(blk, w), b.export_state_tensor(blk, w)), f"{what}: block {blk} state {w}"


B_CTX, SAMPLE, L_UNEVEN, L_4K1, DECODE = 16, [0, 5, 10, 15], 43, 41, 15


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", ["xlstm_48m", "xlstm_110m"])
def test_xlstm_stored_context_then_lazy_decode(hip_lib, monkeypatch, name, scheme):
    """16 envs.  L = 43 through the chunkwise kernels in three chunks of 15 / 15 / 13 timesteps: the chunk lanes == one chunk at a
    time (LRAM_PREFILL_CHUNK=3) bit for bit; the bf16x3 chunk cell within 1e-5 of the exact-fp32 one (LRAM_PREFILL_CHUNK=2); the
    oracle stepped through the same context: actions and the final state; then 15 lazy env-steps against the oracle continuing.
    L = 41 = 4 * 10 + 1 under LRAM_PREFILL_CHUNK=0: token-sequential chunks of 4 timesteps and a one-timestep last chunk through
    the lanes, against the oracle at step 41."""
    from lram_amd.engine import Engine
    spec, sd = _spec_sd(name, scheme)
    assert (spec.head_dim, spec.n_heads) in ((384, 4), (512, 4))
    seq = make_inputs(spec, B_CTX, L_UNEVEN + DECODE, seed=77, reset_prob=0.0)
    ones = torch.ones(B_CTX, dtype=torch.uint8, device="cuda")
    engines = {}
    for env in (None, "3", "2", "0"):
        if env is None:
            monkeypatch.delenv("LRAM_PREFILL_CHUNK", raising=False)
        else:
            monkeypatch.setenv("LRAM_PREFILL_CHUNK", env)
        engines[env] = Engine(spec, sd, B_CTX, device="cuda:0")
    monkeypatch.delenv("LRAM_PREFILL_CHUNK")
    lanes = engines[None]
    lanes.set_state_mode("lazy")
    a_l, _ = lanes.prefill(*_seq_tensors(seq, L_UNEVEN), reset_mask=ones)
    a_l = a_l.clone()
    a_s, _ = engines["3"].prefill(*_seq_tensors(seq, L_UNEVEN), reset_mask=ones)
    a_f, _ = engines["2"].prefill(*_seq_tensors(seq, L_UNEVEN), reset_mask=ones)
    a_t, _ = engines["0"].prefill(*_seq_tensors(seq, L_4K1), reset_mask=ones)
    torch.cuda.synchronize()
    assert torch.equal(a_l, a_s)
    assert float((a_l - a_f).abs().max()) <= 1e-5
    _all_states_equal(lanes, engines["3"], spec, f"{name} lanes vs one chunk at a time")
    for blk in range(spec.n_blocks):
        kinds = (0, 3) if blk in spec.slstm_at else (0, 1, 2, 3)
        for w in kinds:
            assert rel_err(lanes.export_state_tensor(blk, w), engines["2"].export_state_tensor(blk, w)) < 1e-5, (blk, w)
    ora = OraclePolicy(spec, sd)
    sample = torch.tensor(SAMPLE)
    ties = 0
    for t, (obs, rtg, rew, mask) in enumerate(seq):
        a_ref, dbg = ora.step(obs[sample], rtg[sample], rew[sample], mask[sample], return_debug=True)
        if t + 1 == L_4K1:
            ties += assert_actions_match(a_t[sample], a_ref, dbg["logits"], spec, what=f"{name} prefill L={L_4K1}")
            state_vs_oracle(sampled_state(engines["0"], spec, SAMPLE), ora.state, spec, f"{name} prefill L={L_4K1}")
        elif t + 1 == L_UNEVEN:
            ties += assert_actions_match(a_l[sample], a_ref, dbg["logits"], spec, what=f"{name} prefill L={L_UNEVEN}")
            state_vs_oracle(sampled_state(lanes, spec, SAMPLE), ora.state, spec, f"{name} prefill L={L_UNEVEN}")
        elif t + 1 > L_UNEVEN:   # lazy decoding from the state the prefill left
            a, _ = lanes.step(obs.cuda(), rtg.cuda(), rew.cuda(), None)
            torch.cuda.synchronize()
            assert lanes.state_mode == "lazy"
            _, hidden, _ = lanes.taps()
            assert rel_err(hidden[sample.cuda()], dbg["hidden"]) < 2e-4, f"{name} decode step {t}: hidden"
            ties += assert_actions_match(a[sample.cuda()], a_ref, dbg["logits"], spec, what=f"{name} decode step {t}")
    state_vs_oracle(sampled_state(lanes, spec, SAMPLE), ora.state, spec, f"{name} after {DECODE} lazy steps")
    assert ties == 0, ties
    for e in engines.values():
        e.close()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", ["mamba_16m", "mamba_110m", "mamba_206m"])
def test_mamba_stored_context_through_the_chunk_lanes(hip_lib, monkeypatch, name, scheme):
    """16 envs x 41 timesteps = ten chunks of 4 and a one-timestep last chunk, three chunks in flight: bit-identical to one chunk
    at a time (LRAM_PREFILL_CHUNK=3), equal to 41 lram_step calls (actions within 1e-4, states within 1e-4) and to the oracle."""
    from lram_amd.engine import Engine
    spec, sd = _spec_sd(name, scheme)
    seq = make_inputs(spec, B_CTX, L_4K1, seed=78, reset_prob=0.0)
    ones = torch.ones(B_CTX, dtype=torch.uint8, device="cuda")
    lanes = Engine(spec, sd, B_CTX, device="cuda:0")
    monkeypatch.setenv("LRAM_PREFILL_CHUNK", "3")
    serial = Engine(spec, sd, B_CTX, device="cuda:0")
    monkeypatch.delenv("LRAM_PREFILL_CHUNK")
    stepper = Engine(spec, sd, B_CTX, device="cuda:0")
    a_l, _ = lanes.prefill(*_seq_tensors(seq, L_4K1), reset_mask=ones)
    a_s, _ = serial.prefill(*_seq_tensors(seq, L_4K1), reset_mask=ones)
    for t, (obs, rtg, rew, _) in enumerate(seq):
        a_step, _ = stepper.step(obs.cuda(), rtg.cuda(), rew.cuda(), ones if t == 0 else None)
    torch.cuda.synchronize()
    assert torch.equal(a_l, a_s)
    _all_states_equal(lanes, serial, spec, f"{name} lanes vs one chunk at a time")
    assert float((a_l - a_step).abs().max()) <= 1e-4
    for blk in range(spec.n_blocks):
        for w in (0, 3):
            assert rel_err(lanes.export_state_tensor(blk, w), stepper.export_state_tensor(blk, w)) < 1e-4, (blk, w)
    ora = OraclePolicy(spec, sd)
    sample = torch.tensor(SAMPLE)
    for obs, rtg, rew, mask in seq:
        a_ref, dbg = ora.step(obs[sample], rtg[sample], rew[sample], mask[sample], return_debug=True)
    assert assert_actions_match(a_l[sample.cuda()], a_ref, dbg["logits"], spec, what=f"{name} prefill") == 0
    state_vs_oracle(sampled_state(lanes, spec, SAMPLE), ora.state, spec, f"{name} prefill")
    for e in (lanes, serial, stepper):
        e.close()
