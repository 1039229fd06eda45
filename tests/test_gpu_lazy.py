"""Lazy matrix memory (lram_set_state_mode, csrc/mlstm_lazy.hip): C_base is read once per step and rewritten once per
fold period, the tokens in between live in a window the readout attends over.  Must be indistinguishable from the
materialised update: oracle parity, equality with the eager engine, resets, exports in the middle of a window,
prefill hand-over, env slices, every fold period, the 206M head geometry."""
import pytest
import torch

from lram_amd import init_state_dict, preset
from lram_amd.config import ModelSpec
from oracle import dt_ref
from tests.geometry_cases import case_spec
from tests.helpers import assert_actions_match, make_inputs, rel_err

pytestmark = pytest.mark.gpu


def _run(eng, seq):
    acts = []
    for obs, rtg, rew, mask in seq:
        a, _ = eng.step(obs.cuda(), rtg.cuda(), rew.cuda(), mask.cuda())
        acts.append(a.clone())
    torch.cuda.synchronize()
    return torch.stack(acts)


@pytest.mark.parametrize("period", [13, 1, 5, 14])   # (period 13 over 1000 steps: tests/test_gpu_horizon.py)
def test_lazy_steps_match_oracle_and_eager(hip_lib, period):
    """45 steps with random per-env resets: several staggered folds per env; actions follow the oracle, the exported
    state equals the eager engine's."""
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=51)
    B, steps = 5, 45
    seq = make_inputs(spec, B, steps, seed=21, reset_prob=0.1)
    eager = Engine(spec, sd, B, device="cuda:0")
    eager.set_state_mode("eager")
    lazy = Engine(spec, sd, B, device="cuda:0")
    lazy.set_state_mode(True, period)
    assert eager.state_mode == "materialised" and lazy.state_mode == "lazy"
    a_e, a_l = _run(eager, seq), _run(lazy, seq)
    ora = dt_ref.OraclePolicy(spec, sd)
    for t, (obs, rtg, rew, mask) in enumerate(seq):
        ref, dbg = ora.step(obs, rtg, rew, mask, return_debug=True)
        assert_actions_match(a_l[t], ref, dbg["logits"], spec, what=f"lazy period {period} step {t}")
    assert float((a_e - a_l).abs().max()) <= 1e-4
    for blk in (0, 2, 7):
        for which in (0, 1, 2, 3):
            assert rel_err(lazy.export_state_tensor(blk, which), eager.export_state_tensor(blk, which)) < 2e-4, (blk, which)
    eager.close(), lazy.close()


def test_lazy_export_prefill_and_mode_switches(hip_lib):
    """Exports in the middle of a window, a prefill in between, leaving and re-entering lazy mode: none of it changes
    the trajectory."""
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=52)
    B = 4
    seq = make_inputs(spec, B, 30, seed=22, reset_prob=0.0)
    ctx = make_inputs(spec, B, 20, seed=23, reset_prob=0.0)
    obs_seq = torch.stack([x[0] for x in ctx], 1).contiguous().cuda()
    rtg_seq = torch.stack([x[1] for x in ctx], 1).contiguous().cuda()
    rew_seq = torch.stack([x[2] for x in ctx], 1).contiguous().cuda()
    eager = Engine(spec, sd, B, device="cuda:0")
    eager.set_state_mode("eager")
    lazy = Engine(spec, sd, B, device="cuda:0")
    lazy.set_state_mode(True)
    outs = []
    for eng in (eager, lazy):
        acts = [_run(eng, seq[:7])]
        c_mid = eng.export_state_tensor(3, 0).clone()          # folds the pending windows in lazy mode
        acts.append(_run(eng, seq[7:11]))
        a_pre, _ = eng.prefill(obs_seq, rtg_seq, rew_seq)        # chunkwise kernels on the materialised state
        acts.append(a_pre.clone().unsqueeze(0))
        acts.append(_run(eng, seq[11:20]))
        if eng is lazy:
            eng.set_state_mode(False)
        acts.append(_run(eng, seq[20:24]))
        if eng is lazy:
            eng.set_state_mode(True, 4)
        acts.append(_run(eng, seq[24:]))
        outs.append((torch.cat(acts), c_mid, eng.export_state_tensor(0, 0).clone(), eng.export_state_tensor(7, 1).clone()))
    assert float((outs[0][0] - outs[1][0]).abs().max()) <= 1e-4
    for i in (1, 2, 3):
        assert rel_err(outs[1][i], outs[0][i]) < 2e-4, i
    eager.close(), lazy.close()


def test_lazy_env_slices_and_206m_geometry(hip_lib, monkeypatch):
    """Two env slices fold the same envs at the same steps as one slice (bit-identical), and the 5-column-slice head
    geometry of the 206M model (DH = 640) follows the oracle.  Bit for bit needs the same projection kernel for a GEMM of 3
    operand rows (a slice's state embedding, its head) and of 6 (the un-sliced batch): the few-row kernel's lower limit (5
    rows by default, GEMV below) is raised above both for that comparison; with the default limit the two runs agree to
    fp32 rounding, which is asserted as well."""
    from lram_amd.engine import Engine
    spec = ModelSpec(backbone="xlstm", d_model=1280, n_blocks=2, slstm_at=[1])
    sd = init_state_dict(spec, seed=53)
    B = 6
    seq = make_inputs(spec, B, 18, seed=24, reset_prob=0.1)

    def both(min_rows):
        if min_rows is None:
            monkeypatch.delenv("LRAM_GEMM_SKINNY_MIN", raising=False)
        else:
            monkeypatch.setenv("LRAM_GEMM_SKINNY_MIN", str(min_rows))
        res = []
        for micro in (1, 2):
            eng = Engine(spec, sd, B, device="cuda:0")
            eng.set_state_mode(True, 5)
            eng.set_micro_batches(micro)
            res.append((_run(eng, seq), eng.export_state_tensor(0, 0).clone()))
            eng.close()
        return res

    dflt = both(None)
    assert float((dflt[0][0] - dflt[1][0]).abs().max()) <= 1e-4 and rel_err(dflt[0][1], dflt[1][1]) < 1e-5
    outs = both(9)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ora = dt_ref.OraclePolicy(spec, sd)
    for t, (obs, rtg, rew, mask) in enumerate(seq):
        ref, dbg = ora.step(obs, rtg, rew, mask, return_debug=True)
        assert_actions_match(outs[0][0][t], ref, dbg["logits"], spec, what=f"206M geometry step {t}")


# Seeds of test_lazy_long_window_on_sliced_heads (weights: seed; inputs: 1234 + seed), chosen on the CPU as geometry_cases.STEP_SEEDS
# are: over the whole trajectory (5 envs, 40 steps, reset probability 0.1) the ORACLE's own smallest top-2 logit gap is at least
# 1e-3, five times the tie rule of helpers.assert_actions_match.  Value: (spec, seed, measured smallest gap).
LONG_WINDOW_CASES = {
    "nh2_dh512": (lambda: case_spec("nh2_dh512"), 7, 1.1e-03),
    # (the 206M head geometry, 4 heads x 640, with the sweep's state_dim 20 / act_dim 4: 800 logit rows, as nh2_dh512 has)
    "dh640": (lambda: ModelSpec(backbone="xlstm", d_model=1280, n_blocks=2, slstm_at=[1], state_dim=20, act_dim=4), 27, 2.0e-03),
}


@pytest.mark.parametrize("cid", list(LONG_WINDOW_CASES))
def test_lazy_long_window_on_sliced_heads(hip_lib, cid):
    """More than 36 pending rows in front of a sliced-head read pass (scores from mlstm_lazy_score_kernel, v rows beyond the 36-row
    register prefetch loaded late): fold period 14 -- the longest lram_set_state_mode accepts, period * 3 + 4 <= 48; 39 rows are
    pending at an env's last read pass before its fold -- over 40 steps with random restarts, at head dims 512 (LPR 64) and 640
    (LPR 32).  Actions follow the oracle without a tie, lazy equals eager at the bars of test_lazy_steps_match_oracle_and_eager."""
    from lram_amd.engine import Engine
    make_spec, seed, gap = LONG_WINDOW_CASES[cid]
    assert gap >= 1e-3
    spec = make_spec()
    sd = init_state_dict(spec, seed=seed)
    B, steps = 5, 40
    seq = make_inputs(spec, B, steps, seed=1234 + seed, reset_prob=0.1)
    eager = Engine(spec, sd, B, device="cuda:0")
    eager.set_state_mode("eager")
    lazy = Engine(spec, sd, B, device="cuda:0")
    lazy.set_state_mode(True, 14)
    assert eager.state_mode == "materialised" and lazy.state_mode == "lazy"
    a_e, a_l = _run(eager, seq), _run(lazy, seq)
    ora = dt_ref.OraclePolicy(spec, sd)
    ties = 0
    for t, (obs, rtg, rew, mask) in enumerate(seq):
        ref, dbg = ora.step(obs, rtg, rew, mask, return_debug=True)
        ties += assert_actions_match(a_l[t], ref, dbg["logits"], spec, what=f"{cid} period 14 step {t}")
    assert ties == 0
    assert float((a_e - a_l).abs().max()) <= 1e-4
    for which in (0, 1, 2, 3):
        assert rel_err(lazy.export_state_tensor(0, which), eager.export_state_tensor(0, which)) < 2e-4, which
    eager.close(), lazy.close()


def test_lazy_mode_is_refused_or_ignored_where_it_does_not_apply(hip_lib):
    from lram_amd.engine import Engine, LramError
    tiny = preset("xlstm_tiny")                                   # head dim 64
    eng = Engine(tiny, init_state_dict(tiny, 0), 2, device="cuda:0")
    with pytest.raises(LramError):
        eng.set_state_mode(True)
    eng.close()
    mam = preset("mamba_tiny")
    eng = Engine(mam, init_state_dict(mam, 0), 2, device="cuda:0")
    with pytest.raises(LramError):
        eng.set_state_mode(True)
    eng.close()


def test_auto_mode_picks_lazy_only_where_the_state_pass_dominates(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=1)
    small = Engine(spec, sd, 8, device="cuda:0")          # 8 MiB of matrix memory per block: materialised
    assert small.state_mode == "materialised"
    small.close()
    mid = Engine(spec, sd, 96, device="cuda:0")           # 96 MiB: still materialised
    assert mid.state_mode == "materialised"
    mid.close()
    big = Engine(spec, sd, 128, device="cuda:0")          # 128 MiB per block: lazy
    assert big.state_mode == "lazy"
    big.set_state_mode("eager")
    assert big.state_mode == "materialised"
    big.set_state_mode("auto")
    assert big.state_mode == "lazy"
    big.close()


@pytest.mark.parametrize("period", [13, 3])
def test_lazy_encoder_step_token_counts(hip_lib, period):
    """lram_encoder_step with 1..4 tokens per call in lazy mode (4-token calls fill the 48-token window faster than the
    fold phase empties it: the overflow folds take the full-grid path), longer calls fold first and run on the
    materialised kernels; hidden states and the final state follow the oracle."""
    from lram_amd.engine import Engine
    from oracle import xlstm_ref
    spec = ModelSpec(backbone="xlstm", d_model=256, n_blocks=3, slstm_at=[1])   # 4 heads x 128
    sd = init_state_dict(spec, seed=61)
    B = 3
    eng = Engine(spec, sd, B, device="cuda:0")
    eng.set_state_mode("lazy", period)
    state = None
    g = torch.Generator().manual_seed(12)
    for T in [4] * 14 + [1, 2, 3, 4, 9, 4, 4, 1, 30, 2, 4, 4, 4]:
        x = torch.randn(B, T, spec.d_model, generator=g)
        ref, state = xlstm_ref.encoder_forward_cached(spec, sd, x, state)
        out = eng.encoder_step(x.cuda())
        torch.cuda.synchronize()
        assert rel_err(out, ref) < 2e-4, T
    pkv = eng.export_past_key_values()
    for i in range(3):
        assert rel_err(pkv["block_0"]["mlstm_state"][i], state["block_0"]["mlstm_state"][i]) < 2e-4, i
    assert rel_err(pkv["block_2"]["mlstm_state"][0], state["block_2"]["mlstm_state"][0]) < 2e-4
    eng.close()


def test_lazy_fused_group_norm_variant(hip_lib, monkeypatch):
    """LRAM_GN_FUSE=1 (opt-in): output group norm + skip in the read pass's epilogue, silu(z) from proj_up's epilogue,
    the gate applied while proj_down stages its operand.  Same trajectory as the default lazy engine and the oracle."""
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=57)
    B, steps = 64, 30
    seq = make_inputs(spec, B, steps, seed=27, reset_prob=0.05)
    base = Engine(spec, sd, B, device="cuda:0")
    base.set_state_mode(True)
    monkeypatch.setenv("LRAM_GN_FUSE", "1")
    fused = Engine(spec, sd, B, device="cuda:0")
    monkeypatch.delenv("LRAM_GN_FUSE")
    fused.set_state_mode(True)
    a_b, a_f = _run(base, seq), _run(fused, seq)
    assert float((a_b - a_f).abs().max()) <= 1e-4
    ora = dt_ref.OraclePolicy(spec, sd)
    sample = [0, 17, 63]
    for t, (obs, rtg, rew, mask) in enumerate(seq):
        ref, dbg = ora.step(obs[sample], rtg[sample], rew[sample], mask[sample], return_debug=True)
        assert_actions_match(a_f[t][sample], ref, dbg["logits"], spec, what=f"fused group norm step {t}")
    for blk in (0, 2, 7):
        assert rel_err(fused.export_state_tensor(blk, 0), base.export_state_tensor(blk, 0)) < 2e-4
    base.close(), fused.close()


def test_lazy_peek_looks_without_folding(hip_lib):
    """lram_lazy_peek (evidence hook of the long-horizon tests): g, m and the pending-token counts of the lazy representation
    without the fold an export triggers; refused in materialised mode and for sLSTM blocks."""
    from lram_amd.engine import Engine, LramError
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=59)
    B = 6
    eng = Engine(spec, sd, B, device="cuda:0")
    eng.set_state_mode("lazy", 13)
    seq = make_inputs(spec, B, 5, seed=29, reset_prob=0.0)
    _run(eng, seq)
    pend = eng.lazy_peek(0, "pending")
    # 5 steps x 3 tokens, minus what an env folded when its phase came up ((step + env) % 13 == 0 within these steps)
    assert pend.shape == (B,) and float(pend.max()) == 15.0 and float(pend.min()) >= 3.0
    g, m = eng.lazy_peek(0, "g"), eng.lazy_peek(0, "m")
    assert g.shape == (B, spec.n_heads) and bool((g > 0).all()) and bool((g <= 1).all()) and bool(torch.isfinite(m).all())
    assert torch.equal(eng.lazy_peek(0, "pending"), pend)            # looking twice changes nothing
    assert torch.equal(m.view(-1), eng.export_state_tensor(0, 2).view(-1))   # (the export folds: afterwards nothing is pending)
    assert float(eng.lazy_peek(0, "pending").max()) == 0.0
    with pytest.raises(LramError):
        eng.lazy_peek(spec.slstm_at[0], "g")
    eng.set_state_mode("eager")
    with pytest.raises(LramError):
        eng.lazy_peek(0, "g")
    eng.close()


def test_read_pass_occupancy_cap_changes_nothing(hip_lib, monkeypatch):
    """Slices of at most LRAM_LAZY_CAP2_ENVS envs run their read pass two workgroups to a CU (so that the other slice's projection
    workgroups start beside it); larger ones three.  Occupancy is not arithmetic: 1024 slots (two slices of 512) give the same
    bits with the cap off, and so does a batch whose slices are above the threshold."""
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=57)
    B = 1024
    seq = make_inputs(spec, B, 5, seed=29, reset_prob=0.05)
    outs = []
    for cap in (None, "0", "256"):
        if cap is None:
            monkeypatch.delenv("LRAM_LAZY_CAP2_ENVS", raising=False)
        else:
            monkeypatch.setenv("LRAM_LAZY_CAP2_ENVS", cap)
        eng = Engine(spec, sd, B, device="cuda:0")
        assert eng.state_mode == "lazy"
        outs.append((_run(eng, seq), eng.export_state_tensor(2, 0).clone()))
        eng.close()
    for a, c in outs[1:]:
        assert torch.equal(a, outs[0][0]) and torch.equal(c, outs[0][1])
