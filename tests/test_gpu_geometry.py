"""GPU: every model geometry `validate_config` accepts, not only the reference's presets (4 heads, d_state 16), against the CPU
oracle (tests/geometry_cases.py: 1 / 2 / 8 heads, mLSTM head dims 16 .. 1024, the three forms of the sLSTM recurrence, Mamba
d_state 4 .. 64 with ragged channel groups and dt_rank values that are no multiple of 4).  Geometry selects the code path here --
template instances per head count, cell column slices, the sLSTM dispatch on d_model / num_heads, channels per workgroup of the
selective state update, dt_proj fused / as a GEMM / as a plain kernel -- so each case runs: step parity on two weight
distributions, the lazy matrix memory where the head dim allows it (a refusal where not), stored contexts through encoder_step
and prefill, and the path switches of the sLSTM block and of dt_proj against each other.

Bars are the project's fixed ones: embedded tokens 1e-5, hidden and state 2e-4 (helpers.rel_err), C and n per element within
ELEM_STATE_TOL, continuous actions within 1e-4 and discrete ones exact, ZERO ties (seeds chosen on the CPU so that the oracle's
own top-2 logit gap never drops below 1e-3) and never the fp64 rule (cond_aware stays False: the fp32 oracle is within 7e-5 of
its float64 evaluation on the worst of these cases)."""
import pytest
import torch

from lram_amd import init_state_dict
from oracle import dt_ref, mamba_ref, xlstm_ref
from tests.geometry_cases import (ALL_CASES, BIG_CASES, BIG_SEEDS, CONTEXT_SEEDS, DISCRETE_SEEDS, MAMBA_CASES, STEP_SEEDS, STEP_STEPS,
                                  XLSTM_CASES, case_spec, step_batch)
from tests.helpers import (ELEM_STATE_TOL, assert_actions_match, elem_rel_err, make_inputs, rel_err, sampled_state, state_vs_oracle)
from tests.slot_state_helpers import exported_slice, feed_as, record_layout, run_steps
from tests.test_gpu_parity import _run_parity

pytestmark = pytest.mark.gpu

LAZY_CASES = [c for c in XLSTM_CASES if XLSTM_CASES[c][1] % 128 == 0]
NOT_LAZY_CASES = [c for c in XLSTM_CASES if XLSTM_CASES[c][1] % 128 != 0]


def _engine(spec, sd, B):
    from lram_amd.engine import Engine
    return Engine(spec, sd, B, device="cuda:0")


def _run(eng, seq):
    acts, hids = [], []
    for obs, rtg, rew, mask in seq:
        a, _ = eng.step(obs.cuda(), rtg.cuda(), rew.cuda(), mask.cuda())
        torch.cuda.synchronize()
        acts.append(a.clone())
        hids.append(eng.taps()[1].clone())
    return torch.stack(acts), torch.stack(hids)


def _seq_tensors(seq):
    return tuple(torch.stack([x[i] for x in seq], 1).contiguous().cuda() for i in range(3))


def _oracle_run(spec, sd, seq, sample=None, discrete=False):
    """The oracle over seq (on the env slots `sample`): per step (actions, logits, hidden), and the oracle itself for its state."""
    ora = dt_ref.OraclePolicy(spec, sd)
    out = []
    for obs, rtg, rew, mask in seq:
        if sample is not None:
            obs, rtg, rew, mask = obs[sample], rtg[sample], rew[sample], mask[sample]
        a, dbg = ora.step(obs, rtg, rew, mask, discrete=discrete, return_debug=True)
        out.append((a, dbg["logits"], dbg["hidden"]))
    return out, ora


# ---------------------------------------------------------------------------------------------------------------------
# 1. step parity, two weight distributions; the discrete head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["exercise", "trained_like"])
@pytest.mark.parametrize("cid", ALL_CASES)
def test_step_parity_against_the_oracle(hip_lib, cid, scheme):
    """8 env-steps with random restarts at a batch that is ragged against every env tile: embedded tokens, hidden states, actions
    and the final recurrent state (C and n per element too) against the fp32 oracle at the fixed bars, no fp64 rule, no ties."""
    seed, gap = STEP_SEEDS[(cid, scheme)]
    assert gap >= 1e-3
    assert _run_parity(f"{cid}/{scheme}", B=step_batch(cid), steps=STEP_STEPS, seed=seed, spec=case_spec(cid), scheme=scheme,
                       cond_aware=False) == 0


@pytest.mark.parametrize("cid", list(DISCRETE_SEEDS))
def test_discrete_head(hip_lib, cid):
    seed, gap = DISCRETE_SEEDS[cid]
    assert gap >= 1e-3
    assert _run_parity(f"{cid}/discrete", B=7, steps=STEP_STEPS, seed=seed, spec=case_spec(cid), discrete=True) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. lazy matrix memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,micro", [(c, 1) for c in LAZY_CASES] + [("nh1_dh128", 2), ("nh8_dh128", 2)])
def test_lazy_matrix_memory_matches_materialised_and_the_oracle(hip_lib, cid, micro):
    """The step-parity trajectory with a fold period of 3 (every env folds two or three times in 8 steps) against the materialised
    mode and the oracle at the bars of tests/test_gpu_lazy.py; after the last step windows still hold tokens (lazy_peek), and the
    export that folds them gives the oracle's C.  micro = 2: two env slices, so the fold tail runs -- with 1 and 8 heads."""
    spec = case_spec(cid)
    seed, _ = STEP_SEEDS[(cid, "exercise")]
    sd = init_state_dict(spec, seed=seed)
    B = step_batch(cid)
    seq = make_inputs(spec, B, STEP_STEPS, seed=1234 + seed, reset_prob=0.15)
    eager, lazy = _engine(spec, sd, B), _engine(spec, sd, B)
    eager.set_state_mode("eager")
    lazy.set_state_mode("lazy", fold_period=3)
    lazy.set_micro_batches(micro)
    assert eager.state_mode == "materialised" and lazy.state_mode == "lazy"
    (a_e, h_e), (a_l, h_l) = _run(eager, seq), _run(lazy, seq)
    ref, ora = _oracle_run(spec, sd, seq)
    ties = 0
    for t, (a_ref, logits, hidden) in enumerate(ref):
        ties += assert_actions_match(a_l[t], a_ref, logits, spec, what=f"{cid} lazy step {t}")
        assert rel_err(h_l[t], hidden) < 2e-4, (cid, t, rel_err(h_l[t], hidden))
    assert ties == 0
    assert float((a_e - a_l).abs().max()) <= 1e-4
    blocks = [i for i in range(spec.n_blocks) if i not in spec.slstm_at]
    pend = lazy.lazy_peek(blocks[0], "pending")
    assert float(pend.max()) >= 3.0, "no window holds a token after the last step: the export below folds nothing"
    g = lazy.lazy_peek(blocks[-1], "g")
    assert g.shape == (B, spec.n_heads) and bool((g > 0).all()) and bool((g <= 1).all())
    for blk in blocks:
        want = ora.state[f"block_{blk}"]["mlstm_state"]
        for which in (0, 1, 2, 3):
            got = lazy.export_state_tensor(blk, which)
            assert rel_err(got, eager.export_state_tensor(blk, which)) < 2e-4, (cid, blk, which)
            if which < 3:
                assert rel_err(got, want[which]) < 2e-4, (cid, blk, which)
            if which < 2:
                assert elem_rel_err(got, want[which]) < ELEM_STATE_TOL, (cid, blk, which)
    assert float(lazy.lazy_peek(blocks[0], "pending").max()) == 0.0
    eager.close(), lazy.close()


@pytest.mark.parametrize("cid", NOT_LAZY_CASES + ["m_ds8"])
def test_lazy_mode_is_refused_where_the_head_dim_does_not_allow_it(hip_lib, cid):
    from lram_amd.engine import LramError
    spec = case_spec(cid)
    eng = _engine(spec, init_state_dict(spec, seed=0), 2)
    assert eng.state_mode == "materialised"
    with pytest.raises(LramError, match="multiple of 128"):
        eng.set_state_mode("lazy")
    assert eng.state_mode == "materialised"
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. stored contexts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(XLSTM_CASES))
def test_xlstm_encoder_step_token_counts(hip_lib, cid):
    """13 .. 64 tokens per call take the chunkwise kernels where the mLSTM head dim is a multiple of 128 (with 1, 2 and 8 heads),
    else the token-sequential ones in calls of 12 / 9 / 6 tokens; shorter calls in between use the step kernels on the same state."""
    from lram_amd.engine import LramError
    spec = case_spec(cid)
    sd = init_state_dict(spec, seed=31)
    B = 3
    eng = _engine(spec, sd, B)
    state = None
    g = torch.Generator().manual_seed(9)
    chunkwise = spec.head_dim % 128 == 0
    # without a chunkwise form lram_encoder_step takes 1..4, 6, 9 or 12 tokens per call and says so: the same token runs are
    # then fed as calls of those sizes (12, 9 and 6 all occur), and compared as the one run the oracle saw
    pieces = {63: [12, 12, 12, 12, 9, 6], 13: [12, 1], 48: [12, 12, 12, 12], 21: [12, 9]}
    if not chunkwise:
        with pytest.raises(LramError, match="tokens must be 1..4, 6, 9 or 12"):
            eng.encoder_step(torch.zeros(B, 63, spec.d_model).cuda())
    for T in (63, 13, 3, 48, 1, 21):
        x = torch.randn(B, T, spec.d_model, generator=g)
        ref, state = xlstm_ref.encoder_forward_cached(spec, sd, x, state)
        if chunkwise or T <= 4:
            out = eng.encoder_step(x.cuda())
        else:
            assert sum(pieces[T]) == T
            out, t0 = [], 0
            for n in pieces[T]:
                out.append(eng.encoder_step(x[:, t0:t0 + n].contiguous().cuda()).clone())
                t0 += n
            out = torch.cat(out, 1)
        torch.cuda.synchronize()
        assert rel_err(out, ref) < 2e-4, (cid, T, rel_err(out, ref))
    pkv = eng.export_past_key_values()
    for blk in range(spec.n_blocks):
        got, want = pkv[f"block_{blk}"], state[f"block_{blk}"]
        assert rel_err(got["conv_state"][0], want["conv_state"][0]) < 1e-5, (cid, blk)
        if blk in spec.slstm_at:
            assert rel_err(got["slstm_state"], want["slstm_state"]) < 2e-4, (cid, blk)
        else:
            for i, name in enumerate(("C", "n", "m")):
                assert rel_err(got["mlstm_state"][i], want["mlstm_state"][i]) < 2e-4, (cid, blk, name)
    eng.close()


@pytest.mark.parametrize("cid", list(MAMBA_CASES))
def test_mamba_encoder_step_token_counts(hip_lib, cid):
    spec = case_spec(cid)
    sd = init_state_dict(spec, seed=3)
    B = 5
    eng = _engine(spec, sd, B)
    state = None
    g = torch.Generator().manual_seed(4)
    for T in (1, 4, 2, 3, 12, 6, 9):
        x = torch.randn(B, T, spec.d_model, generator=g)
        ref, state = mamba_ref.encoder_forward_cached(spec, sd, x, state)
        out = eng.encoder_step(x.cuda())
        torch.cuda.synchronize()
        assert rel_err(out, ref) < 2e-4, (cid, T, rel_err(out, ref))
    pkv = eng.export_past_key_values()
    for i in range(spec.n_blocks):
        assert rel_err(pkv[i][0], state[i][0]) < 2e-4 and rel_err(pkv[i][1], state[i][1]) < 2e-4, (cid, i)
    eng.close()


@pytest.mark.parametrize("cid", ALL_CASES)
def test_prefill_equals_oracle_steps(hip_lib, cid):
    """lram_prefill of L timesteps against L oracle steps: actions of the last timestep and every state tensor.  xLSTM: L = 21 is one
    63-token chunk, L = 5 fifteen tokens (12 + 3 on the token-sequential kernels where the head dim is no multiple of 128).
    Mamba: L = 9, which makes 12-token passes, and L = 5."""
    spec = case_spec(cid)
    seed, gap = CONTEXT_SEEDS[cid]
    assert gap >= 1e-3
    sd = init_state_dict(spec, seed=seed)
    B = 3
    seq = make_inputs(spec, B, 21, seed=300 + seed, reset_prob=0.0)
    ref, _ = _oracle_run(spec, sd, seq)
    ones = torch.ones(B, dtype=torch.uint8).cuda()
    for L in ((21, 5) if cid in XLSTM_CASES else (9, 5, 21)):
        eng = _engine(spec, sd, B)
        obs_seq, rtg_seq, rew_seq = _seq_tensors(seq[:L])
        act, _ = eng.prefill(obs_seq, rtg_seq, rew_seq, reset_mask=ones)
        torch.cuda.synchronize()
        assert assert_actions_match(act, ref[L - 1][0], ref[L - 1][1], spec, what=f"{cid} prefill L={L}") == 0
        ora = dt_ref.OraclePolicy(spec, sd)
        for obs, rtg, rew, mask in seq[:L]:
            ora.step(obs, rtg, rew, mask)
        state_vs_oracle(eng.export_state_tensor, ora.state, spec, f"{cid} prefill L={L}")
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the forms of the sLSTM recurrence against each other
# ---------------------------------------------------------------------------------------------------------------------
# sLSTM head dim -> the forms it can take, as (name, LRAM_SLSTM_FUSED_ROWS, LRAM_SLSTM_SEQ); None = the default
SLSTM_FORMS = {
    "nh2_dh512": [("token", None, "1"), ("step", "0", "1"), ("gemm", "0", "0")],     # 256: all three
    "nh1_sdh384": [("step", None, "1"), ("gemm", None, "0")],                         # 384: no token kernel
    "nh1_dh1024": [("gemm", None, "1"), ("gemm", "0", "0")],                          # 512: neither kernel; K = 512 recurrent GEMM
    "nh8_dh16": [("gemm", None, "1"), ("gemm", "0", "0")],                            # 8: neither; K = 8 block GEMMs, nb1 = 8
}


def _set_forms(monkeypatch, rows, seq):
    if rows is None:
        monkeypatch.delenv("LRAM_SLSTM_FUSED_ROWS", raising=False)
    else:
        monkeypatch.setenv("LRAM_SLSTM_FUSED_ROWS", rows)
    monkeypatch.setenv("LRAM_SLSTM_SEQ", seq)


@pytest.mark.parametrize("cid", list(SLSTM_FORMS))
def test_slstm_forms_against_the_oracle_and_each_other(hip_lib, monkeypatch, cid):
    """Every form of the sLSTM recurrence a geometry can take -- one launch per token, one launch per step, batched block-diagonal
    GEMM + pointwise kernel -- against the oracle (the step-parity run under that setting) and against the others at the bars of
    test_slstm_token_kernel_matches_oracle_and_the_gemm_path: env-steps with restarts, two 1-token encoder calls, a 9-timestep
    prefill.  lram_slstm_counts shows that the form meant is the form that ran, and no other."""
    spec = case_spec(cid)
    seed, _ = STEP_SEEDS[(cid, "exercise")]
    B = step_batch(cid)
    forms = SLSTM_FORMS[cid]
    for name, rows, sq in forms:
        _set_forms(monkeypatch, rows, sq)
        assert _run_parity(f"{cid}/slstm-{name}", B=B, steps=STEP_STEPS, seed=seed, spec=spec) == 0
    sd = init_state_dict(spec, seed=7)
    seq = make_inputs(spec, B, 9, seed=21, reset_prob=0.2)
    x = torch.randn(B, 1, spec.d_model, generator=torch.Generator().manual_seed(3)).cuda()
    obs_seq, rtg_seq, rew_seq = _seq_tensors(seq)
    outs = []
    for name, rows, sq in forms:
        _set_forms(monkeypatch, rows, sq)
        eng = _engine(spec, sd, B)
        eng.slstm_counts(reset=True)
        acts, _ = _run(eng, seq[:5])
        n_tok = 5 * spec.tokens_per_step
        want = {"token": (n_tok, 0, 0), "step": (0, 5, 0), "gemm": (0, 0, n_tok)}[name]
        got = eng.slstm_counts(reset=True)
        assert (got["token"], got["step"], got["gemm"]) == want, (cid, name, got)
        enc = [eng.encoder_step(x).clone() for _ in range(2)]   # the second reads the h plane the first one left
        got = eng.slstm_counts(reset=True)
        assert got[name] == 2 and sum(got.values()) == 2, (cid, name, got)
        pre, _ = eng.prefill(obs_seq, rtg_seq, rew_seq)   # (27 tokens in one pass: beyond the step kernel's 4, which hands over to the GEMM form)
        torch.cuda.synchronize()
        got = eng.slstm_counts()
        assert got["token" if name == "token" else "gemm"] == 27 and sum(got.values()) == 27, (cid, name, got)
        outs.append((acts, enc, pre.clone(), eng.export_state_tensor(1, 0).clone()))
        eng.close()
    for (name, _, _), o in zip(forms[1:], outs[1:]):
        assert float((o[0] - outs[0][0]).abs().max()) <= 1e-4, (cid, name)
        for y, y0 in zip(o[1], outs[0][1]):
            assert rel_err(y, y0) < 1e-5, (cid, name, rel_err(y, y0))
        assert float((o[2] - outs[0][2]).abs().max()) <= 1e-4, (cid, name)
        assert rel_err(o[3], outs[0][3]) < 1e-5, (cid, name, rel_err(o[3], outs[0][3]))


# ---------------------------------------------------------------------------------------------------------------------
# 5. dt_proj inside the state-update kernel against dt_proj as its own launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["m_ds16_di144", "m_r128"])
def test_mamba_dt_proj_fused_against_its_own_launch(hip_lib, monkeypatch, cid):
    """LRAM_MAMBA_DT_FUSE=0 at dt_rank 5 (rows of 37 floats: neither K nor the row pitch a multiple of 4, the plain fp32 kernel)
    and at dt_rank 128 (a K = 128 GEMM): oracle parity, and the two forms agree step by step and after a 9-timestep prefill, as
    test_mamba_dt_proj_as_its_own_gemm_stays_correct holds the presets to."""
    spec = case_spec(cid)
    seed, _ = STEP_SEEDS[(cid, "exercise")]
    B = step_batch(cid)
    monkeypatch.setenv("LRAM_MAMBA_DT_FUSE", "0")
    assert _run_parity(f"{cid}/dt-unfused", B=B, steps=STEP_STEPS, seed=seed, spec=spec) == 0
    sd = init_state_dict(spec, seed=5)
    seq = make_inputs(spec, B, 9, seed=11, reset_prob=0.15)
    engines, launches = {}, {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("LRAM_MAMBA_DT_FUSE", fuse)
        engines[fuse] = _engine(spec, sd, B)
    for obs, rtg, rew, mask in seq:
        a0, _ = engines["0"].step(obs.cuda(), rtg.cuda(), rew.cuda(), mask.cuda())
        a1, _ = engines["1"].step(obs.cuda(), rtg.cuda(), rew.cuda(), mask.cuda())
        assert float((a0 - a1).abs().max()) <= 1e-4
    for fuse in ("0", "1"):
        launches[fuse] = sum(v["launches"] for v in engines[fuse].gemm_counts().values())
    if spec.dt_rank % 4 == 0:   # (as a GEMM it is counted; the plain kernel of dt_rank 5 is no GEMM launch)
        assert launches["0"] == launches["1"] + len(seq) * spec.n_blocks, launches
    else:
        assert launches["0"] == launches["1"], launches
    obs_seq, rtg_seq, rew_seq = _seq_tensors(seq)
    ones = torch.ones(B, dtype=torch.uint8).cuda()
    p0, _ = engines["0"].prefill(obs_seq, rtg_seq, rew_seq, reset_mask=ones)
    p1, _ = engines["1"].prefill(obs_seq, rtg_seq, rew_seq, reset_mask=ones)
    torch.cuda.synchronize()
    assert float((p0 - p1).abs().max()) <= 1e-4
    for blk in range(spec.n_blocks):
        for which in (0, 3):
            assert rel_err(engines["0"].export_state_tensor(blk, which), engines["1"].export_state_tensor(blk, which)) < 1e-5
    for e in engines.values():
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. two larger batches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(BIG_CASES))
def test_larger_batches_on_sampled_slots(hip_lib, cid):
    """nh8_dh128 at 520 env slots: lazy matrix memory by default, a slice past the multi-env front end's threshold (which 8 heads do
    not take) and past the sLSTM token kernel's row limit, so the recurrence runs as GEMM + pointwise kernel.  m_ds32_e3_r7 at 130
    slots in two slices of 65: 195 rows per projection, slice rows of 71 floats.  The oracle on 12 slots: first, last, both sides
    of the slice boundary."""
    B, steps, micro, sample = BIG_CASES[cid]
    seed, gap = BIG_SEEDS[cid]
    assert gap >= 1e-3
    spec = case_spec(cid)
    sd = init_state_dict(spec, seed=seed)
    seq = make_inputs(spec, B, steps, seed=1234 + seed, reset_prob=0.15)
    eng = _engine(spec, sd, B)
    eng.set_micro_batches(micro)
    if cid in XLSTM_CASES:
        assert eng.state_mode == "lazy", "the batch no longer selects the lazy matrix memory"
    acts, hids = _run(eng, seq)
    if cid in XLSTM_CASES:
        got = eng.slstm_counts()
        assert got == {"token": 0, "step": 0, "gemm": steps * spec.tokens_per_step}, got
    ref, ora = _oracle_run(spec, sd, seq, sample=torch.tensor(sample))
    ties = 0
    for t, (a_ref, logits, hidden) in enumerate(ref):
        ties += assert_actions_match(acts[t][sample], a_ref, logits, spec, what=f"{cid} B={B} step {t}")
        assert rel_err(hids[t][sample], hidden) < 2e-4, (cid, t, rel_err(hids[t][sample], hidden))
    assert ties == 0
    state_vs_oracle(sampled_state(eng, spec, sample), ora.state, spec, f"{cid} B={B}", rows=sample)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. per-slot state: the segment table follows NH, DH and d_state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["nh8_dh16", "nh2_dh128", "m_ds32_e3_r7"])
def test_slot_state_copy_save_load(hip_lib, cid):
    """Records equal the whole-batch exports tensor by tensor (record layout restated in slot_state_helpers.record_layout); a copied
    slot fed its source's inputs follows it bit for bit; records loaded into other slots of an engine of another batch size save
    back bit for bit and continue the source's trajectory bit for bit (materialised state, same kernels at both batch sizes)."""
    spec = case_spec(cid)
    sd = init_state_dict(spec, seed=71)
    B, B2 = 7, 6
    src, dst = [1, 1, 4], [0, 5, 6]
    seq = feed_as(make_inputs(spec, B, 12, seed=31, reset_prob=0.1), 6, src, dst)
    eng = _engine(spec, sd, B)
    assert eng.state_mode == "materialised"
    run_steps(eng, seq, 0, 6, taps=False)
    layout, numel = record_layout(spec)
    assert eng.slot_state_numel == numel == eng.state_bytes_per_env() // 4
    slots = [4, 1, 6]
    rec = eng.save_slots(slots)
    assert rec.shape == (3, numel)
    for block, which, shape, off in layout:
        n = 1
        for s in shape:
            n *= s
        assert torch.equal(rec[:, off:off + n], exported_slice(eng, spec, block, which, slots)), (cid, block, which)
    other = _engine(spec, sd, B2)
    other.load_slots([3, 0, 5], rec)
    assert torch.equal(other.save_slots([3, 0, 5]), rec)
    eng.copy_slots(src, dst)
    assert torch.equal(eng.save_slots([4, 1]), rec[:2]), "a copy changed its sources"
    assert torch.equal(eng.save_slots(dst), eng.save_slots(src))
    out = run_steps(eng, seq, 6, 12)
    for k in ("a", "tok", "hid", "logits"):
        for t in range(6):
            assert torch.equal(out[k][t][dst], out[k][t][src]), (cid, k, t)
    # the other engine: slots 3 / 0 continue slots 4 / 1 of the first
    seq2 = make_inputs(spec, B2, 12, seed=32, reset_prob=0.1)
    for t in range(12):
        for xa, xb in zip(seq[t], seq2[t]):
            xb[[3, 0]] = xa[[4, 1]]
    out2 = run_steps(other, seq2, 6, 12)
    for t in range(6):
        assert torch.equal(out2["a"][t][[3, 0]], out["a"][t][[4, 1]]), (cid, t)
        assert rel_err(out2["hid"][t][[3, 0]], out["hid"][t][[4, 1]]) < 1e-5, (cid, t)
    assert rel_err(other.save_slots([3, 0]), eng.save_slots([4, 1])) < 1e-5
    eng.close(), other.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. what the kernels refuse is refused at creation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_state", [12, 128])
def test_unsupported_d_state_is_refused_at_creation(hip_lib, d_state):
    from lram_amd.config import ModelSpec, engine_limits
    from lram_amd.engine import LramError
    spec = ModelSpec(backbone="mamba", kind="MDDMamba", d_model=64, n_blocks=2, d_state=d_state, state_dim=20, act_dim=4)
    assert engine_limits(spec) == [f"Mamba d_state {d_state} must be 4, 8, 16, 32 or 64"]
    with pytest.raises(LramError, match="d_state must be 4, 8, 16, 32 or 64"):
        _engine(spec, init_state_dict(spec, seed=0), 2)
