"""GPU: appended contexts (Engine.prefill with lengths and append=True: lram_prefill_append) at every model geometry, block
layout, sLSTM form and env count at which a launcher picks another HOLD instance of a state-writing kernel.  tests/test_gpu_append.py
runs the hold rule on three models (xlstm_16m, xlstm_tiny, mamba_tiny) at up to 6 envs; the instances chosen by head count, head
dim, env count, sLSTM head dim, d_state and tokens per launch are run here, by ONE call per case (tests/append_cases.py): 21
timesteps, lengths 0, 21, 14, 8, 3, 1, 0 and the reset mask 1, 1, 0, 1, 0, 1, 0 after three env-steps, NaN in every padded input
position.  Slots 0 and 6 are held in every chunk (slot 0's reset flag must be ignored), 1, 3, 5 restart, 2, 4 continue.

Per case, at the bars of tests/test_gpu_append.py (none tuned to the code under test):
  * first, before the engine is consulted: the oracle's smallest top-2 logit gap over every compared row is at least 1e-3;
  * the chunk plan of the call is the one the case is there for (append_cases.PLAN_4 / PLAN_21);
  * held slots: every exported tensor and the save_slots record bit for bit what they were, action row 0, tokens -1;
  * restarted slots against the oracle from an empty state: action with no tie tolerated, helpers.state_vs_oracle (2e-4), block
    0's conv state 1e-5;
  * continuing slots: action against the oracle, state against a stepping engine's snapshot right after that env's own last step,
    rel_err < 1e-4 per tensor and over the record;
  * the env-step behind the call: every slot's action against the oracle, the held slots' too;
  * isolation under hold: a second engine whose two held slots were fed NaN observations in the env-steps ahead of the call (their
    state is non-finite) runs the same call: the live slots end bit-identical to the first engine's -- actions, tokens, every state
    tensor -- and the held slots' bytes are unchanged, NaN payloads included.  A third engine has the three restarting slots fed
    NaN as well: a restart discards the state it finds, so the same identities hold.
With more than 7 env slots the oracle and the stepping engine are consulted on sampled slots (append_cases.sampled_slots); the
bit-level checks cover every slot."""
import pytest
import torch

from lram_amd.engine import context_plan
from tests import append_cases as ac
from tests.context_cases import (DEV, NAN, bits, check_continued, check_restarted, clear_margins, new_engine, stack, state_kinds,
                                 stepping_snapshots, u8_mask)
from tests.helpers import assert_actions_match

pytestmark = pytest.mark.gpu

_ORACLE, _SNAPS = {}, {}     # per case: the oracle runs and the stepping engine's snapshots, shared by every setting and never changed


def _oracle(key):
    if key not in _ORACLE:
        spec, sd, seq = ac.case_data(key)
        _ORACLE[key] = (spec, sd, seq, ac.env_refs(key, spec, sd, seq))
    return _ORACLE[key]


def _snaps(key):
    """The stepping engine (default settings) over the case's inputs: the continuing sampled slots' states."""
    if key not in _SNAPS:
        spec, sd, seq, _ = _oracle(key)
        B = ac.case_batch(key)
        n, r = ac.lengths(B), ac.restart(B)
        only = [b for b in ac.sampled_slots(key) if n[b] and not r[b]]
        _SNAPS[key] = stepping_snapshots(spec, sd, B, seq, ac.PRE, n, r, ac.L, only=only)
    return _SNAPS[key]


def _rows(eng, spec, idx):
    """The rows `idx` of every exported state tensor, env slot on axis 0, and the slots' records: on the host."""
    ix = torch.as_tensor(idx, device=DEV)
    out = []
    for blk in range(spec.n_blocks):
        for w in state_kinds(spec, blk):
            t = eng.export_state_tensor(blk, w)
            slstm = spec.backbone == "xlstm" and blk in spec.slstm_at and w == 0     # [4, B, D]
            out.append((t[:, ix].transpose(0, 1) if slstm else t[ix]).contiguous().clone())
    out.append(eng.save_slots(list(idx)).clone())
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _same_bits(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(bits(x), bits(y)), f"{what}: state tensor {i} (the last one is the save_slots record) differs"


def _settings(monkeypatch, env):
    for k in ("LRAM_PREFILL_CHUNK", "LRAM_SLSTM_FUSED_ROWS", "LRAM_SLSTM_SEQ"):
        if env.get(k) is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, env[k])


def expected_slstm_counts(spec, plan, form):
    """Launches per form of the sLSTM recurrence over the call's chunks: the token kernel one per token, the step kernel one per
    pass of up to 4 tokens -- here the one-timestep chunk alone; longer passes hand over to the recurrent GEMM + pointwise kernel,
    one launch per token."""
    want = {"token": 0, "step": 0, "gemm": 0}
    for n in (b - a for a, b in zip(plan, plan[1:] + [ac.L])):
        T = n * spec.tokens_per_step
        if form == "token":
            want["token"] += T
        elif form == "step" and T <= 4:
            want["step"] += 1
        else:
            want["gemm"] += T
    return {k: v * len(spec.slstm_at) for k, v in want.items()}


def _append_run(key, eng, poisoned):
    """PRE env-steps (poisoned: the slots that are fed NaN observations in them, or None), then the call.  Returns the held slots'
    state before and after the call, the live slots' state after it, actions and tokens (host)."""
    spec, sd, seq, _ = _oracle(key)
    B = ac.case_batch(key)
    n, r = ac.lengths(B), ac.restart(B)
    held = [b for b in range(B) if n[b] == 0]
    live = [b for b in range(B) if n[b] > 0]
    eng.gemm_counts(reset=True)     # (over the env-steps and the call: what decides whether two slicings can agree bit for bit)
    for t in ac.PRE:
        obs, rtg, rew = (x.clone() for x in seq[t][:3])
        if poisoned:
            obs[poisoned] = NAN
        eng.step(obs.to(DEV), rtg.to(DEV), rew.to(DEV), None)
    before = _rows(eng, spec, held)
    poison_rec = eng.save_slots(poisoned).cpu() if poisoned else None
    eng.slstm_counts(reset=True)
    act, tok = eng.prefill(*stack(seq, ac.L, n), reset_mask=u8_mask(r), lengths=n, append=True)
    torch.cuda.synchronize()
    return dict(held=held, live=live, before=before, after=_rows(eng, spec, held), state=_rows(eng, spec, live), act=act.cpu().clone(),
                tok=tok.cpu().clone(), slstm=eng.slstm_counts(), gemm=eng.gemm_counts(), poisoned=poisoned, poison_rec=poison_rec)


def _check_held(run, what):
    _same_bits(run["before"], run["after"], f"{what}: held slots")
    for b in run["held"]:
        assert bool((run["act"][b] == 0).all()) and bool((run["tok"][b] == -1).all()), (what, b)


def _check_slots(key, eng, run, what):
    """The per-slot bars on the sampled slots, then the env-step behind the call on the same slots (the held ones too)."""
    spec, sd, seq, refs = _oracle(key)
    B = ac.case_batch(key)
    n, r = ac.lengths(B), ac.restart(B)
    snaps = _snaps(key)
    assert bool(run["act"].isfinite().all())
    for b in ac.sampled_slots(key):
        if n[b] == 0:
            continue
        assert bool((run["tok"][b] >= 0).all()), (what, b)
        if r[b]:
            check_restarted(eng, spec, b, run["act"], refs[b], what)
        else:
            check_continued(eng, spec, b, run["act"], refs[b], snaps[b], what)
    a_next, _ = eng.step(*(x.to(DEV) for x in seq[ac.BEHIND[0]][:3]), None)
    torch.cuda.synchronize()
    a_next = a_next.cpu()
    for b in ac.sampled_slots(key):
        act_ref, lg_ref = refs[b].cont[-1]
        assert assert_actions_match(a_next[b:b + 1], act_ref, lg_ref, spec, what=f"{what}: step behind the call, env {b}") == 0


def _run_case(monkeypatch, key, env=None, form=None, micro=None, isolation=True, per_slot=True):
    """One case under one setting: every check of the module's docstring.  Returns the first engine's run."""
    env = env or {}
    spec, sd, seq, refs = _oracle(key)
    what = key + "".join(f" {k[5:]}={v}" for k, v in env.items() if v is not None) + (f" micro={micro}" if micro else "")
    clear_margins(list(refs.values()), what)                                  # the oracle gap first
    B = ac.case_batch(key)
    plan = ac.case_plan(key, env.get("LRAM_PREFILL_CHUNK"))
    assert context_plan(ac.L, ac.lengths(B), ac.plan_cap(key, env.get("LRAM_PREFILL_CHUNK"))) == plan
    if per_slot:
        _snaps(key)                                                           # (taken under the default settings)
    _settings(monkeypatch, env)
    eng = new_engine(spec, sd, B)
    if micro:
        eng.set_micro_batches(micro)
    assert eng.state_mode == "materialised"
    run = _append_run(key, eng, None)
    _check_held(run, what)
    if form is not None:
        assert run["slstm"] == expected_slstm_counts(spec, plan, form), (what, form, run["slstm"])
    if per_slot:
        _check_slots(key, eng, run, what)
    eng.close()
    r = ac.restart(B)
    # isolation under hold: the held slots hold NaN; and once more with the restarting slots' states non-finite as well -- a restart
    # inside a chunk with held envs discards the state it finds, as a reset does everywhere else (tests/test_gpu_env_isolation.py)
    poisons = ((run["held"], "held slots fed NaN"), (run["held"] + [b for b in run["live"] if r[b]], "held and restarting slots fed NaN"))
    for poisoned, tag in poisons if isolation else ():
        eng = new_engine(spec, sd, B)
        if micro:
            eng.set_micro_batches(micro)
        bad = _append_run(key, eng, poisoned)
        eng.close()
        for b, rec in zip(poisoned, bad["poison_rec"]):
            assert not bool(rec.isfinite().all()), f"{what}: the NaN observations left slot {b} a finite state"
        _check_held(bad, f"{what}, {tag}")
        assert torch.equal(bits(bad["act"][run["live"]]), bits(run["act"][run["live"]])), f"{what}, {tag}: actions of the live slots"
        assert torch.equal(bad["tok"][run["live"]], run["tok"][run["live"]]), f"{what}, {tag}: tokens of the live slots"
        _same_bits(bad["state"], run["state"], f"{what}, {tag}: live slots")
    _settings(monkeypatch, {})
    return run


# ---- 1. every model geometry, default settings ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ac.gc.ALL_CASES)
def test_appended_contexts_at_every_geometry(hip_lib, monkeypatch, cid):
    """Head dims that are multiples of 128: the chunkwise kernels on chunks of 7, 6 and 5 timesteps, the token-sequential ones on
    the chunks of 2 and 1 in the same call; the others and Mamba: 12, 9, 6 and 3 tokens per launch.  Every chunk holds two envs."""
    assert ac.case_plan(cid) == (ac.PLAN_21 if cid in ac.CHUNKWISE else ac.PLAN_4)
    _run_case(monkeypatch, cid)


@pytest.mark.parametrize("chunk", [None, "0"], ids=["chunkwise", "token_sequential"])
def test_four_heads_with_two_channel_groups_per_thread(hip_lib, monkeypatch, chunk):
    """d_model 1024 with 4 heads (inner 2048: 512 channel groups for the front end's 256 threads): the 4-head HOLD instances of
    mlstm_pre_kernel / mlstm_pre_seq_kernel that the one-group-per-thread geometries (the 16M, the layouts) do not take."""
    spec = ac.case_spec("nh4_dh512")
    assert spec.n_heads == 4 and spec.inner // 4 > 256
    _run_case(monkeypatch, "nh4_dh512", env={"LRAM_PREFILL_CHUNK": chunk})


# ---- 2. the chunkwise cases on the token-sequential kernels and on the exact-fp32 chunk cell -----------------------------------------
@pytest.mark.parametrize("chunk", ["0", "2"])
@pytest.mark.parametrize("cid", ac.CHUNKWISE)
def test_chunkwise_geometries_under_the_other_prefill_forms(hip_lib, monkeypatch, cid, chunk):
    """LRAM_PREFILL_CHUNK=0: chunks of at most 4 timesteps -- every cell token count (12, 9, 6, 3) at every head count;
    LRAM_PREFILL_CHUNK=2: the chunkwise cell on the fp32-input matrix cores."""
    assert ac.case_plan(cid, chunk) == (ac.PLAN_4 if chunk == "0" else ac.PLAN_21)
    _run_case(monkeypatch, cid, env={"LRAM_PREFILL_CHUNK": chunk})


# ---- 3. the forms of the sLSTM recurrence under hold --------------------------------------------------------------------------------
# (case, form, LRAM_SLSTM_FUSED_ROWS, LRAM_SLSTM_SEQ): the switches of test_gpu_geometry.SLSTM_FORMS; the sLSTM-head-dim-128 case
# takes the step kernel once as it comes (two f16 planes) and once in its fp32 form
SLSTM_RUNS = [("nh2_dh512", "token", None, "1"), ("nh2_dh512", "step", "0", "1"), ("nh2_dh512", "gemm", "0", "0"),
              ("nh1_sdh384", "step", None, "1"), ("nh1_sdh384", "gemm", None, "0"), ("nh1_dh1024", "gemm", None, "1"),
              (ac.SLSTM_128, "step", "0", "1"), (ac.SLSTM_128, "step", "0", "2")]


@pytest.mark.parametrize("cid,form,rows,seq", SLSTM_RUNS, ids=[f"{c}-{f}-seq{s}" for c, f, _, s in SLSTM_RUNS])
def test_slstm_forms_under_hold(hip_lib, monkeypatch, cid, form, rows, seq):
    """lram_slstm_counts over the append call alone: the form meant, and no other, ran -- the step kernel on the one-timestep
    chunk only, the recurrent GEMM + pointwise kernel on every longer chunk of that setting."""
    plan = ac.case_plan(cid)
    assert plan[-1] == ac.L - 1, "no one-timestep chunk: the step kernel's held form would not run"
    want = expected_slstm_counts(ac.case_spec(cid), plan, form)
    if form == "step":
        assert want["step"] == 1 and want["gemm"] == 3 * (ac.L - 1) and want["token"] == 0
    else:
        assert want[form] == 3 * ac.L and sum(want.values()) == 3 * ac.L
    _run_case(monkeypatch, cid, env={"LRAM_SLSTM_FUSED_ROWS": rows, "LRAM_SLSTM_SEQ": seq}, form=form)


# ---- 4. block layouts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ac.LAYOUTS)
def test_appended_contexts_at_every_layout(hip_lib, monkeypatch, cid):
    """The hold flags are offset per env slice and handed on block by block: sLSTM first, last, adjacent, alternating, everywhere,
    the only block; one-block stacks of each kind.  The sLSTM blocks take the token kernel here (head dim 64, 7 envs)."""
    spec = ac.case_spec(cid)
    _run_case(monkeypatch, cid, form="token" if spec.backbone == "xlstm" else None)


# ---- 5. env counts that change the instance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["nh8_dh256@35", "nh8_dh128@35"])
def test_mlstm_cell_column_slices_of_larger_batches(hip_lib, monkeypatch, key):
    """35 envs x 8 heads = 280 (env, head) items: the token-sequential cell takes 64 lanes per row at head dim 256 and 32 at head
    dim 128 (launch_cell_t), on the chunks of 2 and 1 timesteps of the chunk-21 plan and, under LRAM_PREFILL_CHUNK=0, on all."""
    _run_case(monkeypatch, key)
    _run_case(monkeypatch, key, env={"LRAM_PREFILL_CHUNK": "0"}, isolation=False)


@pytest.mark.parametrize("seq", ["1", "2"], ids=["f16_planes", "fp32"])
def test_slstm_step_kernel_partial_workgroups(hip_lib, monkeypatch, seq):
    """37 envs under LRAM_SLSTM_FUSED_ROWS=0: the step kernel's held form with a partial last workgroup (16 envs per workgroup on
    the f16 planes, 32 in fp32), the pointwise kernel's held form on every longer chunk."""
    _run_case(monkeypatch, "pf1_nh2@37", env={"LRAM_SLSTM_FUSED_ROWS": "0", "LRAM_SLSTM_SEQ": seq}, form="step")


def test_mamba_lane_kernel_held_form(hip_lib, monkeypatch):
    """mamba_48m cut to two blocks at 70 envs: the one-timestep chunk's state update is the dt_rank-48 lane kernel (d_state 16,
    from 64 envs), with held envs and a partial wave of 8 envs."""
    key = "mamba_48m_2b@70"
    spec = ac.case_spec(key)
    assert (spec.d_state, spec.dt_rank, spec.d_inner % 64) == (16, 48, 0) and ac.case_batch(key) >= 64
    plan = ac.case_plan(key)
    assert plan[-1] == ac.L - 1 and plan == ac.PLAN_4, "no held one-timestep chunk: the lane kernel's held form would not run"
    _run_case(monkeypatch, key)


def test_two_env_slices_at_35_envs(hip_lib, monkeypatch):
    """nh8_dh256 at 35 envs with set_micro_batches(2) (slices of 18 and 17 envs: hold is offset per slice).  Bit-identical to one
    slice only where every projection of both runs is served by the few-row kernel, whose rows do not depend on their number;
    lram_gemm_counts decides.  The per-slot bars hold either way."""
    key = "nh8_dh256@35"
    one = _run_case(monkeypatch, key, isolation=False, per_slot=False)
    two = _run_case(monkeypatch, key, micro=2)
    other = {k: v["launches"] for r in (one, two) for k, v in r["gemm"].items() if k != "few_row_f32" and v["launches"]}
    print(f"[append] {key}: projection launches of one slice {one['gemm']}, of two {two['gemm']}")
    if not other:
        assert torch.equal(bits(one["act"]), bits(two["act"])) and torch.equal(one["tok"], two["tok"])
        _same_bits(one["state"], two["state"], "two env slices against one")
