"""GPU: stored contexts of per-env length APPENDED to the state a slot holds -- Engine.prefill / Engine.score with lengths and
append=True (lram_prefill_append, lram_score_append) and the agent calls on top of them.  An env that has not started yet is
HELD: no state-writing kernel of the chunk writes a byte of its state.  Every padded input position holds NaN.

Bars: the ones tests/test_gpu_ragged.py holds stored contexts to, none tuned to the code's output --
  * restarted envs against the CPU oracle run over their own timesteps: helpers.state_vs_oracle (2e-4), block 0's conv state 1e-5;
  * continuing envs: the action against the oracle (which took the same env-steps before the context), the state against a second
    engine that took the same 5 + n_b timesteps one lram_step at a time, snapshot right after env b's own last step: rel_err < 1e-4
    per state tensor and over the save_slots record.  (Not the per-element oracle bar: test_gpu_ragged.py records why it measures
    nothing after a handful of timesteps);
  * actions: helpers.assert_actions_match with gap_tol 2e-4, the tolerated-tie count asserted 0; every oracle run first asserts,
    before the engine is consulted, that the smallest top-2 logit gap over the rows it is compared on is at least 1e-3;
  * logp against another engine run's: 2 * 2e-4 * max|logits|;
  * bit for bit wherever two engine runs share a chunk plan, and for every held slot.
Seeds (weights / inputs), chosen on the CPU for the 1e-3 gap rule alone: 16M case 41 / 5 (smallest gap 5.1e-3; the agent test uses
it too), held-slot case 43 / 13 (1.5e-2; inputs 12 leave slot 0 a gap of 9.9e-4), tiny cases 17 / 31 (1.9e-2 and 2.9e-3)."""
import ctypes

import pytest
import torch

from lram_amd import init_state_dict, preset
from lram_amd.engine import context_plan
from tests.context_cases import (DEV, EnvRef, bits, check_continued as _check_continued, check_restarted as _check_restarted,
                                 clear_margins as _clear_margins, env_slices, export_state, new_engine, same_state, stack, steps,
                                 stepping_snapshots as _stepping_snapshots, u8_mask)
from tests.helpers import assert_actions_match, make_inputs, rel_err

pytestmark = pytest.mark.gpu

LENGTHS_16M = [47, 47, 30, 30, 9, 1]
RESTART_16M = [0, 1, 0, 1, 0, 0]
PRE = 5        # env-steps ahead of the append call (16M and held-slot cases)
EXTRA = 3      # env-steps behind the contexts


_CACHE = {}


def _case16():
    """The 16M case: weights, inputs (timesteps 0 .. L - 1 the contexts, L .. L + PRE - 1 the env-steps ahead of the call, the
    EXTRA behind them the env-steps behind it) and the oracle runs, shared by the tests and never changed.
    empty[b]: env b from an empty state over its own context, then EXTRA env-steps; cont[b]: the continuing envs of RESTART_16M
    with the PRE env-steps ahead of the context."""
    if "m16" not in _CACHE:
        spec = preset("xlstm_16m")
        sd = init_state_dict(spec, seed=41)
        B, L = 6, 47
        seq = make_inputs(spec, B, L + PRE + EXTRA, seed=5, reset_prob=0.0)
        behind = range(L + PRE, L + PRE + EXTRA)
        empty = [EnvRef(spec, sd, seq, b, n, cont=behind) for b, n in enumerate(LENGTHS_16M)]
        cont = {b: EnvRef(spec, sd, seq, b, n, pre=range(L, L + PRE)) for b, n in enumerate(LENGTHS_16M) if not RESTART_16M[b]}
        _CACHE["m16"] = (spec, sd, B, L, seq, empty, cont)
    return _CACHE["m16"]


def _snaps16():
    if "snaps16" not in _CACHE:
        spec, sd, B, L, seq, _, _ = _case16()
        _CACHE["snaps16"] = _stepping_snapshots(spec, sd, B, seq, range(L, L + PRE), LENGTHS_16M, RESTART_16M, L)
    return _CACHE["snaps16"]


def _run16(entry="append", mask=RESTART_16M, **kw):
    """A fresh engine: PRE env-steps, then the 16M contexts by the append (or the ragged) entry: (engine, actions, tokens)."""
    spec, sd, B, L, seq, _, _ = _case16()
    eng = new_engine(spec, sd, B)
    for k, v in kw.items():
        getattr(eng, k)(v)
    steps(eng, seq, range(L, L + PRE))
    act, tok = eng.prefill(*stack(seq, L, LENGTHS_16M), reset_mask=u8_mask(mask), lengths=LENGTHS_16M, append=entry == "append")
    torch.cuda.synchronize()
    return eng, act.clone(), tok.clone()


def _default16():
    """The default engine's result (chunk lanes on), kept for the tests that compare another configuration with it."""
    if "default16" not in _CACHE:
        spec = _case16()[0]
        eng, act, tok = _run16()
        _CACHE["default16"] = (act.cpu(), tok.cpu(), [t.cpu() for t in export_state(eng, spec)])
        eng.close()
    return _CACHE["default16"]


def _check16(eng, act, what):
    spec, sd, B, L, seq, empty, cont = _case16()
    snaps = _snaps16()
    for b in range(B):
        if RESTART_16M[b]:
            _check_restarted(eng, spec, b, act.cpu(), empty[b], what)
        else:
            _check_continued(eng, spec, b, act.cpu(), cont[b], snaps[b], what)


# ---- 1. appended contexts, chunkwise kernels -------------------------------------------------------------------------------------
def test_appended_contexts_continue_or_restart_each_env(hip_lib):
    spec, sd, B, L, seq, empty, cont = _case16()
    _clear_margins([empty[b] for b in range(B) if RESTART_16M[b]] + list(cont.values()), "16M append")
    assert context_plan(L, LENGTHS_16M, 16) == [0, 9, 17, 28, 38, 46]
    eng, act, tok = _run16()
    assert bool(act.isfinite().all()) and bool((tok >= 0).all())
    for t in export_state(eng, spec):
        assert bool(t.isfinite().all())
    _check16(eng, act, "16M append")
    eng.close()


# ---- 2. bit identities -----------------------------------------------------------------------------------------------------------
def test_full_lengths_are_bit_identical_to_prefill(hip_lib):
    spec, sd, B, L, seq, _, _ = _case16()
    inputs = stack(seq, L)
    e_dense, e_app = new_engine(spec, sd, B), new_engine(spec, sd, B)
    for rep in range(2):     # the second call continues (no reset)
        mask = u8_mask([1] * B) if rep == 0 else None
        a_d, t_d = e_dense.prefill(*inputs, reset_mask=mask)
        a_a, t_a = e_app.prefill(*inputs, reset_mask=mask, lengths=[L] * B, append=True)
        torch.cuda.synchronize()
        assert torch.equal(bits(a_d), bits(a_a)) and torch.equal(t_d, t_a), rep
        same_state(export_state(e_dense, spec), export_state(e_app, spec), f"full lengths, call {rep}")
    e_dense.close(), e_app.close()


def test_restarting_everybody_is_bit_identical_to_the_ragged_entry(hip_lib):
    """All-ones mask: every env with a context restarts at its own first timestep, which is what lram_prefill_ragged does to it --
    the same chunk plan, the same arithmetic per env; the held envs of a chunk only lose their state writes.
    (On this plan.  Where a chunk of ONE timestep holds an env -- the token-sequential kernels with a stretch of 4 k + 1 timesteps
    ahead of a start -- the held form is a few ulp off the zero-fed one: DESIGN.md section 9, profiles/context_call_digests.txt.)"""
    spec, sd, B, L, seq, _, _ = _case16()
    e_app, a_app, t_app = _run16("append", [1] * B)
    e_rag, a_rag, t_rag = _run16("ragged", [1] * B)
    assert torch.equal(bits(a_app), bits(a_rag)) and torch.equal(t_app, t_rag)
    same_state(export_state(e_app, spec), export_state(e_rag, spec), "append with an all-ones mask against the ragged entry")
    e_app.close(), e_rag.close()


def test_one_chunk_at_a_time_equals_the_chunk_lanes(hip_lib, monkeypatch):
    spec = _case16()[0]
    a0, t0, s0 = _default16()
    monkeypatch.setenv("LRAM_PREFILL_CHUNK", "3")
    eng, act, tok = _run16()
    monkeypatch.delenv("LRAM_PREFILL_CHUNK")
    assert torch.equal(bits(act.cpu()), bits(a0)) and torch.equal(tok.cpu(), t0)
    same_state([t.cpu() for t in export_state(eng, spec)], s0, "lanes against one chunk at a time")
    eng.close()


def test_two_env_slices_equal_one(hip_lib):
    """set_micro_batches(2) at 6 envs, on the shapes test_gpu_ragged.py uses for the same identity (13 timesteps, lengths 13, 13,
    8, 8, 3, 1: every projection of both runs is served by the few-row kernel, whose rows do not depend on their number).  Two
    calls: the second appends to a state that is not empty and restarts two envs."""
    spec, sd, B, L, seq, _, _ = _case16()
    Ls, lengths = 13, [13, 13, 8, 8, 3, 1]
    assert context_plan(Ls, lengths, 13) == [0, 5, 10, 12]
    out = []
    for micro in (1, 2):
        eng = new_engine(spec, sd, B)
        eng.set_micro_batches(micro)
        for mask in ([1] * B, RESTART_16M):
            act, tok = eng.prefill(*stack(seq, Ls, lengths), reset_mask=u8_mask(mask), lengths=lengths, append=True)
        torch.cuda.synchronize()
        out.append((act.cpu(), tok.cpu(), [t.cpu() for t in export_state(eng, spec)]))
        eng.close()
    assert torch.equal(bits(out[0][0]), bits(out[1][0])) and torch.equal(out[0][1], out[1][1])
    same_state(out[0][2], out[1][2], "two env slices against one")


# ---- 3. held slots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "lazy"])
def test_held_slots_keep_every_byte_of_their_state(hip_lib, mode):
    """5 env-steps, export, an append call with lengths 0, 12, 0, 5 and the mask 1, 1, 0, 0: slots 0 and 2 are held in every chunk
    -- bit for bit what they were in every exported tensor and in their records, whatever slot 0's reset flag says (in lazy mode
    against the export taken after the same fold: the first export folds); slot 1 restarts, slot 3 continues; one more env-step of
    all four follows the oracle.  A state writer without the hold rule shows here."""
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=43)
    B, L, lengths, restart = 4, 12, [0, 12, 0, 5], [1, 1, 0, 0]
    seq = make_inputs(spec, B, L + PRE + 1, seed=13, reset_prob=0.0)
    pre, behind = range(L, L + PRE), [L + PRE]
    if "held" not in _CACHE:
        _CACHE["held"] = [EnvRef(spec, sd, seq, b, n, pre=() if (restart[b] and n) else pre, cont=behind) for b, n in enumerate(lengths)]
    refs = _CACHE["held"]
    _clear_margins(refs, f"held slots ({mode})")
    snaps = _stepping_snapshots(spec, sd, B, seq, pre, lengths, [0, 1, 0, 0], L)
    eng = new_engine(spec, sd, B)
    if mode == "lazy":
        eng.set_state_mode("lazy")
    assert eng.state_mode == ("lazy" if mode == "lazy" else "materialised")
    steps(eng, seq, pre)
    before = {b: (env_slices(eng, spec, b), eng.save_slots([b]).cpu()) for b in (0, 2)}
    act, tok = eng.prefill(*stack(seq, L, lengths), reset_mask=u8_mask(restart), lengths=lengths, append=True)
    torch.cuda.synchronize()
    act, tok = act.clone(), tok.clone()
    for b in (0, 2):
        for i, (x, y) in enumerate(zip(before[b][0], env_slices(eng, spec, b))):
            assert torch.equal(bits(x), bits(y)), (mode, b, i)
        assert torch.equal(bits(before[b][1]), bits(eng.save_slots([b]).cpu())), (mode, b)
        assert bool((act[b] == 0).all()) and bool((tok[b] == -1).all()), (mode, b)
    assert assert_actions_match(act[1:2].cpu(), refs[1].act, refs[1].logits, spec, what=f"held slots ({mode}) env 1") == 0
    _check_continued(eng, spec, 1, None, refs[1], snaps[1], f"held slots ({mode})")
    _check_continued(eng, spec, 3, act.cpu(), refs[3], snaps[3], f"held slots ({mode})")
    assert eng.state_mode == ("lazy" if mode == "lazy" else "materialised")
    a_next, _ = eng.step(*(x.to(DEV) for x in seq[L + PRE][:3]), None)
    torch.cuda.synchronize()
    for b in range(B):
        act_ref, lg_ref = refs[b].cont[-1]
        assert assert_actions_match(a_next[b:b + 1].cpu(), act_ref, lg_ref, spec, what=f"step behind the call ({mode}) env {b}") == 0
    eng.close()


# ---- 4. token-sequential kernels -------------------------------------------------------------------------------------------------
def test_appended_contexts_through_the_token_sequential_kernels_16m(hip_lib, monkeypatch):
    """LRAM_PREFILL_CHUNK=0: chunks of at most 4 timesteps through the token-sequential kernels (16 chunks here)."""
    spec, sd, B, L, seq, empty, cont = _case16()
    _clear_margins([empty[b] for b in range(B) if RESTART_16M[b]] + list(cont.values()), "16M append, token-sequential")
    monkeypatch.setenv("LRAM_PREFILL_CHUNK", "0")
    eng, act, tok = _run16()
    monkeypatch.delenv("LRAM_PREFILL_CHUNK")
    _check16(eng, act, "16M append, LRAM_PREFILL_CHUNK=0")
    eng.close()


@pytest.mark.parametrize("name", ["xlstm_tiny", "mamba_tiny"])
def test_appended_contexts_on_the_token_sequential_geometries(hip_lib, name):
    """Head dim 64 (no chunkwise form) and Mamba, 3 env-steps first: 11 timesteps, lengths 11, 7, 0, 3, 1 (plan [0, 4, 8, 10]),
    envs 0 and 3 restart, 1 and 4 continue, 2 is held throughout."""
    spec = preset(name)
    sd = init_state_dict(spec, seed=17)
    B, L, lengths, restart, npre = 5, 11, [11, 7, 0, 3, 1], [1, 0, 0, 1, 0], 3
    assert context_plan(L, lengths, 4) == [0, 4, 8, 10]
    seq = make_inputs(spec, B, L + npre, seed=31, reset_prob=0.0)
    pre = range(L, L + npre)
    refs = [EnvRef(spec, sd, seq, b, n, pre=() if restart[b] else pre) for b, n in enumerate(lengths)]
    _clear_margins(refs, f"{name} append")
    snaps = _stepping_snapshots(spec, sd, B, seq, pre, lengths, restart, L)
    eng = new_engine(spec, sd, B)
    steps(eng, seq, pre)
    held = (env_slices(eng, spec, 2), eng.save_slots([2]).cpu())
    act, tok = eng.prefill(*stack(seq, L, lengths), reset_mask=u8_mask(restart), lengths=lengths, append=True)
    torch.cuda.synchronize()
    act, tok = act.clone(), tok.clone()
    assert bool(act.isfinite().all())
    for b, n in enumerate(lengths):
        if n == 0:
            for i, (x, y) in enumerate(zip(held[0], env_slices(eng, spec, b))):
                assert torch.equal(bits(x), bits(y)), (name, i)
            assert torch.equal(bits(held[1]), bits(eng.save_slots([b]).cpu()))
            assert bool((act[b] == 0).all()) and bool((tok[b] == -1).all())
        elif restart[b]:
            _check_restarted(eng, spec, b, act.cpu(), refs[b], f"{name} append")
        else:
            _check_continued(eng, spec, b, act.cpu(), refs[b], snaps[b], f"{name} append")
    eng.close()


# ---- 5. score --------------------------------------------------------------------------------------------------------------------
def test_score_in_two_appended_windows_against_one_ragged_call(hip_lib):
    """The 16M lengths scored as 24 + 23 timesteps (the second call appends) against one lram_score_ragged call over 47."""
    spec, sd, B, L, seq, _, _ = _case16()
    A, W = spec.act_dim, 24
    obs, rtg, rew = stack(seq, L, LENGTHS_16M)
    g = torch.Generator().manual_seed(3)
    target = (torch.rand(B, L, A, generator=g) * 2 - 1).to(DEV)
    e_one, e_win = new_engine(spec, sd, B), new_engine(spec, sd, B)
    one = e_one.score(obs, rtg, rew, actions=target, reset_mask=u8_mask([1] * B), logits=True, lengths=LENGTHS_16M)
    parts = []
    for lo, hi in ((0, W), (W, L)):
        n = [min(max(x - lo, 0), hi - lo) for x in LENGTHS_16M]
        parts.append(e_win.score(obs[:, lo:hi].contiguous(), rtg[:, lo:hi].contiguous(), rew[:, lo:hi].contiguous(),
                                 actions=target[:, lo:hi].contiguous(), reset_mask=u8_mask([1] * B) if lo == 0 else None, lengths=n,
                                 append=True))
    torch.cuda.synchronize()
    tokens, logp, actions = (torch.cat([getattr(p, k) for p in parts], 1).cpu() for k in ("tokens", "logp", "actions"))
    assert torch.equal(tokens, one.tokens.cpu())
    for b, n in enumerate(LENGTHS_16M):
        assert bool((tokens[b, n:] == -1).all()) and bool((logp[b, n:] == 0).all()) and bool((actions[b, n:] == 0).all()), b
        bar = 2 * 2e-4 * float(one.logits[b, :n].abs().max())
        err = float((logp[b, :n].double() - one.logp[b, :n].cpu().double()).abs().max())
        print(f"[append] score env {b} (n = {n}): logp of two windows off the single call's by {err:.2e} (bar {bar:.2e})")
        assert bool(logp[b, :n].isfinite().all()) and err <= bar, (b, err, bar)
    for i, (got, want) in enumerate(zip(export_state(e_win, spec), export_state(e_one, spec))):
        assert rel_err(got, want) < 1e-4, i
    e_one.close(), e_win.close()


def test_agent_scores_in_windows_or_extends_contexts_and_continues(hip_lib):
    """RecurrentAgent.score_trajectories(window=24) over the 16M lengths, and extend_contexts in two calls over the same rows: both
    agents then follow the oracle (every env from an empty state over its own timesteps) through 3 env-steps."""
    from lram_amd.agent import RecurrentAgent
    spec, sd, B, L, seq, empty, _ = _case16()
    _clear_margins(empty, "agent, 16M")
    obs, rtg, _ = (x.cpu() for x in stack(seq, L, LENGTHS_16M))
    a_win = RecurrentAgent(spec, sd, n_envs=B, device=DEV)
    a_ext = RecurrentAgent(spec, sd, n_envs=B, device=DEV)
    g = torch.Generator().manual_seed(3)
    rec = torch.rand(B, L, spec.act_dim, generator=g) * 2 - 1
    res = a_win.score_trajectories(obs, rtg, actions=rec, lengths=LENGTHS_16M, window=24)
    assert res.tokens.shape == (B, L, spec.act_dim)
    last = None
    for lo, hi in ((0, 24), (24, L)):
        n = [min(max(x - lo, 0), hi - lo) for x in LENGTHS_16M]
        act = a_ext.extend_contexts(obs[:, lo:hi], rtg[:, lo:hi], lengths=n, restart=[lo == 0] * B, want_action=True).clone()
        last = act if last is None else torch.where(torch.tensor(n, device=DEV).view(B, 1) > 0, act, last)
    torch.cuda.synchronize()
    for b, n in enumerate(LENGTHS_16M):
        assert bool((res.tokens[b, n:] == -1).all()) and bool(res.logp[b, :n].isfinite().all()), b
        # the action at env b's own last timestep, by both routes, against the oracle
        assert assert_actions_match(res.actions[b, n - 1:n].cpu(), empty[b].act, empty[b].logits, spec, what=f"windowed score env {b}") == 0
        assert assert_actions_match(last[b:b + 1].cpu(), empty[b].act, empty[b].logits, spec, what=f"extend_contexts env {b}") == 0
    for k in range(EXTRA):
        o, r = seq[L + PRE + k][0], seq[L + PRE + k][1]
        for agent, what in ((a_win, "windowed score"), (a_ext, "extend_contexts")):
            act = agent.predict_batch(o, r).clone()
            torch.cuda.synchronize()
            for b in range(B):
                assert assert_actions_match(act[b:b + 1].cpu(), *empty[b].cont[k], spec, what=f"{what}, step {k}, env {b}") == 0
    a_win.engine.close(), a_ext.engine.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refused_calls_name_the_entry_and_leave_the_state_alone(hip_lib):
    from lram_amd.engine import _ptr, _stream_ptr
    spec = preset("mamba_tiny")
    sd = init_state_dict(spec, seed=17)
    B, L = 5, 47
    seq = make_inputs(spec, B, L, seed=31, reset_prob=0.0)
    eng = new_engine(spec, sd, B)
    inputs = stack(seq, L)
    ones = u8_mask([1] * B)
    eng.prefill(*inputs, reset_mask=ones, want_action=False)     # a state that is not empty
    good = [47, 30, 0, 9, 1]
    logp = torch.zeros(B, L, spec.act_dim, device=DEV)
    tokens = torch.zeros(B, L, spec.act_dim, dtype=torch.int32, device=DEV)

    def call_prefill(lengths):
        arr = (ctypes.c_int32 * B)(*lengths) if lengths is not None else None
        return eng.lib.lram_prefill_append(eng._h, _ptr(inputs[0]), 0, _ptr(inputs[1]), _ptr(inputs[2]), L, arr, _ptr(ones), 0,
                                           _ptr(eng._actions), _ptr(eng._tokens), _stream_ptr(eng.device))

    def call_score(lengths):
        arr = (ctypes.c_int32 * B)(*lengths) if lengths is not None else None
        return eng.lib.lram_score_append(eng._h, _ptr(inputs[0]), 0, _ptr(inputs[1]), _ptr(inputs[2]), L, arr, _ptr(ones), 0, None,
                                         _ptr(tokens), None, 0, 1.0, None, None, _ptr(logp), None, _stream_ptr(eng.device))

    def refused(lengths, *needles):
        for call, entry in ((call_prefill, "lram_prefill_append"), (call_score, "lram_score_append")):
            before = eng.save_slots(list(range(B))).clone()
            torch.cuda.synchronize()
            assert call(lengths) != 0
            msg = eng.lib.lram_last_error().decode()
            assert entry in msg and all(n in msg for n in needles), msg
            after = eng.save_slots(list(range(B)))
            torch.cuda.synchronize()
            assert torch.equal(bits(before), bits(after)), msg

    refused([47, 48, 0, 9, 1], "outside 0 .. timesteps")       # a length of 48
    refused([47, -1, 0, 9, 1], "outside 0 .. timesteps")
    refused([0] * B, "every length is 0")
    refused(None, "host_lengths is NULL")
    for kw, needle in ((dict(mamba_repeat=2), "mamba_repeat"), (dict(stale_state=True), "stale_state")):
        eng.set_compat_mode(**kw)
        refused(good, needle)
        eng.set_compat_mode()
    eng.set_live(3)                                             # parked slots
    refused(good, "parked")
    eng.set_live(B)
    # ... and the engine takes the same call afterwards
    assert call_prefill(good) == 0 and call_score(good) == 0
    torch.cuda.synchronize()
    eng.close()
