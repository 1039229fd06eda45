"""GPU: stored contexts of per-env length -- Engine.prefill(lengths=...) / Engine.score(lengths=...) (lram_prefill_ragged,
lram_score_ragged) and the agent calls on top of them.  Env b's context is rows [b, :n_b] of left-aligned [B, L, ...] inputs;
every padded input position holds NaN, so anything that read one would show.

Bars, the ones the project already holds stored contexts to (none tuned to the code's output):
  * states against the CPU oracle run per env over its own n_b timesteps: helpers.state_vs_oracle (rel_err < 2e-4 per tensor, C / n
    per element), and 1e-4 engine against engine;
  * conv state: 1e-5 on block 0, whose conv input is one projection away from the tokens (the bar and the block
    test_chunkwise_encoder_step_matches_oracle holds); the conv states of deeper blocks take the 2e-4 of every other tensor;
  * actions: helpers.assert_actions_match with its gap_tol = 2e-4 tie rule against the oracle's logits;
  * logp against a dense run's: twice the allowed logit difference, 2 * 2e-4 * max|logits| (log-softmax is 2-Lipschitz);
  * whatever compares two engine runs of the same chunk plan (lanes on / off, score / prefill, one / two env slices, full lengths
    against the dense entry, kept slots before / after) is bit for bit.
The 16M case -- 47 timesteps, lengths 47, 47, 30, 30, 9, 1, chunks of at most 16 -- has the plan [0, 9, 17, 28, 38, 46]: chunkwise
chunks of 8 - 11 timesteps, a last chunk of one timestep on the token-sequential kernels (the env that starts on the last
timestep), an sLSTM block, and six chunks over the three lanes."""
import pytest
import torch

from lram_amd import init_state_dict, preset
from lram_amd.engine import LramError, context_plan
from oracle import dt_ref
from tests.context_cases import DEV, NAN, EnvRef, bits, env_slices, export_state, new_engine, same_state, stack
from tests.helpers import assert_actions_match, make_inputs, rel_err, sampled_state, state_vs_oracle

pytestmark = pytest.mark.gpu

LENGTHS_16M = [47, 47, 30, 30, 9, 1]
EXTRA = 3     # env-steps behind the contexts


def _check_env(eng, spec, b, actions, ref, what, continued=False):
    """env b of the engine against its oracle run: the action (tie rule), every state tensor, block 0's conv state at 1e-5."""
    want_state = ref.cont_state if continued else ref.state
    if actions is not None:
        act, logits = ref.cont[-1] if continued else (ref.act, ref.logits)
        assert_actions_match(actions[b:b + 1], act, logits, spec, what=f"{what} env {b}")
    export = sampled_state(eng, spec, [b])
    state_vs_oracle(export, want_state, spec, f"{what} env {b}", rows=[b])
    conv = want_state[0][0] if spec.backbone == "mamba" else want_state["block_0"]["conv_state"][0]
    err = rel_err(export(0, 3), conv)
    print(f"[ragged] {what} env {b}: block 0 conv state rel_err {err:.2e} (bar 1e-5)")
    assert err < 1e-5, (what, b, err)


_CACHE = {}


def _case16():
    """The 16M case: weights, inputs of L + EXTRA timesteps, one oracle run per env (shared by the tests, never changed)."""
    if "m16" not in _CACHE:
        spec = preset("xlstm_16m")
        sd = init_state_dict(spec, seed=41)
        B, L = 6, 47
        seq = make_inputs(spec, B, L + EXTRA, seed=5, reset_prob=0.0)
        refs = [EnvRef(spec, sd, seq, b, n, cont=range(L, L + EXTRA)) for b, n in enumerate(LENGTHS_16M)]
        _CACHE["m16"] = (spec, sd, B, L, seq, refs)
    return _CACHE["m16"]


def _run16(**kw):
    """A fresh engine's ragged prefill of the 16M case: (engine, actions, tokens), synchronised."""
    spec, sd, B, L, seq, _ = _case16()
    eng = new_engine(spec, sd, B)
    for k, v in kw.items():
        getattr(eng, k)(v)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    act, tok = eng.prefill(*stack(seq, L, LENGTHS_16M), reset_mask=ones, lengths=LENGTHS_16M)
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


# ---- 1. every env primed with its own context ------------------------------------------------------------------------------------
def test_ragged_prefill_gives_every_env_the_state_of_its_own_context(hip_lib):
    spec, sd, B, L, seq, refs = _case16()
    assert context_plan(L, LENGTHS_16M, 16) == [0, 9, 17, 28, 38, 46]
    eng, act, tok = _run16()
    assert bool(act.isfinite().all()) and bool((tok >= 0).all())
    for t in export_state(eng, spec):
        assert bool(t.isfinite().all())
    for b in range(B):
        _check_env(eng, spec, b, act.cpu(), refs[b], "16M ragged prefill")
    eng.close()


# ---- 2. full lengths: the dense entry's launches ---------------------------------------------------------------------------------
def test_full_lengths_are_bit_identical_to_prefill(hip_lib):
    spec, sd, B, L, seq, _ = _case16()
    inputs = stack(seq, L)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    e_dense, e_ragged = new_engine(spec, sd, B), new_engine(spec, sd, B)
    for rep in range(2):     # the second call continues (no reset)
        mask = ones if rep == 0 else None
        a_d, t_d = e_dense.prefill(*inputs, reset_mask=mask)
        a_r, t_r = e_ragged.prefill(*inputs, reset_mask=mask, lengths=[L] * B)
        torch.cuda.synchronize()
        assert torch.equal(bits(a_d), bits(a_r)) and torch.equal(t_d, t_r), rep
        same_state(export_state(e_dense, spec), export_state(e_ragged, spec), f"full lengths, call {rep}")
    e_dense.close(), e_ragged.close()


# ---- 3. token-sequential kernels, one chunk at a time ----------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_mode", ["0", "3"])
def test_ragged_prefill_token_sequential_and_one_chunk_at_a_time(hip_lib, monkeypatch, chunk_mode):
    """LRAM_PREFILL_CHUNK=0: chunks of at most 4 timesteps through the token-sequential kernels (16 chunks here).  =3: the default
    plan, one chunk at a time: bit-identical to the chunk lanes, the header's promise for them."""
    spec, sd, B, L, seq, refs = _case16()
    monkeypatch.setenv("LRAM_PREFILL_CHUNK", chunk_mode)
    eng, act, tok = _run16()
    monkeypatch.delenv("LRAM_PREFILL_CHUNK")
    for b in range(B):
        _check_env(eng, spec, b, act.cpu(), refs[b], f"16M ragged prefill, LRAM_PREFILL_CHUNK={chunk_mode}")
    if chunk_mode == "3":
        a0, t0, s0 = _default16()
        assert torch.equal(bits(act.cpu()), bits(a0)) and torch.equal(tok.cpu(), t0)
        same_state([t.cpu() for t in export_state(eng, spec)], s0, "lanes against one chunk at a time")
    eng.close()


# ---- 4. a rollout continues from the primed state --------------------------------------------------------------------------------
def test_steps_continue_from_the_primed_contexts(hip_lib):
    """Env 0 (full length, reset flag 0) continues the state an earlier dense prefill left -- held against an engine that took the
    same timesteps one lram_step at a time; the other envs restart, are primed, and follow their oracle through 3 env-steps."""
    spec, sd, B, L, seq, refs = _case16()
    L0 = 6
    seq0 = make_inputs(spec, B, L0, seed=77, reset_prob=0.0)
    eng, e_step = new_engine(spec, sd, B), new_engine(spec, sd, B)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    eng.prefill(*stack(seq0, L0), reset_mask=ones, want_action=False)
    mask = torch.tensor([0, 1, 1, 1, 1, 1], dtype=torch.uint8, device=DEV)
    eng.prefill(*stack(seq, L, LENGTHS_16M), reset_mask=mask, lengths=LENGTHS_16M)
    for obs, rtg, rew, _ in seq0 + seq[:L]:
        e_step.step(obs.to(DEV), rtg.to(DEV), rew.to(DEV), None)
    for k in range(EXTRA):
        obs, rtg, rew, _ = (x.to(DEV) for x in seq[L + k])
        act, _ = eng.step(obs, rtg, rew, None)
        a_step, _ = e_step.step(obs, rtg, rew, None)
        torch.cuda.synchronize()
        lg = e_step.taps()[2].view(B, spec.act_dim, spec.n_vocab).cpu()
        assert_actions_match(act[:1].cpu(), a_step[:1].cpu(), lg[:1], spec, what=f"env 0, step {k}")
        for b in range(1, B):
            assert_actions_match(act[b:b + 1].cpu(), *refs[b].cont[k], spec, what=f"env {b}, step {k}")
    for got, want in zip(env_slices(eng, spec, 0), env_slices(e_step, spec, 0)):
        assert rel_err(got, want) < 1e-4
    for b in range(1, B):
        _check_env(eng, spec, b, None, refs[b], "16M, 3 steps behind the contexts", continued=True)
    eng.close(), e_step.close()


# ---- 5. slots without a context are left alone -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "lazy"])
def test_slots_of_length_zero_keep_their_state(hip_lib, mode):
    """5 env-steps, export, a ragged call with lengths 0, 12, 0, 5, export: slots 0 and 2 are bit for bit what they were, in every
    exported tensor and in their save_slots records (in lazy mode against the export taken after the same fold: the first export
    folds), their action rows hold 0 / -1, and one more env-step of all four envs follows the oracle."""
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=43)
    B, L, pre, lengths = 4, 12, 5, [0, 12, 0, 5]
    seq = make_inputs(spec, B, L + pre + 1, seed=12, reset_prob=0.0)
    if "keep" not in _CACHE:   # the oracle: slots 0, 2 take 5 + 1 env-steps (no context), slots 1, 3 their context + 1 env-step
        _CACHE["keep"] = [EnvRef(spec, sd, seq, b, n, pre=() if n else range(L, L + pre), cont=[L + pre]) for b, n in enumerate(lengths)]
    refs = _CACHE["keep"]
    eng = new_engine(spec, sd, B)
    if mode == "lazy":
        eng.set_state_mode("lazy")
    assert eng.state_mode == ("lazy" if mode == "lazy" else "materialised")
    for t in range(L, L + pre):
        eng.step(*(x.to(DEV) for x in seq[t][:3]), None)
    before = {b: (env_slices(eng, spec, b), eng.save_slots([b]).cpu()) for b in (0, 2)}
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    act, tok = eng.prefill(*stack(seq, L, lengths), reset_mask=ones, lengths=lengths)
    torch.cuda.synchronize()
    act, tok = act.clone(), tok.clone()
    for b in (0, 2):
        for i, (x, y) in enumerate(zip(before[b][0], env_slices(eng, spec, b))):
            assert torch.equal(bits(x), bits(y)), (mode, b, i)
        assert torch.equal(bits(before[b][1]), bits(eng.save_slots([b]).cpu())), (mode, b)
        assert bool((act[b] == 0).all()) and bool((tok[b] == -1).all()), (mode, b)
    # the slots with a context: the oracle's action, and the state a dense prefill of the env's own n timesteps leaves (1e-4, the
    # engine-against-engine bar).  Not state_vs_oracle here: slot 3's 5 timesteps are one chunk in both calls -- bit-identical
    # states -- and on these inputs the dense entry itself is 8.0e-3 per element off the oracle in block 7's C (bar 5e-3;
    # 3.6e-3 by 5 lram_step calls), 2.3e-5 by rel_err: after 5 timesteps most of C is cancellation noise.
    e_dense = new_engine(spec, sd, B)
    for b in (1, 3):
        assert_actions_match(act[b:b + 1].cpu(), refs[b].act, refs[b].logits, spec, what=f"kept slots ({mode}) env {b}")
        e_dense.prefill(*stack(seq, lengths[b]), reset_mask=ones, want_action=False)
        for i, (got, want) in enumerate(zip(env_slices(eng, spec, b), env_slices(e_dense, spec, b))):
            assert rel_err(got, want) < 1e-4, (mode, b, i)
    e_dense.close()
    assert eng.state_mode == ("lazy" if mode == "lazy" else "materialised")
    a_next, _ = eng.step(*(x.to(DEV) for x in seq[L + pre][:3]), None)
    torch.cuda.synchronize()
    for b in range(B):
        act_ref, lg_ref = refs[b].cont[-1]
        assert_actions_match(a_next[b:b + 1].cpu(), act_ref, lg_ref, spec, what=f"step behind the call ({mode}) env {b}")
    eng.close()


# ---- 5b. who restarts: a shorter context whatever the mask says, a full one where the mask says so -------------------------------
@pytest.mark.parametrize("name", ["xlstm_tiny", "mamba_tiny"])
def test_shorter_contexts_restart_whatever_the_mask_says_and_full_ones_obey_it(hip_lib, name):
    """3 env-steps, then one replace call of 6 timesteps with lengths 6, 6, 3, 0 (plan [0, 3]), without a mask on one engine and
    with an all-ones mask on another.  Env 2 (shorter) restarts at its first timestep on both: bit-identical state and action.
    Envs 0 and 1 (full length) continue the 3 env-steps without a mask and start from an empty state with one.  Env 3 (length 0)
    is held on both: every exported tensor and its record bit for bit what they were."""
    spec = preset(name)
    sd = init_state_dict(spec, seed=17)
    B, L, lengths, npre = 4, 6, [6, 6, 3, 0], 3
    assert context_plan(L, lengths, 4) == [0, 3]
    seq = make_inputs(spec, B, L + npre, seed=31, reset_prob=0.0)
    pre = range(L, L + npre)
    continued = [EnvRef(spec, sd, seq, b, lengths[b], pre=pre) for b in (0, 1)]
    empty = [EnvRef(spec, sd, seq, b, lengths[b]) for b in (0, 1)]
    inputs = stack(seq, L, lengths)
    out = {}
    for kind, mask in (("no mask", None), ("all-ones mask", torch.ones(B, dtype=torch.uint8, device=DEV))):
        eng = new_engine(spec, sd, B)
        for t in pre:
            eng.step(*(x.to(DEV) for x in seq[t][:3]), None)
        before = (env_slices(eng, spec, 3), eng.save_slots([3]).cpu())
        act, tok = eng.prefill(*inputs, reset_mask=mask, lengths=lengths)
        torch.cuda.synchronize()
        act, tok = act.clone(), tok.clone()
        assert bool(act.isfinite().all())
        for i, (x, y) in enumerate(zip(before[0], env_slices(eng, spec, 3))):
            assert torch.equal(bits(x), bits(y)), (name, kind, i)
        assert torch.equal(bits(before[1]), bits(eng.save_slots([3]).cpu())), (name, kind)
        assert bool((act[3] == 0).all()) and bool((tok[3] == -1).all()), (name, kind)
        for b, ref in zip((0, 1), continued if mask is None else empty):
            _check_env(eng, spec, b, act.cpu(), ref, f"{name} replace call, {kind}")
        out[kind] = (act.cpu(), tok.cpu(), env_slices(eng, spec, 2))
        eng.close()
    (a0, t0, s0), (a1, t1, s1) = out["no mask"], out["all-ones mask"]
    assert torch.equal(bits(a0[2]), bits(a1[2])) and torch.equal(t0[2], t1[2])
    for i, (x, y) in enumerate(zip(s0, s1)):
        assert torch.equal(bits(x), bits(y)), (name, i)


# ---- 6. scores at the left-aligned rows ------------------------------------------------------------------------------------------
def test_ragged_score_against_dense_scores_per_length(hip_lib):
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=41)
    B, L, lengths = 4, 40, [40, 23, 7, 1]
    A = spec.act_dim
    seq = make_inputs(spec, B, L, seed=21, reset_prob=0.0)
    obs, rtg, rew = stack(seq, L, lengths)
    g = torch.Generator().manual_seed(3)
    target = (torch.rand(B, L, A, generator=g) * 2 - 1).to(DEV)
    valid = torch.ones(B, L, dtype=torch.uint8)
    valid[0, 3] = valid[1, 22] = valid[1, 5] = 0       # read at the left-aligned row
    valid = valid.to(DEV)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    e_score, e_pre, e_ref = (new_engine(spec, sd, B) for _ in range(3))
    res = e_score.score(obs, rtg, rew, actions=target, valid=valid, reset_mask=ones, logits=True, lengths=lengths)
    a_pre, t_pre = e_pre.prefill(obs, rtg, rew, reset_mask=ones, lengths=lengths)
    torch.cuda.synchronize()
    for out in (res.actions, res.tokens, res.logp, res.logits):
        assert bool(out.isfinite().all()) if out.is_floating_point() else True
    for b, n in enumerate(lengths):
        # rows behind the context, and the rows `valid` masks: exactly the fill values
        dead = torch.ones(L, dtype=torch.bool)
        dead[:n] = valid[b, :n].cpu() == 0
        assert bool((res.logp[b][dead] == 0).all()) and bool((res.tokens[b][dead] == -1).all()), b
        assert bool((res.actions[b][dead] == 0).all()) and bool((res.logits[b][dead] == 0).all()), b
        # the env's own rows against a dense score of its n timesteps (a clean copy of the inputs: no NaN inside [:n] of env b)
        clean = [torch.nan_to_num(x[:, :n], nan=0.0).contiguous() for x in (obs, rtg, rew)]
        ref = e_ref.score(*clean, actions=target[:, :n].contiguous(), valid=valid[:, :n].contiguous(), reset_mask=ones, logits=True)
        torch.cuda.synchronize()
        live = ~dead[:n]
        lg = ref.logits[b].cpu()
        assert_actions_match(res.actions[b, :n].cpu()[live], ref.actions[b].cpu()[live], lg[live], spec, what=f"score env {b}")
        bar = 2 * 2e-4 * float(lg[live].abs().max())
        err = float((res.logp[b, :n].cpu()[live].double() - ref.logp[b].cpu()[live].double()).abs().max())
        print(f"[ragged] score env {b} (n = {n}): logp off by {err:.2e} (bar {bar:.2e})")
        assert err <= bar, (b, err, bar)
        # the env's last timestep went through the head launches prefill(lengths=...) makes for its action
        if valid[b, n - 1]:
            assert torch.equal(bits(res.actions[b, n - 1]), bits(a_pre[b])) and torch.equal(res.tokens[b, n - 1], t_pre[b]), b
    same_state(export_state(e_score, spec), export_state(e_pre, spec), "score(lengths) against prefill(lengths)")
    for e in (e_score, e_pre, e_ref):
        e.close()


# ---- 7. geometries without a chunkwise form, Mamba, refusals ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["xlstm_tiny", "mamba_tiny"])
def test_ragged_prefill_on_the_token_sequential_geometries(hip_lib, name):
    """Head dim 64 (no chunkwise form) and Mamba: chunks of at most 4 timesteps; 11 timesteps, lengths 11, 6, 2, 1 -> the plan
    [0, 3, 5, 9, 10]."""
    spec = preset(name)
    sd = init_state_dict(spec, seed=17)
    B, L, lengths = 4, 11, [11, 6, 2, 1]
    assert context_plan(L, lengths, 4) == [0, 3, 5, 9, 10]
    seq = make_inputs(spec, B, L, seed=31, reset_prob=0.0)
    refs = [EnvRef(spec, sd, seq, b, n) for b, n in enumerate(lengths)]
    eng = new_engine(spec, sd, B)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    inputs = stack(seq, L, lengths)
    act, _ = eng.prefill(*inputs, reset_mask=ones, lengths=lengths)
    torch.cuda.synchronize()
    assert bool(act.isfinite().all())
    for b in range(B):
        _check_env(eng, spec, b, act.cpu(), refs[b], f"{name} ragged prefill")

    def refused(call, *needles):
        before = export_state(eng, spec)
        with pytest.raises(LramError) as err:
            call()
        assert all(n in str(err.value) for n in needles), str(err.value)
        same_state(before, export_state(eng, spec), str(err.value))

    if spec.backbone == "mamba":
        for kw, needle in ((dict(mamba_repeat=2), "mamba_repeat"), (dict(stale_state=True), "stale_state")):
            eng.set_compat_mode(**kw)
            refused(lambda: eng.prefill(*inputs, reset_mask=ones, lengths=lengths), "lram_prefill_ragged", needle)
            refused(lambda: eng.score(*inputs, reset_mask=ones, lengths=lengths, want=("tokens",)), "lram_score_ragged", needle)
            eng.set_compat_mode()
    # the C entry's own length rules (the Python wrapper checks them first)
    import ctypes
    from lram_amd.engine import _ptr, _stream_ptr
    for bad, needle in (([11, 12, 0, 1], "outside 0 .. timesteps"), ([11, -1, 0, 1], "outside 0 .. timesteps"), ([0, 0, 0, 0], "every length is 0")):
        arr = (ctypes.c_int32 * B)(*bad)
        rc = lambda: eng.lib.lram_prefill_ragged(eng._h, _ptr(inputs[0]), 0, _ptr(inputs[1]), _ptr(inputs[2]), L, arr, _ptr(ones), 0,
                                                 _ptr(eng._actions), _ptr(eng._tokens), _stream_ptr(eng.device))
        before = export_state(eng, spec)
        assert rc() != 0 and needle in eng.lib.lram_last_error().decode(), eng.lib.lram_last_error()
        same_state(before, export_state(eng, spec), needle)
    # ... and the engine is usable afterwards
    act2, _ = eng.prefill(*inputs, reset_mask=ones, lengths=lengths)
    torch.cuda.synchronize()
    assert torch.equal(bits(act2), bits(act))
    eng.close()


# ---- 8. two env slices -----------------------------------------------------------------------------------------------------------
def test_two_env_slices_equal_one(hip_lib):
    """set_micro_batches(2) at 6 envs.  The slices share one workspace whose row ranges move with the chunk length, and the plan's
    chunks differ in length: a missing barrier between them shows as errors of 1e-2 in the envs next to the slice boundary.
      * 13 timesteps, lengths 13, 13, 8, 8, 3, 1 (plan [0, 5, 10, 12]: chunks of 5, 5, 2, 1 timesteps, 90 / 36 / 18 operand rows on
        one slice, 45 / 18 / 9 on each of two): every projection of both runs is served by the few-row kernel (9 .. 192 rows
        whatever the weight), whose rows do not depend on their number -- bit for bit the same states, actions and tokens.
      * the 47-timestep case: its 11-timestep chunk has 198 rows on one slice, where the dispatcher hands the large weights to
        the bf16x3 kernel, and 99 on each of two (few-row kernel): another rounding, as for a dense prefill (3e-6 there).  Held
        to the oracle per env and to the one-slice run at the engine-against-engine bar of 1e-4."""
    spec, sd, B, L, seq, refs = _case16()
    a0, t0, s0 = _default16()
    eng, act, tok = _run16(set_micro_batches=2)
    for b in range(B):
        _check_env(eng, spec, b, act.cpu(), refs[b], "16M ragged prefill, two env slices")
    for i, (got, want) in enumerate(zip(export_state(eng, spec), s0)):
        assert rel_err(got, want) < 1e-4, i
    eng.close()
    Ls, lengths = 13, [13, 13, 8, 8, 3, 1]
    assert context_plan(Ls, lengths, 13) == [0, 5, 10, 12]
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    out = []
    for micro in (1, 2):
        eng = new_engine(spec, sd, B)
        eng.set_micro_batches(micro)
        for rep in range(2):    # the second call over a state that is not empty
            act, tok = eng.prefill(*stack(seq, Ls, lengths), reset_mask=ones, lengths=lengths)
        torch.cuda.synchronize()
        out.append((act.cpu(), tok.cpu(), [t.cpu() for t in export_state(eng, spec)]))
        eng.close()
    assert torch.equal(bits(out[0][0]), bits(out[1][0])) and torch.equal(out[0][1], out[1][1])
    same_state(out[0][2], out[1][2], "two env slices against one")


# ---- 9. the agent ----------------------------------------------------------------------------------------------------------------
def test_agent_scores_or_primes_contexts_and_continues(hip_lib):
    from lram_amd.agent import RecurrentAgent
    spec = preset("xlstm_tiny")
    sd = init_state_dict(spec, seed=33)
    B, L, n_obs, n_act, lengths = 3, 7, 11, 3, [7, 2, 5]
    g = torch.Generator().manual_seed(5)
    mean, std = torch.randn(spec.state_dim, generator=g) * 0.1, torch.rand(spec.state_dim, generator=g) + 0.5
    a_score = RecurrentAgent(spec, sd, n_envs=B, device=DEV, state_mean=mean, state_std=std)
    a_prime = RecurrentAgent(spec, sd, n_envs=B, device=DEV, state_mean=mean, state_std=std)
    obs = torch.rand(B, L + 1, n_obs, generator=g) * 2 - 1
    rtg = torch.full((B, L + 1), 3.0) - 0.01 * torch.arange(L + 1)
    rec = torch.rand(B, L, n_act, generator=g) * 2 - 1
    ctx_obs, ctx_rtg = obs[:, :L].clone(), rtg[:, :L].clone()
    for b, n in enumerate(lengths):
        ctx_obs[b, n:], ctx_rtg[b, n:] = NAN, NAN
    with pytest.raises(ValueError):
        a_score.score_trajectories(ctx_obs, ctx_rtg, actions=rec, lengths=lengths, reset=False)
    res = a_score.score_trajectories(ctx_obs, ctx_rtg, actions=rec, lengths=torch.tensor(lengths))
    last = a_prime.prime_contexts(ctx_obs, ctx_rtg, lengths=lengths, want_action=True)
    torch.cuda.synchronize()
    for b, n in enumerate(lengths):
        assert torch.equal(bits(res.actions[b, n - 1]), bits(last[b])), b
        assert bool((res.tokens[b, n:] == -1).all()) and bool(res.logp[b, :n, :n_act].isfinite().all()), b
    # env b's next observation is the one behind ITS context
    nxt_obs = torch.stack([obs[b, n] for b, n in enumerate(lengths)])
    nxt_rtg = torch.stack([rtg[b, n] for b, n in enumerate(lengths)])
    act_s = a_score.predict_batch(nxt_obs, nxt_rtg).clone()
    act_p = a_prime.predict_batch(nxt_obs, nxt_rtg).clone()
    torch.cuda.synchronize()
    assert torch.equal(bits(act_s), bits(act_p))
    pad = torch.zeros(B, L + 1, spec.state_dim)
    pad[..., :n_obs] = obs
    for b, n in enumerate(lengths):
        ora = dt_ref.OraclePolicy(spec, sd, state_mean=mean, state_std=std)
        for t in range(n + 1):
            a_ref, dbg = ora.step(pad[b:b + 1, t], rtg[b:b + 1, t], torch.zeros(1), return_debug=True)
        assert_actions_match(act_p[b:b + 1].cpu(), a_ref, dbg["logits"], spec, what=f"agent env {b}")
        state_vs_oracle(sampled_state(a_prime.engine, spec, [b]), ora.state, spec, f"agent env {b}", rows=[b])
    a_score.engine.close(), a_prime.engine.close()
