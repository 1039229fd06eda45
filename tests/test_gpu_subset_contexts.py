"""GPU: stored contexts on a subset of the env slots -- Engine.set_context_rows "live" and "started" (lram_set_context_rows,
lram_context_counts) on an engine that has parked slots (Engine.set_live), and RecurrentAgent.extend_contexts(envs=...) on top.

Cases (tests/subset_cases.py): the layout geometry (chunkwise, lazy-capable), xlstm_tiny (token-sequential) and mamba_tiny; 7 live
of 12 slots with the lengths 21, 14, 8, 3, 1, 0, 0 of tests/append_cases.py in slot order, 37 live of 40, 1 live of 12.  Every slot
takes three env-steps ahead of the call, the parked ones included, so a parked slot holds a state of its own.

The bars are those of tests/helpers.py and tests/context_cases.py, none tuned to the code under test: a restarted env against the
CPU oracle (action with no tie tolerated, helpers.state_vs_oracle 2e-4, block 0's conv state 1e-5), a continuing env against an
engine that steps (rel_err < 1e-4 per tensor and over the record), the env-step behind the call against the oracle; parked and
length-0 slots bit for bit (lazy mode: C of a parked slot within 2e-4 of max-abs, tests/test_gpu_live.py's bar for a fold)."""
import ctypes

import pytest
import torch

from lram_amd.engine import LramError, context_plan
from tests import subset_cases as sc
from tests.context_cases import (DEV, NAN, bits, check_continued, check_restarted, clear_margins, env_slices, new_engine, stack,
                                 state_kinds, stepping_snapshots, u8_mask)
from tests.helpers import assert_actions_match, rel_err
from tests.slot_state_helpers import record_layout

pytestmark = pytest.mark.gpu

_CASES, _SNAPS = {}, {}     # per case: data and oracle runs, the stepping engine's snapshots; shared and never changed
CASES = [(g, live, slots) for g in sc.GEOMETRIES for live, slots in sc.COUNTS]
IDS = [sc.case_key(*c) for c in CASES]


def _case(geo, live, slots):
    key = sc.case_key(geo, live, slots)
    if key not in _CASES:
        spec, sd, seq, parked = sc.case_data(geo, live, slots)
        _CASES[key] = (spec, sd, seq, parked, sc.env_refs(spec, sd, seq, live))
    return _CASES[key]


def _snaps(geo, live, slots):
    key = sc.case_key(geo, live, slots)
    if key not in _SNAPS:
        spec, sd, seq, _, _ = _case(geo, live, slots)
        n, r = sc.lengths(live), sc.restart(live)
        only = [b for b in sc.sampled_slots(live) if n[b] and not r[b]]
        _SNAPS[key] = stepping_snapshots(spec, sd, live, seq, sc.PRE, n, r, sc.L, only=only)
    return _SNAPS[key]


def _cap(spec, monkey_chunk=None):
    return 21 if (spec.backbone == "xlstm" and spec.head_dim % 128 == 0 and monkey_chunk != "0") else 4


def _primed(case, poison=(), micro=None, lazy=False):
    """An engine of `slots` slots after the env-steps ahead of the call on EVERY slot (poison: parked slots fed NaN observations),
    the first `live` slots live."""
    geo, live, slots = case
    spec, sd, seq, parked, _ = _case(*case)
    eng = new_engine(spec, sd, slots)
    if lazy:
        eng.set_state_mode("lazy")
        assert eng.state_mode == "lazy"
    else:
        assert eng.state_mode == "materialised"
    if micro:
        eng.set_micro_batches(micro)
    for t in sc.PRE:
        obs, rtg, rew = (torch.cat([a, b]) for a, b in zip(seq[t][:3], parked[t][:3]))
        for p in poison:
            obs[p] = NAN
        eng.step(obs.to(DEV), rtg.to(DEV), rew.to(DEV), None)
    if live < slots:
        eng.set_live(live)
    return eng


def _rows(eng, spec, idx):
    """The rows `idx` of every exported state tensor and the slots' records, on the host."""
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


def _call(case, eng, mode, append=True, kind="prefill", n=None, r=None):
    """One stored-context call on the live prefix under `mode`.  Returns the parked and length-0 slots' state before and after, the
    started slots' state after, actions / tokens (prefill) or the ScoreResult's tokens and actions (score), and the counts."""
    geo, live, slots = case
    spec, _, seq, _, _ = _case(*case)
    n = sc.lengths(live) if n is None else n
    r = sc.restart(live) if r is None else r
    quiet = [b for b in range(live) if n[b] == 0] + list(range(live, slots))
    started = [b for b in range(live) if n[b] > 0]
    before = _rows(eng, spec, quiet)
    eng.set_context_rows(mode)
    eng.context_counts(reset=True)
    inputs = stack(seq, sc.L, n)
    if kind == "prefill":
        act, tok = eng.prefill(*inputs, reset_mask=u8_mask(r), lengths=n, append=append)
    else:
        res = eng.score(*inputs, reset_mask=u8_mask(r), lengths=n, append=append, want=("actions", "tokens"))
        act, tok = res.actions, res.tokens
    torch.cuda.synchronize()
    assert act.shape[0] == live and tok.shape[0] == live
    out = dict(quiet=quiet, started=started, before=before, after=_rows(eng, spec, quiet), state=_rows(eng, spec, started),
               act=act.cpu().clone(), tok=tok.cpu().clone(), counts=eng.context_counts(), n=n, r=r)
    eng.set_context_rows("all")
    return out


def _last(run, b):
    """Action row of env b at its own last timestep: a prefill's row, or row n_b - 1 of a score."""
    return run["act"][b:b + 1] if run["act"].dim() == 2 else run["act"][b:b + 1, run["n"][b] - 1]


def _check_quiet(run, what):
    _same_bits(run["before"], run["after"], f"{what}: parked and length-0 slots")
    for b, nb in enumerate(run["n"]):
        if run["act"].dim() == 2:
            if nb == 0:
                assert bool((run["act"][b] == 0).all()) and bool((run["tok"][b] == -1).all()), (what, b)
            else:
                assert bool((run["tok"][b] >= 0).all()), (what, b)
        else:   # score rows beyond the env's length hold the fill values
            assert bool((run["tok"][b, nb:] == -1).all()) and bool((run["act"][b, nb:] == 0).all()), (what, b)
            assert bool((run["tok"][b, :nb] >= 0).all()), (what, b)


def _check_slots(case, eng, run, what, append=True, behind=True):
    """The per-slot bars on the sampled slots, then (append only) the env-step behind the call on the same slots."""
    geo, live, slots = case
    spec, sd, seq, _, refs = _case(*case)
    n, r = run["n"], run["r"]
    assert bool(run["act"].isfinite().all())
    for b in sc.sampled_slots(live):
        if n[b] == 0:
            continue
        act = _last(run, b)
        if r[b]:
            check_restarted(eng, spec, b, torch.cat([act] * (b + 1)), refs[b], what)
        elif append:
            check_continued(eng, spec, b, torch.cat([act] * (b + 1)), refs[b], _snaps(*case)[b], what)
    if not (append and behind):
        return
    a_next, _ = eng.step(*(x.to(DEV) for x in seq[sc.BEHIND[0]][:3]), None)
    torch.cuda.synchronize()
    a_next = a_next.cpu()
    assert a_next.shape[0] == live
    for b in sc.sampled_slots(live):
        act_ref, lg_ref = refs[b].cont[-1]
        assert assert_actions_match(a_next[b:b + 1], act_ref, lg_ref, spec, what=f"{what}: step behind the call, env {b}") == 0


def _close(a, b, what, bar=1e-4):
    for i, (x, y) in enumerate(zip(a, b)):
        err = rel_err(x, y)
        assert err < bar, (what, i, err)


# ---- 1. mode "live": append and replace, prefill and score ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_live_prefix_append_against_oracle_and_stepping_engine(hip_lib, case):
    geo, live, slots = case
    spec, sd, seq, _, refs = _case(*case)
    what = sc.case_key(*case) + " live append"
    clear_margins(list(refs.values()), what)
    _snaps(*case)
    eng = _primed(case)
    run = _call(case, eng, "live")
    _check_quiet(run, what)
    cap = _cap(spec)
    plan = context_plan(sc.L, run["n"], cap)
    assert run["counts"] == {"calls": 1, "chunks": len(plan), "env_timesteps": live * (sc.L - plan[0]), "kept": 0}, run["counts"]
    _check_slots(case, eng, run, what)
    eng.close()
    # the same call as a score: the state it leaves is the prefill's bit for bit, and so is every env's last action
    eng = _primed(case)
    score = _call(case, eng, "live", kind="score")
    eng.close()
    _check_quiet(score, what + " (score)")
    _same_bits(score["state"], run["state"], what + ": score against prefill")
    for b in run["started"]:
        assert torch.equal(bits(_last(score, b)), bits(_last(run, b))), (what, b)
    # isolation: a parked slot whose state is NaN changes no live bit and keeps its own
    bad_slot = slots - 1
    eng = _primed(case, poison=[bad_slot])
    assert not bool(eng.save_slots([bad_slot]).isfinite().all()), "the NaN observations left the parked slot a finite state"
    bad = _call(case, eng, "live")
    eng.close()
    _check_quiet(bad, what + ", a parked slot holds NaN")
    _same_bits(bad["state"], run["state"], what + ", a parked slot holds NaN: live slots")
    assert torch.equal(bits(bad["act"]), bits(run["act"])) and torch.equal(bad["tok"], run["tok"])


@pytest.mark.parametrize("geo", sc.GEOMETRIES)
def test_live_prefix_replace(hip_lib, geo):
    """lram_prefill_ragged / lram_score_ragged on the live prefix: every started env of length < 21 restarts whatever its flag, the
    length-0 slots are kept through the scratch records, the parked ones are no row at all."""
    case = (geo, 7, 12)
    spec, sd, seq, _, refs = _case(*case)
    from tests.context_cases import EnvRef
    what = sc.case_key(*case) + " live replace"
    n, r = sc.lengths(7), sc.restart(7)
    eng = _primed(case)
    run = _call(case, eng, "live", append=False)
    _check_quiet(run, what)
    assert run["counts"]["kept"] == n.count(0) and run["counts"]["env_timesteps"] == 7 * sc.L
    for b in run["started"]:
        if r[b]:
            check_restarted(eng, spec, b, torch.cat([_last(run, b)] * (b + 1)), refs[b], what)
        else:   # (restarted by the replace rule: its rows are not among those the seed was chosen on -- the state alone)
            check_restarted(eng, spec, b, None, EnvRef(spec, sd, seq, b, n[b]), what)
    eng.close()
    eng = _primed(case)
    score = _call(case, eng, "live", append=False, kind="score")
    eng.close()
    _check_quiet(score, what + " (score)")
    _same_bits(score["state"], run["state"], what + ": score against prefill")


# ---- 2. the identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", sc.GEOMETRIES)
def test_identities_with_mode_all_and_the_dense_entry(hip_lib, geo):
    spec, sd, seq, parked, _ = _case(geo, 7, 12)
    # (a) every slot live: mode "live" makes mode "all"'s launches
    runs = []
    for mode in ("all", "live", "started"):
        eng = new_engine(spec, sd, 7)
        for t in sc.PRE:
            eng.step(*(x.to(DEV) for x in seq[t][:3]), None)
        runs.append(_call((geo, 7, 7), eng, mode))
        eng.close()
    for k in ("state", "after"):
        _same_bits(runs[1][k], runs[0][k], f"{geo}: mode live with every slot live against mode all")
    assert torch.equal(bits(runs[1]["act"]), bits(runs[0]["act"])) and torch.equal(runs[1]["tok"], runs[0]["tok"])
    _same_bits(runs[2]["after"], runs[0]["after"], f"{geo}: mode started, length-0 slots")
    # (b) all lengths 21 on the live prefix: the dense entry's launches, in both modes
    full, none = [sc.L] * 7, [0] * 7
    outs = []
    for mode, lengths in (("live", None), ("live", full), ("started", full)):
        eng = _primed((geo, 7, 12))
        eng.set_context_rows(mode)
        act, tok = eng.prefill(*stack(seq, sc.L), reset_mask=u8_mask(none), lengths=lengths, append=lengths is not None)
        torch.cuda.synchronize()
        outs.append((_rows(eng, spec, list(range(12))), act.cpu().clone(), tok.cpu().clone(), eng.context_counts()))
        eng.close()
    for st, act, tok, counts in outs[1:]:
        _same_bits(st, outs[0][0], f"{geo}: all lengths 21 against the dense entry")
        assert torch.equal(bits(act), bits(outs[0][1])) and torch.equal(tok, outs[0][2])
        assert counts["env_timesteps"] == 7 * sc.L and counts["chunks"] == outs[0][3]["chunks"]


# ---- 3. mode "started" -------------------------------------------------------------------------------------------------------------
SETTINGS = [(None, None), (2, None), (None, "0")]


@pytest.mark.parametrize("micro,chunk", SETTINGS, ids=["default", "micro2", "chunk0"])
@pytest.mark.parametrize("case", [c for c in CASES if c[1] > 1], ids=[i for c, i in zip(CASES, IDS) if c[1] > 1])
def test_started_rows_against_live_rows(hip_lib, monkeypatch, case, micro, chunk):
    geo, live, slots = case
    spec, sd, seq, _, refs = _case(*case)
    what = sc.case_key(*case) + f" started micro={micro} chunk={chunk}"
    _snaps(*case)
    if chunk is not None:
        monkeypatch.setenv("LRAM_PREFILL_CHUNK", chunk)
    runs = {}
    for mode in ("live", "started"):
        eng = _primed(case, micro=micro)
        runs[mode] = _call(case, eng, mode)
        _check_quiet(runs[mode], f"{what} ({mode})")
        if mode == "started":
            _check_slots(case, eng, runs[mode], what)
        eng.close()
    if chunk is not None:
        monkeypatch.delenv("LRAM_PREFILL_CHUNK")
    n = runs["live"]["n"]
    plan = context_plan(sc.L, n, _cap(spec, chunk))
    assert runs["started"]["counts"] == {"calls": 1, "chunks": len(plan), "env_timesteps": sum(n), "kept": 0}, runs["started"]["counts"]
    assert runs["live"]["counts"] == {"calls": 1, "chunks": len(plan), "env_timesteps": live * (sc.L - plan[0]), "kept": 0}
    _same_bits(runs["started"]["after"], runs["live"]["after"], what + ": parked and length-0 slots")
    _close(runs["started"]["state"], runs["live"]["state"], what + ": started against live, state")
    for b in sc.sampled_slots(live):     # the actions: both against the oracle, no tie tolerated
        if n[b]:
            for mode in ("live", "started"):
                assert assert_actions_match(runs[mode]["act"][b:b + 1], refs[b].act, refs[b].logits, spec, what=f"{what} {mode} env {b}") == 0
    # replace under "started": nothing is kept, an env of length < 21 restarts at its own start
    eng = _primed(case, micro=micro)
    rep = _call(case, eng, "started", append=False)
    eng.close()
    _check_quiet(rep, what + " replace")
    assert rep["counts"]["kept"] == 0 and rep["counts"]["env_timesteps"] == sum(n)
    # ... and a score: the prefill's state bit for bit
    eng = _primed(case, micro=micro)
    score = _call(case, eng, "started", kind="score")
    eng.close()
    _check_quiet(score, what + " (score)")
    if chunk is None:
        _same_bits(score["state"], runs["started"]["state"], what + ": score against prefill")


# ---- 4. lazy matrix memory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["live", "started"])
def test_lazy_engine_with_pending_windows(hip_lib, mode):
    case = ("layout", 7, 12)
    geo, live, slots = case
    spec, sd, seq, parked, refs = _case(*case)
    what = f"{sc.case_key(*case)} lazy {mode}"
    _snaps(*case)
    eng = _primed(case, lazy=True)
    m0 = [i for i in range(spec.n_blocks) if i not in spec.slstm_at][0]
    pend = eng.lazy_peek(m0, "pending").cpu()
    assert float(pend[:live].max()) > 0 and float(pend[live:].max()) > 0, "no pending window in a live and a parked slot"
    n = sc.lengths(live)
    rec0 = eng.save_slots(list(range(live, slots))).cpu()
    eng.set_context_rows(mode)
    act, tok = eng.prefill(*stack(seq, sc.L, n), reset_mask=u8_mask(sc.restart(live)), lengths=n, append=True)
    torch.cuda.synchronize()
    eng.set_context_rows("all")
    rec1 = eng.save_slots(list(range(live, slots))).cpu()
    for block, which, shape, off in record_layout(spec)[0]:
        k = 1
        for s in shape:
            k *= s
        got, want = rec1[:, off:off + k], rec0[:, off:off + k]
        if block not in spec.slstm_at and which == 0:
            assert rel_err(got, want) <= 2e-4, (what, block, rel_err(got, want))
        else:
            assert torch.equal(bits(got), bits(want)), (what, block, which)
    run = dict(act=act.cpu().clone(), tok=tok.cpu().clone(), n=n, r=sc.restart(live))
    _check_slots(case, eng, run, what, behind=False)
    # five env-steps on the live prefix behind the call: the first is the case's own, the others re-use the inputs ahead of it
    from oracle.dt_ref import OraclePolicy
    ts = [sc.BEHIND[0]] + list(sc.PRE) + [sc.BEHIND[0]]
    got = []
    for t in ts:
        a, _ = eng.step(*(x.to(DEV) for x in seq[t][:3]), None)
        got.append(a.cpu().clone())
    torch.cuda.synchronize()
    eng.close()
    ties = 0
    for b in range(live):
        ora = OraclePolicy(spec, sd)
        row = lambda t: tuple(x[b:b + 1] for x in seq[t][:3])
        for t in (list(sc.PRE) if not (run["r"][b] and n[b]) else []) + list(range(n[b])):
            ora.step(*row(t))
        for k, t in enumerate(ts):
            a, dbg = ora.step(*row(t), return_debug=True)
            ties += assert_actions_match(got[k][b:b + 1], a, dbg["logits"], spec, what=f"{what}: step {k} behind the call, env {b}")
    print(f"[subset] {what}: ties over the five steps behind the call: {ties}")


# ---- 5. lram_encoder_step on the live rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["layout", "xlstm_tiny"])
def test_encoder_step_on_the_live_rows(hip_lib, geo):
    case = (geo, 7, 12)
    spec, sd, seq, parked, _ = _case(*case)
    x = torch.randn(7, 3, spec.d_model, generator=torch.Generator().manual_seed(5)).to(DEV)
    eng = _primed(case)
    with pytest.raises(LramError, match="parked"):
        eng.encoder_step(x)
    before = _rows(eng, spec, list(range(7, 12)))
    eng.set_context_rows("live")
    out = eng.encoder_step(x)
    torch.cuda.synchronize()
    _same_bits(before, _rows(eng, spec, list(range(7, 12))), f"{geo}: encoder_step, parked slots")
    live_state = _rows(eng, spec, list(range(7)))
    eng.close()
    # an engine of 7 slots with the same history: the rows, the kernels and the results of the live prefix
    ref = new_engine(spec, sd, 7)
    for t in sc.PRE:
        ref.step(*(x_.to(DEV) for x_ in seq[t][:3]), None)
    want = ref.encoder_step(x)
    torch.cuda.synchronize()
    assert out.shape == want.shape and rel_err(out.cpu(), want.cpu()) < 1e-4
    _close(live_state, _rows(ref, spec, list(range(7))), f"{geo}: encoder_step, live slots against a 7-slot engine")
    ref.close()


# ---- 6. frames on a mixed slot table -----------------------------------------------------------------------------------------------
def test_frames_take_the_image_slots_below_the_live_count(hip_lib):
    """tests/test_gpu_frame_contexts.py's mixed table (3 image slots ahead of 4 vector slots) as the live prefix of 10 slots whose
    parked tail holds one more image slot and two vector slots: the call is handed the frames of the three live image slots."""
    from lram_amd.domains import Domain, SlotTable
    from tests import test_gpu_frame_contexts as fc
    spec, sd, _, img, vec, refs, gap = fc.mixed_case()
    assert gap >= fc.MIN_GAP
    tab = SlotTable.from_domains([(Domain("procgen", True, 1, image=True), fc.N_IMG), (Domain("metaworld", False, 3), fc.N_VEC),
                                  (Domain("procgen_parked", True, 1, image=True), 1), (Domain("metaworld_parked", False, 3), 2)],
                                 max_act_dim=spec.act_dim)
    frames, rtg, rew = fc.frame_stack(img, fc.L, fc.LENGTHS, pad=255, rows=list(range(fc.N_IMG)))
    obs = torch.stack([x[0] for x in vec[:fc.L]], 1).contiguous()
    obs[:fc.N_IMG] = NAN
    for b, n in enumerate(fc.LENGTHS):
        obs[b, n:] = NAN
    eng = new_engine(spec, sd, 10)
    eng.set_slot_table(*tab.engine_arrays())
    eng.set_live(7)
    parked = eng.save_slots([7, 8, 9]).cpu()
    eng.set_context_rows("live")
    eng.image_counts(reset=True)
    act, tok = eng.prefill_frames(frames, rtg, rew, obs_seq=obs.to(DEV), lengths=fc.LENGTHS, reset_mask=u8_mask([1] * 7), discrete="per_slot")
    torch.cuda.synchronize()
    act = act.cpu().clone()
    assert act.shape[0] == 7 and eng.image_counts()["frames"] == sum(fc.LENGTHS[:fc.N_IMG]) == 35
    assert torch.equal(bits(parked), bits(eng.save_slots([7, 8, 9]).cpu()))
    for b, n in enumerate(fc.LENGTHS):
        if n == 0:
            continue
        ref = refs[b]
        if b < fc.N_IMG:
            want = torch.argmax(ref.logits.reshape(1, -1)[:, :spec.n_discrete], dim=-1)
            assert assert_actions_match(act[b:b + 1, :1], want, ref.logits, spec, discrete=True, what=f"mixed, image slot {b}") == 0
        else:
            assert assert_actions_match(act[b:b + 1, :3], ref.act[:, :3], ref.logits[..., :3, :], spec, what=f"mixed, vector slot {b}") == 0
        check_restarted(eng, spec, b, None, ref, "mixed table on the live prefix")
    eng.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched(hip_lib):
    case = ("xlstm_tiny", 7, 12)
    spec, sd, seq, _, _ = _case(*case)
    eng = _primed(case)
    state = _rows(eng, spec, list(range(12)))
    n = sc.lengths(7)
    unsorted = [14, 21, 8, 3, 1, 0, 0]
    eng.set_context_rows("started")
    with pytest.raises(LramError, match=r"length 21 of env slot 1 exceeds length 14 of env slot 0"):
        eng.prefill(*stack(seq, sc.L, unsorted), lengths=unsorted, append=True)
    with pytest.raises(LramError, match=r"env slot 5"):
        eng.score(*stack(seq, sc.L, n), lengths=[21, 14, 8, 3, 0, 1, 0], append=False, want=("tokens",))
    assert eng.context_counts() == {"calls": 0, "chunks": 0, "env_timesteps": 0, "kept": 0}
    assert eng.lib.lram_set_context_rows(eng._h, 3) != 0 and b"outside 0 .. 2" in eng.lib.lram_last_error()
    assert eng.lib.lram_set_context_rows(eng._h, -1) != 0 and eng.lib.lram_get_context_rows(eng._h) == 2
    with pytest.raises(ValueError):
        eng.set_context_rows("some")
    eng.set_context_rows("all")
    full = stack(seq + [], sc.L)
    with pytest.raises(LramError, match="5 of 12 env slots are parked"):
        eng.prefill(*(torch.cat([x, x])[:12].contiguous() for x in full))
    arr = (ctypes.c_int32 * 12)(*([21] * 12))
    from lram_amd.engine import _ptr, _stream_ptr
    obs, rtg, rew = (torch.cat([x, x])[:12].contiguous() for x in full)
    rc = eng.lib.lram_prefill_append(eng._h, _ptr(obs), 0, _ptr(rtg), _ptr(rew), sc.L, arr, None, 0, _ptr(eng._actions),
                                     _ptr(eng._tokens), _stream_ptr(eng.device))
    assert rc != 0 and b"env slots are parked (lram_set_live)" in eng.lib.lram_last_error()
    torch.cuda.synchronize()
    _same_bits(state, _rows(eng, spec, list(range(12))), "refused calls")
    eng.alloc(12)
    assert eng.context_rows == "all" and eng.lib.lram_get_context_rows(eng._h) == 0
    eng.close()


# ---- 8. the agent ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["layout", "mamba_tiny"])
def test_agent_extends_the_contexts_of_listed_envs(hip_lib, geo):
    """Eight envs, five of them parked; extend_contexts(envs=[6, 1, 4]) hands a parked env (6) and two active ones the steps they
    missed.  Against an agent that never parks and extends the same envs with lengths 0 for the others, at the bars; the
    bystanders' records are bit-identical, and the active set is what it was."""
    from lram_amd.agent import RecurrentAgent
    spec, sd, seq, _, _ = _case(geo, 7, 12)
    n_envs, envs = 8, [6, 1, 4]
    lengths = [0, 14, 0, 0, 8, 0, 21, 0]
    g = torch.Generator().manual_seed(11)
    obs = torch.rand(n_envs, sc.L, spec.state_dim, generator=g) * 2 - 1
    rtg = torch.rand(n_envs, sc.L, generator=g) + 3.0
    pre = [(torch.rand(n_envs, spec.state_dim, generator=g) * 2 - 1, torch.full((n_envs,), 4.0)) for _ in range(3)]
    agents = [RecurrentAgent(spec, sd, n_envs=n_envs, device=DEV) for _ in range(2)]
    for a in agents:
        for o, r in pre:
            a.predict_batch(o.to(DEV), r.to(DEV), None, None)
    parks, plain = agents
    parks.set_active([1, 4, 5])
    slot_of = list(parks.scheduler.slot_of)
    rec0 = parks.engine.save_slots([slot_of[e] for e in range(n_envs)]).cpu()
    got = parks.extend_contexts(obs, rtg, lengths=lengths, envs=envs, want_action=True)
    want = plain.extend_contexts(obs, rtg, lengths=lengths, want_action=True)
    torch.cuda.synchronize()
    assert sorted(parks.active) == [1, 4, 5] and parks.engine.live == 3 and parks.engine.context_rows == "all"
    assert list(parks.scheduler.slot_of) == slot_of
    rec1 = parks.engine.save_slots([slot_of[e] for e in range(n_envs)]).cpu()
    ref = plain.engine.save_slots(list(range(n_envs))).cpu()
    for e in range(n_envs):
        if e in envs:
            assert rel_err(rec1[e], ref[e]) < 1e-4, (geo, e, rel_err(rec1[e], ref[e]))
            assert float((got[e].float().cpu() - want[e].float().cpu()).abs().max()) <= 2.0 / 256 + 1e-6, (geo, e)
        else:
            assert torch.equal(bits(rec1[e]), bits(rec0[e])), (geo, e)
            assert bool((got[e] == 0).all())
    for a in agents:
        a.engine.close()
