"""GPU: every block layout and stack depth the engine accepts (tests/layout_cases.py): an sLSTM block first, last, twice in a row,
alternating, behind three mLSTM blocks, everywhere and nowhere; one block; 64 blocks, xLSTM and Mamba.  The layout selects HOST
code -- the schedule of the lazy folds with two env slices (folds ahead of the first read pass, shared out over the sLSTM
stretches, right ahead of a block, behind the last mLSTM block for the next step), the per-slot record, the per-block events of
the chunk lanes, the keys of past_key_values -- so every case runs step parity, the lazy matrix memory with one and two slices,
stored contexts, per-slot state, graph replay and env slices.

Bars are the project's fixed ones and none is new: hidden and state 2e-4 against the fp32 oracle (helpers.rel_err,
helpers.state_vs_oracle with C / n per element), actions through helpers.assert_actions_match with ZERO ties (seeds chosen on the
CPU: the oracle's own top-2 gap is at least 1e-3 and it stays within 2e-5 of its float64 evaluation), engine against engine 1e-4
(actions 1e-4, lazy against materialised state 2e-4), and torch.equal wherever two runs launch the same kernels on the same bits
(tail fold on / off, chunk lanes on / off, graph replay, loaded records, imported past_key_values).
deep64 runs on the reference's own weight initialisation (layout_cases.DEEP64_SCHEME: on the two other weight distributions the
fp32 recurrence of 64 xLSTM blocks is 5.6e-2 from float64, and two engine runs that round differently are as far apart) and is
held by the engine-against-engine comparisons; its one oracle run is the step parity."""
import copy
import ctypes
import os

import pytest
import torch

from lram_amd import init_state_dict
from lram_amd.config import ModelSpec
from oracle import dt_ref, mamba_ref, xlstm_ref
from tests import layout_cases as lc
from tests.helpers import assert_actions_match, make_inputs, rel_err, state_vs_oracle
from tests.slot_state_helpers import exported_slice, record_layout

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPORT = bool(os.environ.get("LRAM_TEST_REPORT"))
_CACHE = {}


def _engine(spec, sd, B):
    from lram_amd.engine import Engine
    return Engine(spec, sd, B, device=DEV)


def _model(cid, seed, scheme=None):
    scheme = lc.case_scheme(cid) if scheme is None else scheme
    key = ("model", cid, seed, scheme)
    if key not in _CACHE:
        spec = lc.case_spec(cid)
        _CACHE[key] = (spec, init_state_dict(spec, seed=seed, scheme=scheme))
    return _CACHE[key]


def _oracle(key, spec, sd, seq, discrete=False):
    """The oracle's run over seq, computed once per key and never changed: per step (actions, logits, hidden, tokens), final state."""
    key = ("oracle",) + key
    if key not in _CACHE:
        ora = dt_ref.OraclePolicy(spec, sd)
        steps = []
        for obs, rtg, rew, mask in seq:
            a, dbg = ora.step(obs, rtg, rew, mask, discrete=discrete, return_debug=True)
            steps.append((a, dbg["logits"], dbg["hidden"], dbg["tokens"]))
        _CACHE[key] = (steps, copy.deepcopy(ora.state))
    return _CACHE[key]


def _kinds(spec, blk):
    return (0, 3) if (spec.backbone == "mamba" or blk in spec.slstm_at) else (0, 1, 2, 3)


def _state(eng, spec):
    out = [eng.export_state_tensor(blk, w).clone() for blk in range(spec.n_blocks) for w in _kinds(spec, blk)]
    torch.cuda.synchronize()
    return out


def _mlstm_state(eng, spec):
    return [eng.export_state_tensor(i, w).clone() for i in lc.mlstm_blocks(spec) for w in (0, 1, 2)]


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, (tuple, list)):
            _same(g, w, f"{what}[{k}]")
        else:
            assert torch.equal(g, w), f"{what}[{k}]: {int((g != w).sum())} of {g.numel()} elements differ"


def _steps(eng, seq, taps=False, discrete=False):
    out = []
    for obs, rtg, rew, mask in seq:
        a, t = eng.step(obs.to(DEV), rtg.to(DEV), rew.to(DEV), None if mask is None else mask.to(DEV), discrete=discrete)
        row = [a.clone(), t.clone()]
        if taps:
            tok, hid, logits = eng.taps()
            row += [tok, hid, logits]
        out.append(row)
    torch.cuda.synchronize()
    return out


def _stack(seq):
    return tuple(torch.stack([x[i] for x in seq], 1).contiguous().to(DEV) for i in range(3))


def _report(line):
    if REPORT:
        print(f"[layout] {line}")


def _worst_state_err(eng, spec, ora_state):
    """Largest rel_err over the state tensors (for the report only; the bars are state_vs_oracle's)."""
    worst = 0.0
    for i in range(spec.n_blocks):
        for w in _kinds(spec, i):
            got = eng.export_state_tensor(i, w)
            if spec.backbone == "mamba":
                want = ora_state[i][1 if w == 0 else 0]
            elif w == 3:
                want = ora_state[f"block_{i}"]["conv_state"][0]
            elif i in spec.slstm_at:
                want = ora_state[f"block_{i}"]["slstm_state"]
            else:
                want = ora_state[f"block_{i}"]["mlstm_state"][w]
            worst = max(worst, rel_err(got, want))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# a. step parity, two weight distributions; the discrete head
# ---------------------------------------------------------------------------------------------------------------------
def _parity(cid, scheme, seed, B, discrete=False):
    spec, sd = _model(cid, seed, scheme)
    seq = make_inputs(spec, B, lc.STEP_STEPS, seed=1234 + seed, reset_prob=lc.RESET_PROB)
    ref, ora_state = _oracle((cid, scheme, seed, B, discrete), spec, sd, seq, discrete)
    eng = _engine(spec, sd, B)
    assert eng.state_mode == "materialised"
    eng.gemm_counts(reset=True), eng.slstm_counts(reset=True)
    got = _steps(eng, seq, taps=True, discrete=discrete)
    ties, worst_h = 0, 0.0
    for t, ((a, _, tok, hid, _), (a_ref, logits, hidden, tokens)) in enumerate(zip(got, ref)):
        assert rel_err(tok, tokens) < 1e-5, f"{cid}/{scheme} step {t}: embedded tokens"
        err = rel_err(hid, hidden)
        worst_h = max(worst_h, err)
        assert err < 2e-4, f"{cid}/{scheme} step {t}: hidden {err:.2e}"
        ties += assert_actions_match(a[:, :1] if discrete else a, a_ref, logits, spec, discrete, what=f"{cid}/{scheme} step {t}")
    assert ties == 0
    if REPORT:
        gc = {k: v["launches"] for k, v in eng.gemm_counts().items()}
        _report(f"parity {cid} {scheme}{' discrete' if discrete else ''}: hidden {worst_h:.1e} state {_worst_state_err(eng, spec, ora_state):.1e} "
                f"mode {eng.state_mode} slices 1 gemm {gc} slstm {eng.slstm_counts() if spec.backbone == 'xlstm' else '-'}")
    state_vs_oracle(eng.export_state_tensor, ora_state, spec, f"{cid}/{scheme}")
    eng.close()


@pytest.mark.parametrize("scheme", ["exercise", "trained_like"])
@pytest.mark.parametrize("cid", lc.ORACLE_CASES)
def test_step_parity_against_the_oracle(hip_lib, cid, scheme):
    """8 env-steps with random restarts, 7 env slots (Mamba 5): embedded tokens, hidden taps, actions with zero ties, and every
    block's final state against the fp32 oracle."""
    seed, gap, dist, elem = lc.STEP_SEEDS[(cid, scheme)]
    assert gap >= lc.GAP_MIN and dist <= lc.DIST_MAX and elem <= lc.ELEM_MAX
    _parity(cid, scheme, seed, lc.step_batch(cid))


def test_step_parity_of_the_64_block_stack(hip_lib):
    """deep64 on the reference's initialisation, where its fp32 recurrence is well conditioned (layout_cases.DEEP64_SCHEME)."""
    seed, gap, dist, elem = lc.DEEP64_STEP
    assert gap >= lc.GAP_MIN and dist <= lc.DIST_MAX and elem <= lc.ELEM_MAX
    _parity("deep64", lc.DEEP64_SCHEME, seed, lc.step_batch("deep64"))


@pytest.mark.parametrize("cid", lc.DISCRETE_CASES)
def test_discrete_head(hip_lib, cid):
    seed, gap, dist, elem = lc.DISCRETE_SEEDS[cid]
    assert gap >= lc.GAP_MIN and dist <= lc.DIST_MAX and elem <= lc.ELEM_MAX
    _parity(cid, "exercise", seed, 7, discrete=True)


# ---------------------------------------------------------------------------------------------------------------------
# b. lazy matrix memory: one slice against the materialised engine and the oracle; two slices with the tail fold on and off
# ---------------------------------------------------------------------------------------------------------------------
def _lazy_case(cid):
    """Model, inputs and the materialised engine's run of the 30-step trajectory (once per case, shared by both periods)."""
    key = ("lazy", cid)
    if key not in _CACHE:
        seed = lc.DEEP64_SEED if cid == "deep64" else lc.LAZY_SEEDS[cid][0]
        spec, sd = _model(cid, seed)
        seq = make_inputs(spec, lc.LAZY_B, lc.LAZY_STEPS, seed=1234 + seed, reset_prob=lc.RESET_PROB)
        eager = _engine(spec, sd, lc.LAZY_B)
        eager.set_state_mode("eager")
        assert eager.state_mode == "materialised"
        acts = torch.stack([r[0] for r in _steps(eager, seq)]).cpu()
        state = [t.cpu() for t in _mlstm_state(eager, spec)]
        eager.close()
        _CACHE[key] = (seed, spec, sd, seq, acts, state)
    return _CACHE[key]


@pytest.mark.parametrize("period", lc.LAZY_PERIODS)
@pytest.mark.parametrize("cid", lc.LAZY_CASES)
def test_lazy_one_slice_against_materialised_and_the_oracle(hip_lib, cid, period):
    """30 steps with restarts in the lazy mode (fold period 13: two or three folds per env; 3: ten), one slice -- fold(i) right
    ahead of block i: actions within 1e-4 of the materialised engine's, exported C / n / m within 2e-4; and (not deep64) hidden
    taps, actions with zero ties and every block's state against the oracle."""
    seed, spec, sd, seq, a_e, s_e = _lazy_case(cid)
    lazy = _engine(spec, sd, lc.LAZY_B)
    lazy.set_state_mode("lazy", period)
    lazy.set_micro_batches(1)
    assert lazy.state_mode == "lazy"
    got = _steps(lazy, seq, taps=True)
    a_l = torch.stack([r[0] for r in got]).cpu()
    worst_a = float((a_l - a_e).abs().max())
    s_l = [t.cpu() for t in _mlstm_state(lazy, spec)]
    worst_s = max(rel_err(g, w) for g, w in zip(s_l, s_e))
    _report(f"lazy {cid} period {period} one slice: actions off the materialised engine's by {worst_a:.1e} (bar 1e-4), C / n / m {worst_s:.1e} (bar 2e-4)")
    assert worst_a <= 1e-4, (cid, period, worst_a)
    for k, (g, w) in enumerate(zip(s_l, s_e)):
        assert rel_err(g, w) < 2e-4, (cid, period, k, rel_err(g, w))
    if cid in lc.ORACLE_CASES:
        _, gap, dist, elem = lc.LAZY_SEEDS[cid]
        assert gap >= lc.GAP_MIN and dist <= lc.DIST_MAX and elem <= lc.ELEM_MAX
        ref, ora_state = _oracle((cid, "lazy", seed), spec, sd, seq)
        ties, worst_h = 0, 0.0
        for t, (row, (a_ref, logits, hidden, _)) in enumerate(zip(got, ref)):
            err = rel_err(row[3], hidden)
            worst_h = max(worst_h, err)
            assert err < 2e-4, (cid, period, t, err)
            ties += assert_actions_match(row[0], a_ref, logits, spec, what=f"{cid} lazy period {period} step {t}")
        assert ties == 0
        _report(f"lazy {cid} period {period} one slice: hidden {worst_h:.1e} state {_worst_state_err(lazy, spec, ora_state):.1e}")
        state_vs_oracle(lazy.export_state_tensor, ora_state, spec, f"{cid} lazy period {period}")
    lazy.close()


# ---- two slices: the tail fold changes no bit; one other entry over a pending tail fold -----------------------------------------
TB, BEFORE, AFTER = 9, 20, 10      # 9 env slots = slices of 5 + 4


def _due(period):
    """The envs whose fold is due at step BEFORE (0-based): what a tail fold at the end of step BEFORE - 1 folds early."""
    return [b for b in range(TB) if (BEFORE + b) % period == 0]


def _op_save_slots(eng, spec, seq, period):
    keep = [b for b in range(TB) if b not in _due(period)]   # (a record of a slot folded early has another rounding of C:
    return [eng.save_slots(keep[:3]).clone()]                #  tests/test_gpu_fold_tail.py::test_record_of_a_slot_folded_early)


def _op_copy_slots(eng, spec, seq, period):
    """One slot forked and the due slot overwritten, both from slots that are not due.  (Not FROM the due slot: with the tail fold
    its copy is a folded C_base and an empty window, without it an unfolded C_base and a full window -- the same state in two
    representations, which later folds round differently: test_record_of_a_slot_folded_early.)"""
    due = _due(period)
    other = [b for b in range(TB) if b not in due]
    eng.copy_slots([other[0], other[2]], [other[1], due[0]])
    return []


def _op_export_state_tensor(eng, spec, seq, period):
    blocks = lc.mlstm_blocks(spec)
    return [eng.export_state_tensor(blocks[0], 0).clone(), eng.export_state_tensor(blocks[-1], 1).clone()]


def _op_prefill(eng, spec, seq, period):
    a, t = eng.prefill(*_stack(seq[:9]))
    return [a.clone(), t.clone()]


def _op_lazy_peek(eng, spec, seq, period):
    """lazy_peek completes the pending early fold before it looks: the due envs show an empty window where the engine without the
    tail fold still shows their pending tokens -- the evidence that the step before did leave a tail fold pending.  Returned
    apart from the rest, which is compared bit for bit."""
    blocks = lc.mlstm_blocks(spec)
    pend, g = eng.lazy_peek(blocks[0], "pending").clone(), eng.lazy_peek(blocks[-1], "g").clone()
    rest = [b for b in range(TB) if b not in _due(period)]
    eng.peeked_due = pend[_due(period)].cpu()
    return [pend[rest], g[rest], eng.lazy_peek(blocks[0], "m").clone()]


OPS = [_op_save_slots, _op_copy_slots, _op_export_state_tensor, _op_prefill, _op_lazy_peek]


def _tail_engine(monkeypatch, spec, sd, period, tail):
    if tail:
        monkeypatch.delenv("LRAM_FOLD_TAIL", raising=False)
    else:
        monkeypatch.setenv("LRAM_FOLD_TAIL", "0")
    eng = _engine(spec, sd, TB)     # (the switch is read at lram_create)
    monkeypatch.delenv("LRAM_FOLD_TAIL", raising=False)
    eng.set_state_mode("lazy", period)
    eng.set_micro_batches(2)
    assert eng.state_mode == "lazy"
    return eng


@pytest.mark.parametrize("period", lc.LAZY_PERIODS)
@pytest.mark.parametrize("cid", lc.LAZY_CASES)
def test_lazy_two_slices_tail_fold_changes_no_bit(hip_lib, monkeypatch, cid, period):
    """Two env slices (5 + 4): the folds go to the state-pass stream by the layout's schedule, and with the tail fold the first
    two mLSTM blocks' folds of step n + 1 run behind the last mLSTM block's read passes of step n.  An engine created with
    LRAM_FOLD_TAIL=0 against the default, BIT FOR BIT: actions and tokens of 20 steps, then one entry other than a step over the
    pending tail fold (save_slots, copy_slots, export_state_tensor, a 9-timestep prefill, lazy_peek: rotated over the cases and the
    two periods), ten more steps, and every mLSTM state tensor.  Fold launches per step: one per mLSTM block either way.  The run
    with the tail fold is then held to a materialised one-slice engine that takes the same calls: a schedule that is wrong with
    and without the tail fold alike would pass the first comparison."""
    seed = lc.DEEP64_SEED if cid == "deep64" else lc.LAZY_SEEDS[cid][0]
    spec, sd = _model(cid, seed)
    seq = make_inputs(spec, TB, BEFORE + AFTER, seed=34 + seed, reset_prob=0.1)
    extra = make_inputs(spec, TB, 9, seed=35, reset_prob=0.0)
    op = OPS[(lc.LAZY_CASES.index(cid) + lc.LAZY_PERIODS.index(period)) % len(OPS)]
    assert _due(period), "no env is due at the step behind the entry: no tail fold would be pending"
    n_mlstm = len(lc.mlstm_blocks(spec))
    outs, peeked = [], []
    for tail in (False, True):
        eng = _tail_engine(monkeypatch, spec, sd, period, tail)
        first = _steps(eng, seq[:BEFORE - 3])
        eng.profile_begin()
        first += _steps(eng, seq[BEFORE - 3:BEFORE])
        _, n_main, _, n_aux = eng.profile_end_split()
        assert n_aux == 3 * n_mlstm and n_main == 3 * n_mlstm * 2, (cid, period, tail, n_main, n_aux)
        mid = op(eng, spec, extra, period)
        peeked.append(getattr(eng, "peeked_due", None))
        outs.append([first, mid, _steps(eng, seq[BEFORE:]), _mlstm_state(eng, spec)])
        _report(f"folds {cid} period {period} two slices tail {'on' if tail else 'off'}: {n_aux / 3:g} fold launches per step, "
                f"{n_main / 3:g} read passes, entry {op.__name__[4:]}")
        eng.close()
    _same(outs[1], outs[0], f"{cid} period {period} {op.__name__}")
    if op is _op_lazy_peek:
        assert float(peeked[0].min()) > 0.0 and float(peeked[1].max()) == 0.0, (peeked, "the step before left no tail fold pending")
    # ... and both are right: a materialised engine on one slice through the same calls, at the bars lazy and materialised runs are
    # held to each other (actions by the materialised engine's own logits, C / n / m within 2e-4)
    mat = _engine(spec, sd, TB)
    mat.set_state_mode("eager"), mat.set_micro_batches(1)
    rows = _steps(mat, seq[:BEFORE], taps=True)
    if op is not _op_lazy_peek:
        op(mat, spec, extra, period)
    rows += _steps(mat, seq[BEFORE:], taps=True)
    for t, (got, want) in enumerate(zip(outs[1][0] + outs[1][2], rows)):
        logits = want[4].view(TB, spec.act_dim, spec.n_vocab).cpu()
        assert_actions_match(got[0], want[0].cpu(), logits, spec, what=f"{cid} period {period} two slices, step {t}")
    for k, (g, w) in enumerate(zip(outs[1][3], _mlstm_state(mat, spec))):
        assert rel_err(g, w) < 2e-4, (cid, period, k, rel_err(g, w))
    mat.close()


def test_slstm_only_stack_refuses_the_lazy_mode(hip_lib):
    """No mLSTM block, no matrix memory: lram_set_state_mode(lazy) is refused with a message (include/lram_hip.h), the engine stays
    materialised, and goes on as an engine that was never asked."""
    from lram_amd.engine import LramError
    seed = lc.STEP_SEEDS[("s_all", "exercise")][0]
    spec, sd = _model("s_all", seed)
    B = lc.step_batch("s_all")
    seq = make_inputs(spec, B, 4, seed=1234 + seed, reset_prob=lc.RESET_PROB)
    eng, plain = _engine(spec, sd, B), _engine(spec, sd, B)
    first = _steps(eng, seq[:2], taps=True)
    with pytest.raises(LramError, match="at least one mLSTM block"):
        eng.set_state_mode("lazy", 3)
    assert eng.state_mode == "materialised"
    eng.set_state_mode("auto")
    assert eng.state_mode == "materialised"
    _same(first + _steps(eng, seq[2:], taps=True), _steps(plain, seq, taps=True), "s_all after the refusal")
    _same(_state(eng, spec), _state(plain, spec), "s_all state after the refusal")
    with pytest.raises(LramError):
        eng.lazy_peek(0, "pending")
    eng.profile_begin()
    _steps(eng, seq[:2])
    _, n_main, _, n_aux = eng.profile_end_split()
    assert n_aux == 0, n_aux
    _report(f"folds s_all: {n_aux} fold launches per step, {n_main} state passes counted, mode {eng.state_mode}")
    eng.close(), plain.close()


def test_state_mode_of_an_slstm_only_stack_at_128_slots(hip_lib):
    """The 16M geometry (head dim 256) at 128 env slots is where the automatic mode turns lazy: one block's matrix memory over the
    batch is 128 MiB.  With an mLSTM block it does; an sLSTM-only stack of the same geometry has no matrix memory, runs the
    materialised kernels, and says so."""
    kw = dict(backbone="xlstm", kind="MDDXLSTM", d_model=512, n_blocks=2, state_dim=20, act_dim=4)
    for slstm_at, want in (([0, 1], "materialised"), ([0], "lazy")):
        spec = ModelSpec(slstm_at=slstm_at, **kw)
        eng = _engine(spec, init_state_dict(spec, seed=1), 128)
        assert eng.state_mode == want, (slstm_at, eng.state_mode)
        seq = make_inputs(spec, 128, 2, seed=3, reset_prob=0.1)
        eng.profile_begin()
        acts = _steps(eng, seq)
        _, _, _, n_aux = eng.profile_end_split()
        assert n_aux == (2 if want == "lazy" else 0), (slstm_at, n_aux)
        assert bool(acts[-1][0].isfinite().all())
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# c. stored contexts
# ---------------------------------------------------------------------------------------------------------------------
def _context_case(cid):
    key = ("context", cid)
    if key not in _CACHE:
        seed = lc.DEEP64_SEED if cid == "deep64" else lc.CONTEXT_SEEDS[cid][0]
        spec, sd = _model(cid, seed)
        _CACHE[key] = (seed, spec, sd, make_inputs(spec, lc.CONTEXT_B, 50, seed=300 + seed, reset_prob=0.0))
    return _CACHE[key]


@pytest.mark.parametrize("cid", lc.ALL_CASES)
def test_prefill_equals_steps_and_the_oracle(hip_lib, cid):
    """lram_prefill of 21 timesteps (xLSTM: one 63-token chunk) and of 5 against the same number of lram_step calls -- actions
    within 1e-4, every state tensor within 1e-4 -- and (not deep64) against the oracle: the last action with zero ties, every
    state tensor."""
    seed, spec, sd, seq = _context_case(cid)
    B = lc.CONTEXT_B
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    for L in (21, 5):
        e_pre, e_step = _engine(spec, sd, B), _engine(spec, sd, B)
        act, _ = e_pre.prefill(*_stack(seq[:L]), reset_mask=ones)
        a_step = _steps(e_step, [(o, r, w, None) for o, r, w, _ in seq[:L]])[-1][0]
        worst_a = float((act - a_step).abs().max())
        s_pre, s_step = _state(e_pre, spec), _state(e_step, spec)
        worst_s = max(rel_err(g, w) for g, w in zip(s_pre, s_step))
        _report(f"prefill {cid} L={L}: actions off the steps' by {worst_a:.1e}, state {worst_s:.1e} (bars 1e-4)")
        assert worst_a <= 1e-4 and worst_s < 1e-4, (cid, L, worst_a, worst_s)
        if cid in lc.ORACLE_CASES:
            _, gap, dist, elem = lc.CONTEXT_SEEDS[cid]
            assert gap >= lc.GAP_MIN and dist <= lc.DIST_MAX and elem <= lc.ELEM_MAX
            ref, _ = _oracle((cid, "context", seed, lc.CONTEXT_L), spec, sd, seq[:lc.CONTEXT_L])
            assert assert_actions_match(act, ref[L - 1][0], ref[L - 1][1], spec, what=f"{cid} prefill L={L}") == 0
            _, ora_state = _oracle((cid, "context", seed, L), spec, sd, seq[:L])
            state_vs_oracle(e_pre.export_state_tensor, ora_state, spec, f"{cid} prefill L={L}")
        e_pre.close(), e_step.close()


@pytest.mark.parametrize("cid", lc.ALL_CASES)
def test_prefill_chunk_lanes_change_no_bit(hip_lib, monkeypatch, cid):
    """50 timesteps with the default chunk lanes (block i of chunk c + 1 waits for block i of chunk c: one event per block and
    lane, 64 of them per lane for deep64 and m_64) against one chunk at a time (LRAM_PREFILL_CHUNK=3), bit for bit, two prefills
    in a row -- the second continues from the state the first one left."""
    seed, spec, sd, seq = _context_case(cid)
    B = lc.CONTEXT_B
    inputs = _stack(seq[:50])
    e_lanes = _engine(spec, sd, B)
    monkeypatch.setenv("LRAM_PREFILL_CHUNK", "3")
    e_serial = _engine(spec, sd, B)
    monkeypatch.delenv("LRAM_PREFILL_CHUNK")
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    for rep in range(2):
        mask = ones if rep == 0 else None
        a_l, t_l = e_lanes.prefill(*inputs, reset_mask=mask)
        a_s, t_s = e_serial.prefill(*inputs, reset_mask=mask)
        torch.cuda.synchronize()
        assert bool(a_l.isfinite().all()), (cid, rep)
        assert torch.equal(a_l, a_s) and torch.equal(t_l, t_s), (cid, rep)
        _same(_state(e_lanes, spec), _state(e_serial, spec), f"{cid} lanes against one chunk at a time, prefill {rep}")
    e_lanes.close(), e_serial.close()


@pytest.mark.parametrize("cid", lc.ORACLE_CASES)
def test_encoder_step_token_counts(hip_lib, cid):
    """encoder_step with 1, 4, 12 and 40 tokens on one state (xLSTM: step kernels, token-sequential kernels, the chunkwise ones at
    40; Mamba takes at most 12 tokens per call, so its 40 go as 12 + 12 + 12 + 4) against the reference encoder, and the state it
    leaves in the reference layout."""
    seed, spec, sd, _ = _context_case(cid)
    B = lc.CONTEXT_B
    eng = _engine(spec, sd, B)
    fwd = xlstm_ref.encoder_forward_cached if spec.backbone == "xlstm" else mamba_ref.encoder_forward_cached
    state = None
    g = torch.Generator().manual_seed(9)
    for T in (1, 4, 12, 40):
        x = torch.randn(B, T, spec.d_model, generator=g)
        ref, state = fwd(spec, sd, x, state)
        pieces = [T] if (spec.backbone == "xlstm" or T <= 12) else [12, 12, 12, 4]
        out, t0 = [], 0
        for n in pieces:
            out.append(eng.encoder_step(x[:, t0:t0 + n].contiguous().to(DEV)).clone())
            t0 += n
        out = torch.cat(out, 1)
        torch.cuda.synchronize()
        assert rel_err(out, ref) < 2e-4, (cid, T, rel_err(out, ref))
    pkv = eng.export_past_key_values()
    for i in range(spec.n_blocks):
        if spec.backbone == "mamba":
            assert rel_err(pkv[i][0], state[i][0]) < 2e-4 and rel_err(pkv[i][1], state[i][1]) < 2e-4, (cid, i)
            continue
        got, want = pkv[f"block_{i}"], state[f"block_{i}"]
        assert rel_err(got["conv_state"][0], want["conv_state"][0]) < 2e-4, (cid, i)
        if i in spec.slstm_at:
            assert rel_err(got["slstm_state"], want["slstm_state"]) < 2e-4, (cid, i)
        else:
            for k in range(3):
                assert rel_err(got["mlstm_state"][k], want["mlstm_state"][k]) < 2e-4, (cid, i, k)
    eng.close()


def _env_slices(eng, spec, b):
    out = []
    for blk in range(spec.n_blocks):
        for w in _kinds(spec, blk):
            t = eng.export_state_tensor(blk, w)
            out.append((t[:, b] if (spec.backbone == "xlstm" and blk in spec.slstm_at and w == 0) else t[b]).clone())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cid", lc.ALL_CASES)
def test_ragged_prefill_and_score_against_the_dense_calls(hip_lib, cid):
    """prefill(lengths=[21, 0, 8]) and score over the same context, every padded input NaN, as tests/test_gpu_ragged.py holds the
    16M stack: both leave bit-identical states and the same last action; the slot without a context keeps its state bit for bit
    (action 0, token -1); each env with a context against the dense calls over its own length -- states within 1e-4, actions by
    the dense run's logits, logp within 2 * 2e-4 * max|logits|."""
    seed, spec, sd, seq = _context_case(cid)
    B, L, lengths = lc.CONTEXT_B, 21, [21, 0, 8]
    A = spec.act_dim
    obs, rtg, rew = (torch.stack([x[i] for x in seq[:L]], 1).contiguous() for i in range(3))
    for b, n in enumerate(lengths):
        obs[b, n:], rtg[b, n:], rew[b, n:] = float("nan"), float("nan"), float("nan")
    obs, rtg, rew = obs.to(DEV), rtg.to(DEV), rew.to(DEV)
    target = (torch.rand(B, L, A, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    e_pre, e_score, e_ref = (_engine(spec, sd, B) for _ in range(3))
    for eng in (e_pre, e_score):     # two env-steps first: the slot without a context has a state to keep
        _steps(eng, [(o, r, w, None) for o, r, w, _ in seq[30:32]])
    kept = _env_slices(e_pre, spec, 1)
    a_pre, t_pre = e_pre.prefill(obs, rtg, rew, reset_mask=ones, lengths=lengths)
    res = e_score.score(obs, rtg, rew, actions=target, reset_mask=ones, logits=True, lengths=lengths)
    torch.cuda.synchronize()
    _same(_state(e_score, spec), _state(e_pre, spec), f"{cid}: score(lengths) against prefill(lengths)")
    _same(_env_slices(e_pre, spec, 1), kept, f"{cid}: the slot of length 0")
    assert bool((a_pre[1] == 0).all()) and bool((t_pre[1] == -1).all())
    assert bool((res.logp[1] == 0).all()) and bool((res.tokens[1] == -1).all())
    for b, n in ((0, 21), (2, 8)):
        assert bool((res.tokens[b, n:] == -1).all()) and bool((res.logp[b, n:] == 0).all()) and bool((res.logits[b, n:] == 0).all())
        assert torch.equal(res.actions[b, n - 1], a_pre[b]) and torch.equal(res.tokens[b, n - 1], t_pre[b]), (cid, b)
        clean = [torch.nan_to_num(x[:, :n], nan=0.0).contiguous() for x in (obs, rtg, rew)]
        ref = e_ref.score(*clean, actions=target[:, :n].contiguous(), reset_mask=ones, logits=True)
        torch.cuda.synchronize()
        lg = ref.logits[b].cpu()
        assert_actions_match(res.actions[b, :n].cpu(), ref.actions[b].cpu(), lg, spec, what=f"{cid} score env {b}")
        bar = 2 * 2e-4 * float(lg.abs().max())
        err = float((res.logp[b, :n].double() - ref.logp[b].double()).abs().max())
        worst = max(rel_err(g, w) for g, w in zip(_env_slices(e_pre, spec, b), _env_slices(e_ref, spec, b)))
        _report(f"ragged {cid} env {b} (n = {n}): logp off the dense score's by {err:.1e} (bar {bar:.1e}), state {worst:.1e} (bar 1e-4)")
        assert err <= bar, (cid, b, err, bar)
        assert worst < 1e-4, (cid, b, worst)
    for e in (e_pre, e_score, e_ref):
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# d. per-slot state and the reference layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,lazy", [(c, False) for c in lc.ALL_CASES] + [(c, True) for c in lc.LAZY_CASES])
def test_records_and_past_key_values_follow_the_layout(hip_lib, cid, lazy):
    """After the step-parity run: save_slots of every slot equals the exports concatenated in block order (bit for bit; in the
    lazy mode C within 2e-4 of the tensor's max-abs, as tests/test_gpu_slot_state.py holds the record's plain-FMA window sum);
    export_past_key_values has exactly the layout's keys and the oracle's state; a fresh engine that loaded the
    records and one that imported the past_key_values take the next step bit for bit -- materialised: as the engine they came
    from does."""
    seed = lc.DEEP64_SEED if cid == "deep64" else lc.STEP_SEEDS[(cid, "exercise")][0]
    spec, sd = _model(cid, seed)
    B = lc.step_batch(cid)
    seq = make_inputs(spec, B, lc.STEP_STEPS, seed=1234 + seed, reset_prob=lc.RESET_PROB)
    nxt = make_inputs(spec, B, 1, seed=77, reset_prob=0.0)
    nxt = [(nxt[0][0], nxt[0][1], nxt[0][2], None)]

    def fresh():
        eng = _engine(spec, sd, B)
        if lazy:
            eng.set_state_mode("lazy", 3)
        assert eng.state_mode == ("lazy" if lazy else "materialised")
        return eng

    src = fresh()
    _steps(src, seq)
    if lazy:
        assert float(src.lazy_peek(lc.mlstm_blocks(spec)[0], "pending").max()) >= 3.0, "no window holds a token: the record's window sum shows nothing"
    layout, numel = record_layout(spec)
    assert src.slot_state_numel == numel == src.state_bytes_per_env() // 4 == spec.state_bytes_per_env() // 4
    slots = list(range(B))
    rec = src.save_slots(slots)
    assert rec.shape == (B, numel)
    for block, which, shape, off in layout:
        n = 1
        for s in shape:
            n *= s
        got, want = rec[:, off:off + n], exported_slice(src, spec, block, which, slots)
        if lazy and block not in spec.slstm_at and which == 0:
            assert rel_err(got, want) <= 2e-4, (cid, block, which, rel_err(got, want))
        else:
            assert torch.equal(got, want), (cid, block, which, float((got - want).abs().max()))
    pkv = src.export_past_key_values()
    if spec.backbone == "mamba":
        assert list(pkv) == list(range(spec.n_blocks))
    else:
        assert list(pkv) == [f"block_{i}" for i in range(spec.n_blocks)]
        for i in range(spec.n_blocks):
            want = {"slstm_state" if i in spec.slstm_at else "mlstm_state", "conv_state"}
            assert set(pkv[f"block_{i}"]) == want, (cid, i, set(pkv[f"block_{i}"]))
    if cid in lc.ORACLE_CASES or cid == "deep64":     # (deep64: the oracle of its step-parity run)
        _, ora_state = _oracle((cid, lc.case_scheme(cid), seed, B, False), spec, sd, seq)
        for i in range(spec.n_blocks):
            if spec.backbone == "mamba":
                pairs = [(pkv[i][0], ora_state[i][0]), (pkv[i][1], ora_state[i][1])]
            else:
                got, want = pkv[f"block_{i}"], ora_state[f"block_{i}"]
                pairs = [(got["conv_state"][0], want["conv_state"][0])]
                if i in spec.slstm_at:
                    pairs.append((got["slstm_state"], want["slstm_state"]))
                else:
                    pairs += list(zip(got["mlstm_state"], want["mlstm_state"]))
            for k, (g, w) in enumerate(pairs):
                assert g.shape == w.shape and rel_err(g, w) < 2e-4, (cid, i, k, rel_err(g, w))
        state_vs_oracle(src.export_state_tensor, ora_state, spec, f"{cid} {'lazy' if lazy else 'materialised'}")
    rec = src.save_slots(slots)      # (lazy: behind the exports, which folded every window -- the record is now C_base itself)
    loaded, imported = fresh(), fresh()
    loaded.load_slots(slots, rec)
    assert torch.equal(loaded.save_slots(slots), rec), "a loaded record does not save back bit for bit"
    imported.import_past_key_values(pkv)
    assert torch.equal(imported.save_slots(slots), rec), "records of the imported past_key_values are not the source's"
    out_l, out_i = _steps(loaded, nxt, taps=True), _steps(imported, nxt, taps=True)
    _same(out_l, out_i, f"{cid}: one step behind load_slots against import_past_key_values")
    if not lazy:
        _same(out_l, _steps(src, nxt, taps=True), f"{cid}: one step behind load_slots against the source engine")
    for e in (src, loaded, imported):
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# e. graph replay
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", lc.ALL_CASES)
def test_graph_replay_equals_the_eager_engine(hip_lib, cid):
    """Ten steps on fixed buffers with set_graph_mode(True) (captured at the first, replayed after) against the engine without:
    actions, tokens, taps of every step and the final state, bit for bit (one slice, materialised)."""
    seed = lc.DEEP64_SEED if cid == "deep64" else lc.STEP_SEEDS[(cid, "exercise")][0]
    spec, sd = _model(cid, seed)
    B = lc.step_batch(cid)
    seq = make_inputs(spec, B, 10, seed=1234 + seed, reset_prob=lc.RESET_PROB)
    outs = []
    for graph in (False, True):
        eng = _engine(spec, sd, B)
        eng.set_micro_batches(1)
        eng.set_graph_mode(graph)
        assert eng.state_mode == "materialised"
        d = [torch.empty_like(t).to(DEV) for t in seq[0]]
        rows = []
        for inp in seq:
            for dst, x in zip(d, inp):
                dst.copy_(x)
            a, tok = eng.step(*d)
            torch.cuda.synchronize()
            rows.append([a.clone(), tok.clone(), *eng.taps()])
        outs.append([rows, _state(eng, spec)])
        eng.close()
    _same(outs[1], outs[0], f"{cid} graph replay")


# ---------------------------------------------------------------------------------------------------------------------
# f. env slices, materialised
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,micro", [(c, 2) for c in lc.ALL_CASES] + [("deep64", 8), ("m_64", 8)])
def test_env_slices_match_one_slice(hip_lib, cid, micro):
    """set_micro_batches(2) at 9 env slots (5 + 4) against one slice: actions equal, hidden taps and every state tensor within
    1e-4 (test_micro_batch_pipeline_matches_single_slice's rule: the per-slice kernel choices differ with the slice size).  Mamba:
    slice 1 runs one stage behind slice 0, over 192 stages for m_64.  Eight slices for the two 64-block stacks: more than 512
    ring events inside one call."""
    seed = lc.DEEP64_SEED if cid == "deep64" else lc.STEP_SEEDS[(cid, "exercise")][0]
    spec, sd = _model(cid, seed)
    B = 9
    seq = make_inputs(spec, B, 6, seed=99, reset_prob=lc.RESET_PROB)
    key = ("slices", cid)
    if key not in _CACHE:
        one = _engine(spec, sd, B)
        one.set_micro_batches(1)
        one.set_state_mode("eager")
        rows = _steps(one, seq, taps=True)
        _CACHE[key] = (torch.stack([r[0] for r in rows]), torch.stack([r[3] for r in rows]), _state(one, spec))
        one.close()
    a1, h1, s1 = _CACHE[key]
    eng = _engine(spec, sd, B)
    eng.set_micro_batches(micro)
    eng.set_state_mode("eager")
    rows = _steps(eng, seq, taps=True)
    a, h = torch.stack([r[0] for r in rows]), torch.stack([r[3] for r in rows])
    worst_h = rel_err(h, h1)
    worst_s = max(rel_err(g, w) for g, w in zip(_state(eng, spec), s1))
    _report(f"slices {cid} micro {micro}: {int((a != a1).sum())} actions differ, hidden {worst_h:.1e}, state {worst_s:.1e} (bars 1e-4)")
    assert torch.equal(a, a1), (cid, micro, int((a != a1).sum()))
    assert worst_h < 1e-4 and worst_s < 1e-4, (cid, micro, worst_h, worst_s)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# g. the depth boundary
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", ["xlstm", "mamba"])
def test_65_blocks_are_refused_and_64_accepted(hip_lib, backbone):
    """validate_config (csrc/engine.hip), engine_limits and make_config agree on LRAM_MAX_BLOCKS = 64, each with a message that
    names n_blocks."""
    from lram_amd.config import engine_limits
    from lram_amd.engine import Engine, make_config
    cid = "deep64" if backbone == "xlstm" else "m_64"
    spec = lc.case_spec(cid)
    assert spec.n_blocks == lc.MAX_BLOCKS and engine_limits(spec) == []
    too_deep = ModelSpec(**{**(lc.XLSTM_CASES if backbone == "xlstm" else lc.MAMBA_CASES)[cid], "n_blocks": 65})
    assert engine_limits(too_deep) == ["n_blocks 65 must be in 1..64"]
    with pytest.raises(ValueError, match="n_blocks 65"):
        Engine(too_deep, {}, 2, device=DEV)
    cfg = make_config(spec)
    h = ctypes.c_void_p()
    for n, ok in ((65, False), (0, False), (64, True)):
        cfg.n_blocks = n
        rc = hip_lib.lram_create(ctypes.byref(cfg), 0, ctypes.byref(h))
        assert (rc == 0) == ok, (n, rc)
        if ok:
            hip_lib.lram_destroy(h)
        else:
            assert "n_blocks" in hip_lib.lram_last_error().decode(), hip_lib.lram_last_error()
