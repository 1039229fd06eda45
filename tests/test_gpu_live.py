"""Live prefix on the GPU, through the C ABI via Engine (lram_set_live / lram_state_swap_slots; csrc/slot_state.hip,
csrc/mlstm_lazy.hip): an engine that never parks is bit-identical to one that never heard of parking; parked slots are left alone
(the lazy bookkeeping follows the step parity, folds keep the host bounds true); resumed envs continue as if they had never been
parked; live slots compute what they always computed and nothing is touched beyond them; a swap exchanges two slots bit for bit;
images / slot table, sampling, graph replay, the Mamba repeated forwards and the refusals; the scheduler end to end.

Geometries: those of tests/test_gpu_slot_state.py -- tiny xLSTM and tiny Mamba at 12 slots, 16M at 32 (materialised) and at 160
slots (lazy, fused scores, period 13), 206M at 24 slots (lazy, head dim 640: score kernel; two envs against the oracle).

One twin engine per geometry runs all TOTAL steps on the full batch, never parked.  The engine under test is fed, per ENV, a
prefix of what the twin feeds that env: a live env every step; a parked env the 30 warm-up steps, nothing while parked, then the
twin's steps 30 .. 49 -- so the k-th output of every env has the twin's k-th output of that env to be held against, whatever K.
The CPU oracle runs once per geometry on a few envs over the same sequence.

Bars (the project's own): bit-identical where stated; otherwise 2e-4 relative on hidden state (helpers.rel_err), actions through
helpers.assert_actions_match with ZERO ties on the committed seeds, hidden state against the oracle through
helpers.assert_close_or_as_close_as_fp32_oracle with at most 5 % of the rows on the float64 rule.  The dispatcher picks kernels
by row count, so a parked engine and its twin are not asked to agree bit for bit."""
import ctypes
import functools

import pytest
import torch

from lram_amd import init_state_dict, preset
from oracle import dt_ref
from tests.helpers import (Fp64Oracle, assert_actions_match, assert_close_or_as_close_as_fp32_oracle, make_inputs, rel_err,
                           relaxed_rows_fraction, relaxed_rows_reset)
from tests.slot_state_helpers import force_mask, record_layout

pytestmark = pytest.mark.gpu

PERIOD = 13
WARM, RESUME = 30, 20
KS = (1, 2, 13, 27)
TOTAL = WARM + max(KS) + RESUME
# name -> (preset, slots, lazy?, n_live of the park / resume scenario, slot reset in the last warm-up step, weight seed, input seed,
#          env rows the oracle follows: live ones, parked ones -- also the pairs of the swap scenario)
# Lazy geometries, fold class = slot % 13: after 30 steps class 9 is due NEXT (slots 9 and 22 are never reset: 39 tokens pending)
# and class 10 (slot 23) has JUST folded; the parked tail holds 22, 23, the slot reset in the last step and the rest of class 9.
GEOMS = {
    "xlstm_tiny": ("xlstm_tiny", 12, False, 5, 9, 171, 131, [0, 3], [9, 11]),
    "mamba_tiny": ("mamba_tiny", 12, False, 5, 9, 172, 132, [0, 3], [9, 11]),
    "xlstm_16m_32": ("xlstm_16m", 32, False, 13, 20, 174, 134, [0, 7], [20, 31]),
    "xlstm_16m_160": ("xlstm_16m", 160, True, 20, 40, 173, 141, [9, 0], [23, 40, 22]),
    "xlstm_206m_24": ("xlstm_206m", 24, True, 12, 17, 175, 135, [9], [22]),
}
FULL_WINDOW = (9, 22)
KEYS = ("a", "tok", "hid", "logits")


@functools.lru_cache(maxsize=None)
def _geom(name):
    """(spec, weights, slots, lazy, n_live, reset slot, inputs of all TOTAL steps, followed envs); shared: read, never written."""
    pre, B, lazy, n_live, zslot, wseed, iseed, live_rows, parked_rows = GEOMS[name]
    spec = preset(pre)
    sd = init_state_dict(spec, seed=wseed)
    seq = make_inputs(spec, B, TOTAL, seed=iseed, reset_prob=0.06)
    force_mask(seq, zslot, steps_on=[WARM - 1])
    if lazy:
        for s in FULL_WINDOW:
            force_mask(seq, s, steps_off=range(1, TOTAL))
    return spec, sd, B, lazy, n_live, zslot, seq, live_rows + parked_rows


def _engine(spec, sd, B, lazy):
    from lram_amd.engine import Engine
    eng = Engine(spec, sd, B, device="cuda:0")
    assert eng.state_mode == ("lazy" if lazy else "materialised"), "the geometry no longer selects the intended state mode"
    return eng


def _new_rec():
    return {k: [] for k in KEYS + ("emb",)}


def _step(eng, inputs, rec, out=None):
    """One step on rows the caller has cut; appends CPU copies of actions, tokens and the three taps."""
    obs, rtg, rew, mask = (x.cuda() for x in inputs)
    a, tok = eng.step(obs, rtg, rew, mask) if out is None else eng.step(obs, rtg, rew, mask, out_actions=out[0], out_tokens=out[1])
    emb, hid, logits = eng.taps()
    for k, v in zip(KEYS + ("emb",), (a, tok, hid, logits, emb)):
        rec[k].append(v.cpu())


def _rows(step, lo, hi=None):
    return tuple(x[lo:hi].clone() for x in step)


def _mblocks(spec):
    return [i for i in range(spec.n_blocks) if i not in spec.slstm_at]


def _peek(eng, spec):
    m = _mblocks(spec)
    return [eng.lazy_peek(m[0], "pending").cpu(), eng.lazy_peek(m[0], "g").cpu(), eng.lazy_peek(m[-1], "g").cpu()]


@functools.lru_cache(maxsize=None)
def _twin(name):
    spec, sd, B, lazy, _, _, seq, _ = _geom(name)
    T = _engine(spec, sd, B, lazy)
    rec = _new_rec()
    for t in range(TOTAL):
        _step(T, seq[t], rec)
    out = {k: torch.stack(v) for k, v in rec.items()}
    out["final"] = T.save_slots(list(range(B))).cpu()
    T.close()
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The fp32 and float64 oracles on the followed envs over the twin's sequence: per step (actions, logits, hidden, hidden64)."""
    spec, sd, _, _, _, _, seq, rows = _geom(name)
    ora, ora64 = dt_ref.OraclePolicy(spec, sd), Fp64Oracle(spec, sd)
    out = []
    for obs, rtg, rew, mask in seq:
        ref, dbg = ora.step(obs[rows], rtg[rows], rew[rows], mask[rows], return_debug=True)
        _, dbg64 = ora64.step(obs[rows], rtg[rows], rew[rows], mask[rows], return_debug=True)
        out.append((ref, dbg["logits"], dbg["hidden"], dbg64["hidden"]))
    return out


def _hold(name, spec, got, t_twin, rows_got, rows_twin, what, exact=False):
    """Rows of one step of the engine under test against rows of the twin's step t_twin: the bars, or bit for bit.  Returns the
    hidden-state error."""
    tw = _twin(name)
    if exact:
        for k in KEYS:
            assert torch.equal(got[k][rows_got], tw[k][t_twin][rows_twin]), (what, k)
        return 0.0
    lg = tw["logits"][t_twin][rows_twin].reshape(len(rows_twin), spec.act_dim, spec.n_vocab)
    ties = assert_actions_match(got["a"][rows_got], tw["a"][t_twin][rows_twin], lg, spec, what=what)
    assert ties == 0, (what, ties)
    err = rel_err(got["hid"][rows_got], tw["hid"][t_twin][rows_twin])
    assert err <= 2e-4, (what, err)
    return err


def _hold_oracle(name, spec, got, t_ora, row, what):
    """One followed env of one step against the oracle's step t_ora of that env."""
    rows = GEOMS[name][7] + GEOMS[name][8]
    ref, logits, hid, hid64 = _oracle(name)[t_ora]
    i = rows.index(row[1])
    ties = assert_actions_match(got["a"][[row[0]]], ref[[i]], logits[[i]].reshape(1, spec.act_dim, spec.n_vocab), spec, what=what)
    assert_close_or_as_close_as_fp32_oracle(got["hid"][[row[0]]], hid[[i]], hid64[[i]], what=what)
    return ties


def _at(rec, j):
    return {k: rec[k][j] for k in KEYS}


# ---------------------------------------------------------------------------------------------------------------------
# 1. never parked
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMS))
def test_never_parked_is_bit_identical(hip_lib, name):
    """set_live(batch) at step 0 changes nothing: actions, tokens, the three taps of every step and the final records equal the
    twin's bit for bit."""
    spec, sd, B, lazy, _, _, seq, _ = _geom(name)
    A = _engine(spec, sd, B, lazy)
    assert A.live == B
    A.set_live(B)
    assert A.live == B and A.lib.lram_get_live(A._h) == B
    rec = _new_rec()
    for t in range(TOTAL):
        _step(A, seq[t], rec)
    tw = _twin(name)
    for k in KEYS + ("emb",):
        assert torch.equal(torch.stack(rec[k]), tw[k]), (name, k)
    assert torch.equal(A.save_slots(list(range(B))).cpu(), tw["final"]), name
    A.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2 - 4. one run per (geometry, n_live, K): warm up, park the tail, K live steps, resume, 20 steps of all slots
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parked_run(name, n_live, K):
    spec, sd, B, lazy, _, _, seq, _ = _geom(name)
    A = _engine(spec, sd, B, lazy)
    warm = _new_rec()
    for t in range(WARM):
        _step(A, seq[t], warm)
    parked = list(range(n_live, B))
    r = {"before": A.save_slots(parked).cpu(), "peek_before": _peek(A, spec) if lazy else None}
    A.set_live(n_live)
    assert A.live == n_live
    # caller buffers of `batch` rows pre-filled with NaN / a sentinel: the call gets the view of the live rows
    out_a = torch.full((B, spec.act_dim), float("nan"), device="cuda:0")
    out_t = torch.full((B, spec.act_dim), -7, dtype=torch.int32, device="cuda:0")
    live = _new_rec()
    pend = 0.0
    for k in range(K):
        _step(A, _rows(seq[WARM + k], 0, n_live), live, out=(out_a[:n_live], out_t[:n_live]))   # (a mask of exactly n_live bytes)
        if lazy:
            pend = max(pend, float(A.lazy_peek(_mblocks(spec)[0], "pending")[n_live:].max()))
    torch.cuda.synchronize()
    r["tail_untouched"] = bool(torch.isnan(out_a[n_live:]).all()) and bool((out_t[n_live:] == -7).all())
    r["live_rows_written"] = not bool(torch.isnan(out_a[:n_live]).any())
    r["after"] = A.save_slots(parked).cpu()
    r["peek_after"] = _peek(A, spec) if lazy else None
    A.set_live(B)
    res = _new_rec()
    for j in range(RESUME):
        step = tuple(torch.cat([x[:n_live], y[n_live:]]) for x, y in zip(seq[WARM + K + j], seq[WARM + j]))
        _step(A, step, res)
        if lazy:
            pend = max(pend, float(A.lazy_peek(_mblocks(spec)[0], "pending").max()))
    r["pending_max"] = pend
    r["live"], r["resume"] = live, res
    A.close()
    return r


def _check_against_twin_and_oracle(name, n_live, K):
    spec, _, B, _, _, _, _, followed = _geom(name)
    r = _parked_run(name, n_live, K)
    lo, hi = list(range(n_live)), list(range(n_live, B))
    worst, ties = 0.0, 0
    relaxed_rows_reset()
    for k in range(K):
        got = _at(r["live"], k)
        assert got["a"].shape[0] == got["hid"].shape[0] == got["logits"].shape[0] == n_live, "outputs are not the live rows"
        worst = max(worst, _hold(name, spec, got, WARM + k, lo, lo, f"{name} n_live {n_live}: live step {k}"))
        for row in followed:
            if row < n_live:
                ties += _hold_oracle(name, spec, got, WARM + k, (row, row), f"{name} n_live {n_live}: live step {k} env {row} vs oracle")
    for j in range(RESUME):
        got = _at(r["resume"], j)
        worst = max(worst, _hold(name, spec, got, WARM + K + j, lo, lo, f"{name} n_live {n_live} K {K}: resumed step {j}, live envs"))
        worst = max(worst, _hold(name, spec, got, WARM + j, hi, hi, f"{name} n_live {n_live} K {K}: resumed step {j}, parked envs"))
        for row in followed:
            t = WARM + K + j if row < n_live else WARM + j
            ties += _hold_oracle(name, spec, got, t, (row, row), f"{name} n_live {n_live} K {K}: resumed step {j} env {row} vs oracle")
    print(f"[live] {name} n_live {n_live} K {K}: hidden vs twin {worst:.3e} (bar 2e-4), oracle ties {ties}, "
          f"rows on the float64 rule {relaxed_rows_fraction():.2%}, pending max {r['pending_max']:.0f}")
    assert ties == 0, (name, ties)
    assert relaxed_rows_fraction() <= 0.05, (name, relaxed_rows_fraction())
    assert r["pending_max"] <= 48.0, (name, r["pending_max"])
    assert r["tail_untouched"] and r["live_rows_written"], f"{name}: rows >= n_live of the caller's buffers were written"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(GEOMS))
def test_parked_slots_are_left_alone(hip_lib, name, K):
    """The records of the parked slots before and after K live steps: bit-identical in materialised mode; in lazy mode every
    tensor but C bit-identical and C within 2e-4 of max-abs (folds keep covering parked slots: C is folded at most once), the
    pending count never beyond the window.  K = 1 is the case that catches the ping-pong side."""
    spec, _, B, lazy, n_live, zslot, _, _ = _geom(name)
    r = _parked_run(name, n_live, K)
    if lazy:
        pend = r["peek_before"][0]
        assert all(int(pend[s]) == 3 * PERIOD for s in FULL_WINDOW), "slots 9 / 22 do not hold 39 tokens: the case shows nothing"
        assert n_live <= 22 and zslot >= n_live and int(pend[zslot]) <= 3, "the parked tail misses the slots the case is about"
        assert float(r["peek_after"][0][n_live:].max()) <= 48.0
        if K < PERIOD:
            assert float(r["peek_after"][0][n_live:].max()) > 0.0, "every parked window is empty: the ping-pong side carries nothing"
        # what no fold touches is carried over bit for bit: pending counts and scales of parked slots whose class was not due
        due = {(PERIOD - (WARM + k) % PERIOD) % PERIOD for k in range(K)}
        keep = [b for b in range(n_live, B) if b % PERIOD not in due]
        for x, y in zip(r["peek_before"], r["peek_after"]):
            assert torch.equal(x[keep], y[keep]), f"{name} K {K}: bookkeeping of parked slots changed"
    worst = 0.0
    for block, which, shape, off in record_layout(spec)[0]:
        n = 1
        for s in shape:
            n *= s
        got, want = r["after"][:, off:off + n], r["before"][:, off:off + n]
        if lazy and block not in spec.slstm_at and which == 0:
            worst = max(worst, rel_err(got, want))
            assert rel_err(got, want) <= 2e-4, (name, K, block, rel_err(got, want))
        else:
            assert torch.equal(got, want), (name, K, block, which)
    print(f"[live] {name} K {K}: parked records, worst lazy C change {worst:.3e} of max-abs (bar 2e-4)")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(GEOMS))
def test_resumed_envs_continue_where_they_stopped(hip_lib, name, K):
    """set_live(batch) after K live steps, then 20 steps of all slots: the k-th output of every env against the twin that never
    parked, and the followed envs against the CPU oracle on their own input history.  20 steps run beyond one fold period: a
    wrong host bound would show as an overflowed window."""
    _check_against_twin_and_oracle(name, _geom(name)[4], K)


def _live_counts(name):
    B = GEOMS[name][1]
    return sorted({1, 5, B - 1} | ({81} if name == "xlstm_16m_160" else set()))


@pytest.mark.parametrize("name,n_live", [(n, k) for n in GEOMS for k in _live_counts(n)])
def test_live_slots_while_others_are_parked(hip_lib, name, n_live):
    """Slots below n_live against the twin and the oracle while the others are parked (13 steps: one fold period), at n_live 1, 5,
    batch - 1, and 81 of 160 (two fold classes straddle the boundary).  The caller's action and token buffers beyond n_live
    stay as they were; the reset mask holds exactly n_live bytes."""
    _check_against_twin_and_oracle(name, n_live, 13)


# ---------------------------------------------------------------------------------------------------------------------
# 5. swap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMS))
def test_swap_exchanges_two_slots_bit_for_bit(hip_lib, name):
    """After one swap record[a] is the old record[b] and vice versa, lazy included; every other slot is untouched; a second swap
    restores everything (records and lazy_peek).  Then the swapped slots are fed each other's inputs for 20 steps: bit-identical
    to the twin in materialised mode, within the bars in lazy mode (another fold class), and the CPU oracle on the exchanged
    histories; every slot not listed stays bit-identical to the twin.  Refused lists leave the state as it was."""
    from lram_amd.engine import LramError
    spec, sd, B, lazy, _, _, seq, followed = _geom(name)
    a, b = GEOMS[name][7], GEOMS[name][8][:len(GEOMS[name][7])]
    everyone = list(range(B))
    others = [s for s in everyone if s not in a + b]
    A = _engine(spec, sd, B, lazy)
    rec = _new_rec()
    for t in range(WARM):
        _step(A, seq[t], rec)
    rec0, peek0 = A.save_slots(everyone), (_peek(A, spec) if lazy else [])
    # refusals first: Python's check, then the C entry's own
    for x, y in (([a[0], a[0]], [b[0], others[0]]), ([a[0]], [a[0]]), ([a[0]], [B]), ([-1], [b[0]])):
        with pytest.raises(ValueError):
            A.swap_slots(x, y)
        arr_x, arr_y = (ctypes.c_int32 * len(x))(*x), (ctypes.c_int32 * len(y))(*y)
        assert A.lib.lram_state_swap_slots(A._h, arr_x, arr_y, len(x), None) != 0
        assert b"lram_state_swap_slots" in A.lib.lram_last_error()
    assert torch.equal(A.save_slots(everyone), rec0), f"{name}: a refused swap changed the state"
    A.swap_slots([], [])
    A.swap_slots(a, b)
    rec1, peek1 = A.save_slots(everyone), (_peek(A, spec) if lazy else [])
    assert torch.equal(rec1[a], rec0[b]) and torch.equal(rec1[b], rec0[a]), f"{name}: swapped records are not exchanged bit for bit"
    assert torch.equal(rec1[others], rec0[others]), f"{name}: a swap touched a slot it does not list"
    for p0, p1 in zip(peek0, peek1):
        assert torch.equal(p1[a], p0[b]) and torch.equal(p1[b], p0[a]) and torch.equal(p1[others], p0[others]), name
    A.swap_slots(b, a)
    assert torch.equal(A.save_slots(everyone), rec0), f"{name}: swapping twice is not the identity"
    for p0, p2 in zip(peek0, _peek(A, spec) if lazy else []):
        assert torch.equal(p0, p2), name
    A.swap_slots(a, b)
    ties, worst = 0, 0.0
    relaxed_rows_reset()
    for j in range(RESUME):
        step = tuple(x.clone() for x in seq[WARM + j])
        for x, src in zip(step, seq[WARM + j]):
            x[a], x[b] = src[b], src[a]
        one = _new_rec()
        _step(A, step, one)
        got = _at(one, 0)
        _hold(name, spec, got, WARM + j, others, others, f"{name} swap: step {j}, unlisted slots", exact=True)
        worst = max(worst, _hold(name, spec, got, WARM + j, a + b, b + a, f"{name} swap: step {j}", exact=not lazy))
        for s, e in zip(a + b, b + a):
            ties += _hold_oracle(name, spec, got, WARM + j, (s, e), f"{name} swap: step {j}, slot {s} holding env {e} vs oracle")
    print(f"[live] {name} swap: hidden vs twin {worst:.3e} (bar 2e-4), oracle ties {ties}, float64 rule {relaxed_rows_fraction():.2%}")
    assert ties == 0 and relaxed_rows_fraction() <= 0.05, (name, ties, relaxed_rows_fraction())
    if lazy:
        assert float(A.lazy_peek(_mblocks(spec)[0], "pending").max()) <= 48.0
    A.close()


def test_swap_across_the_parked_boundary_and_fold_classes(hip_lib):
    """160 slots, lazy, 20 live: slot 9 (class 9, due next, 39 tokens pending) <-> slot 23 (class 10, just folded, parked).  Env 23
    goes on in slot 9 for 5 steps while env 9 waits in slot 23 with its full window in a class whose bound said "empty"; then all
    slots run 20 steps -- beyond the overflow of that window -- and both envs follow the CPU oracle on their own histories."""
    name, n_live, P = "xlstm_16m_160", 20, 5
    spec, sd, B, lazy, _, _, seq, _ = _geom(name)
    A = _engine(spec, sd, B, lazy)
    rec = _new_rec()
    for t in range(WARM):
        _step(A, seq[t], rec)
    A.set_live(n_live)
    A.swap_slots([9], [23])
    ties = 0
    relaxed_rows_reset()
    for k in range(P):
        step = _rows(seq[WARM + k], 0, n_live)
        for x, src in zip(step, seq[WARM + k]):
            x[9] = src[23]
        one = _new_rec()
        _step(A, step, one)
        ties += _hold_oracle(name, spec, _at(one, 0), WARM + k, (9, 23), f"swap across the boundary: live step {k}, env 23 in slot 9")
    assert int(A.lazy_peek(0, "pending")[23]) == 3 * PERIOD, "the parked full window did not stay as it was"
    A.set_live(B)
    pend = 0.0
    for j in range(RESUME):
        step = tuple(torch.cat([x[:n_live], y[n_live:]]) for x, y in zip(seq[WARM + P + j], seq[WARM + j]))
        for x, went_on, waited in zip(step, seq[WARM + P + j], seq[WARM + j]):
            x[9], x[23] = went_on[23], waited[9]
        one = _new_rec()
        _step(A, step, one)
        pend = max(pend, float(A.lazy_peek(0, "pending").max()))
        ties += _hold_oracle(name, spec, _at(one, 0), WARM + P + j, (9, 23), f"swap across the boundary: step {j}, env 23 in slot 9")
        ties += _hold_oracle(name, spec, _at(one, 0), WARM + j, (23, 9), f"swap across the boundary: step {j}, env 9 in slot 23")
    print(f"[live] swap across the boundary: oracle ties {ties}, float64 rule {relaxed_rows_fraction():.2%}, pending max {pend:.0f}")
    assert ties == 0 and relaxed_rows_fraction() <= 0.05 and pend <= 48.0, (ties, relaxed_rows_fraction(), pend)
    A.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. surfaces
# ---------------------------------------------------------------------------------------------------------------------
def _bars(spec, a, lg_ref, a_ref, hid, hid_ref, what):
    assert assert_actions_match(a.cpu(), a_ref.cpu(), lg_ref.cpu().reshape(a.shape[0], spec.act_dim, spec.n_vocab), spec, what=what) == 0
    assert rel_err(hid, hid_ref) <= 2e-4, (what, rel_err(hid, hid_ref))


def test_images_and_slot_table_on_a_live_prefix(hip_lib):
    """step_images on the live frames, and step_slots with a table of image and vector slots handed the frames of the image
    slots below n_live only, against twins that step every slot."""
    from lram_amd.engine import Engine
    spec, B, n_live = preset("xlstm_tiny"), 8, 5
    sd = init_state_dict(spec, seed=181, with_image_encoder=True)
    img = make_inputs(spec, B, 12, seed=141, reset_prob=0.1, image=True)
    vec = make_inputs(spec, B, 12, seed=142, reset_prob=0.1)
    image = [True, False, False, True, True, False, True, False]           # image slots 0, 3, 4 are live, 6 is parked
    acts = [1, 3, 2, 1, 3, 3, 2, 1]
    fr = [i for i in range(B) if image[i]]
    fr_live = [i for i in fr if i < n_live]
    for mode in ("images", "slots"):
        A, T = Engine(spec, sd, B, device="cuda:0"), Engine(spec, sd, B, device="cuda:0")
        for e in (A, T):
            if mode == "slots":
                e.set_slot_table([False] * B, acts, image)
        for t in range(12):
            n = B if t < 4 else n_live
            if t == 4:
                A.set_live(n_live)
            frames, (obs, rtg, rew, mask) = img[t][0], vec[t]
            if mode == "images":
                a, _ = A.step_images(frames[:n].cuda(), rtg[:n].cuda(), rew[:n].cuda(), mask[:n].cuda())
                ta, _ = T.step_images(frames.cuda(), rtg.cuda(), rew.cuda(), mask.cuda())
            else:
                a, _ = A.step_slots(obs[:n].cuda(), frames[fr if n == B else fr_live].cuda(), rtg[:n].cuda(), rew[:n].cuda(), mask[:n].cuda())
                ta, _ = T.step_slots(obs.cuda(), frames[fr].cuda(), rtg.cuda(), rew.cuda(), mask.cuda())
            assert a.shape[0] == n
            (_, hid, _), (_, thid, tlg) = A.taps(), T.taps()
            _bars(spec, a, tlg[:n], ta[:n], hid, thid[:n], f"{mode} step {t}")
        if mode == "slots":
            with pytest.raises(ValueError):
                A.step_slots(vec[0][0][:n_live].cuda(), img[0][0][fr].cuda(), vec[0][1][:n_live].cuda(), vec[0][2][:n_live].cuda())
        A.close(), T.close()


@pytest.mark.parametrize("name", ["xlstm_16m_32", "xlstm_16m_160", "mamba_tiny"])
def test_a_live_slot_draws_what_it_would_have_drawn(hip_lib, name):
    """Sampling armed, the tail parked: every call is one draw of the engine-wide counter, and a live slot's tokens are the draw of
    ITS OWN Philox stream (slot index) at that count on its logits row -- what the same slot of a never-parked engine draws."""
    from lram_amd import engine as E
    spec, sd, B, lazy, n_live, _, seq, _ = _geom(name)
    A = _engine(spec, sd, B, lazy)
    A.set_sampling(temperature=1.0, seed=2024)
    rec = _new_rec()
    for t in range(4):
        _step(A, seq[t], rec)
    A.set_live(n_live)
    for t in range(4, 8):
        _step(A, _rows(seq[t], 0, n_live), rec)
        u = E.sample_uniforms(2024, 0, B, spec.act_dim, t, device=A.device).reshape(B, spec.act_dim)[:n_live]
        want = E.sample_tokens(rec["logits"][-1].cuda().reshape(n_live * spec.act_dim, spec.n_vocab), u.reshape(-1), temperature=1.0)
        assert torch.equal(rec["tok"][-1].reshape(-1), want.cpu().reshape(-1)), (name, t)
        lp = A.last_logp(rec["tok"][-1].cuda(), over="sampled")
        assert lp.shape == (n_live, spec.act_dim) and bool(torch.isfinite(lp).all())
    assert A.sampling["draws"] == 8
    A.close()


@pytest.mark.parametrize("pre", ["xlstm_tiny", "mamba_tiny"])
def test_graph_replay_across_a_change_of_the_live_count(hip_lib, pre):
    """Graph mode: the live count is one more field of the captured step's key -- 4 steps of 4 slots, 4 of 2, 4 of 4 again, from
    fixed buffers, give the bits the same sequence gives in eager mode."""
    from lram_amd.engine import Engine
    spec, B = preset(pre), 4
    sd = init_state_dict(spec, seed=191)
    seq = make_inputs(spec, B, 12, seed=151, reset_prob=0.1)
    outs = []
    for graph in (False, True):
        eng = Engine(spec, sd, B, device="cuda:0")
        eng.set_graph_mode(graph)
        bufs = tuple(x.cuda() for x in seq[0])
        rec = []
        for t in range(12):
            n = 2 if 4 <= t < 8 else B
            if t in (4, 8):
                eng.set_live(n)
            for d, x in zip(bufs, seq[t]):
                d.copy_(x)                                       # fixed pointers: the step replays
            a, tok = eng.step(*(d[:n] for d in bufs))
            rec.append(torch.cat([a.clone().reshape(-1), tok.clone().float().reshape(-1), eng.taps()[2].reshape(-1)]))
        torch.cuda.synchronize()
        outs.append(rec + [eng.save_slots(list(range(B))).reshape(-1)])
        eng.close()
    for t, (x, y) in enumerate(zip(*outs)):
        assert torch.equal(x, y), (pre, t)


def test_mamba_repeated_forwards_on_a_live_prefix(hip_lib):
    spec, sd, B, _, n_live, _, seq, _ = _geom("mamba_tiny")
    A, T = _engine(spec, sd, B, False), _engine(spec, sd, B, False)
    for e in (A, T):
        e.set_compat_mode(spec.act_dim, False)
    for t in range(10):
        n = B if t < 4 else n_live
        if t == 4:
            A.set_live(n_live)
        a, _ = A.step(*(x[:n].cuda() for x in seq[t]))
        ta, _ = T.step(*(x.cuda() for x in seq[t]))
        (_, hid, _), (_, thid, tlg) = A.taps(), T.taps()
        _bars(spec, a, tlg[:n], ta[:n], hid, thid[:n], f"repeated forwards step {t}")
    A.close(), T.close()


@pytest.mark.parametrize("name", ["xlstm_16m_160", "mamba_tiny"])
def test_stored_contexts_and_encoder_calls_are_refused_while_parked(hip_lib, name):
    from lram_amd.engine import LramError
    spec, sd, B, lazy, n_live, _, seq, _ = _geom(name)
    A = _engine(spec, sd, B, lazy)
    rec = _new_rec()
    for t in range(6):
        _step(A, seq[t], rec)
    A.set_live(n_live)
    before = A.save_slots(list(range(B)))
    obs = torch.stack([seq[t][0] for t in range(3)], 1).contiguous().cuda()
    rtg = torch.stack([seq[t][1] for t in range(3)], 1).contiguous().cuda()
    rew = torch.zeros(B, 3, device="cuda:0")
    emb = torch.zeros(B, 3, spec.d_model, device="cuda:0")
    ragged = [3] * (B - 1) + [2]
    for call in (lambda: A.prefill(obs, rtg, rew), lambda: A.prefill(obs, rtg, rew, lengths=ragged),
                 lambda: A.score(obs, rtg, rew, want=("actions",)), lambda: A.score(obs, rtg, rew, want=("actions",), lengths=ragged),
                 lambda: A.encoder_step(emb)):
        with pytest.raises(LramError, match="parked"):
            call()
    # ... and the C entries themselves, past Python's own check
    lib, h, P, st = A.lib, A._h, (lambda t: ctypes.c_void_p(t.data_ptr())), None
    n_arr = (ctypes.c_int32 * B)(*ragged)
    act = torch.zeros(B, 3, spec.act_dim, device="cuda:0")
    out = torch.empty_like(emb)
    for rc in (lib.lram_prefill(h, P(obs), 0, P(rtg), P(rew), 3, None, 0, None, None, st),
               lib.lram_prefill_ragged(h, P(obs), 0, P(rtg), P(rew), 3, n_arr, None, 0, None, None, st),
               lib.lram_score(h, P(obs), 0, P(rtg), P(rew), 3, None, 0, None, None, None, 0, 1.0, P(act), None, None, None, st),
               lib.lram_score_ragged(h, P(obs), 0, P(rtg), P(rew), 3, n_arr, None, 0, None, None, None, 0, 1.0, P(act), None, None,
                                     None, st),
               lib.lram_encoder_step(h, P(emb), 3, None, P(out), st)):
        assert rc != 0 and b"parked" in lib.lram_last_error(), lib.lram_last_error()
    assert torch.equal(A.save_slots(list(range(B))), before), f"{name}: a refused call changed the state"
    with pytest.raises(LramError, match="n_live must be in"):
        A.set_live(0)
    with pytest.raises(LramError, match="n_live must be in"):
        A.set_live(B + 1)
    assert A.live == n_live
    A.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the scheduler end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluation_parks_the_envs_that_have_finished(hip_lib):
    """evaluate_policy_batched on SyntheticVecEnv, 12 envs staggered over episodes of 14 steps, 18 episodes: with park_finished
    the same episode counts and lengths, and the same returns EXACTLY -- the env's reward is 1 per step whatever the action, so
    the bound the action bars leave on a return is 0.  The engine ends with one live slot."""
    from lram_amd.agent import RecurrentAgent
    from lram_amd.rollout import SyntheticVecEnv, evaluate_policy_batched
    spec, n = preset("xlstm_tiny"), 12
    sd = init_state_dict(spec, seed=201)
    out = []
    for park in (False, True):
        env = SyntheticVecEnv(n, obs_dim=10, act_dim=spec.act_dim, ep_len=14, device="cuda:0", seed=5)
        agent = RecurrentAgent(spec, sd, n_envs=n, device="cuda:0", target_return=14.0)
        out.append(evaluate_policy_batched(agent, env, n_eval_episodes=18, return_episode_rewards=True, park_finished=park))
        assert agent.engine.live == (1 if park else n)
        assert len(agent.active) == (1 if park else n)
        agent.engine.close()
    assert out[0][1] == out[1][1] and len(out[0][1]) == 18, "episode counts / lengths differ"
    assert out[0][0] == out[1][0], "returns differ"
