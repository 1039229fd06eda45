"""GPU: the window ring with a position per env slot -- Engine.set_window_slots("own") (a window step on the live prefix),
copy_window_slots / swap_window_slots / save_window_slots / load_window_slots, and RecurrentAgent(window_slots="own") under
evaluate_policy_batched(park_finished=True).

Bars (none tuned to the code under test):
  * bookkeeping: every slot's window from window() against a plain-Python list model of what that env has pushed (tests/
    window_cases.History, stepped on the live prefix), bit for bit, after every call; a parked slot's window, count and exported
    recurrent state bit for bit what they were before the call;
  * against the entry it rides on: the live slots' actions, tokens and logits bit for bit those of Engine.prefill under
    set_context_rows("live") on the same engine over window()'s live rows;
  * context_counts()["env_timesteps"] grows by exactly live x K per call in pad mode "reference";
  * between engines of different live counts (test 5) other kernel instances may run: a row's logits within rel_err 2e-4
    (window_cases.LOGIT_TOL, the stored-context bar), tokens equal where the top-2 logit gap is at least 1e-3."""
import ctypes

import pytest
import torch

from lram_amd import init_state_dict
from lram_amd.engine import LramError, _stream_ptr
from tests import window_cases as wc
from tests.context_cases import DEV, NAN, bits, export_state, new_engine, same_state, state_kinds
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu


def _dev(*ts):
    return tuple(t.to(DEV).contiguous() for t in ts)


def _logits(eng):
    lg = eng.taps()[2].clone()
    torch.cuda.synchronize()
    return lg


class SlotHistory(wc.History):
    """window_cases.History whose step runs the first `live` slots only, with the movers' effect on whole histories."""

    def step_live(self, live, vec, rtg, prev, reset=None, relabel=None, keep=None):
        part = wc.History(live, self.K)
        part.rows = self.rows[:live]      # (the same lists: stepped in place)
        part.step(vec, rtg, prev, reset=reset, relabel=relabel, keep=keep)

    def swap(self, a, b):
        for x, y in zip(a, b):
            self.rows[x], self.rows[y] = self.rows[y], self.rows[x]

    def copy(self, src, dst):
        for x, y in zip(src, dst):
            self.rows[y] = [[v.clone(), g, r] for v, g, r in self.rows[x]]

    def tensors_of(self, width):
        """tensors() that does not need slot 0 to hold an entry."""
        vec = torch.zeros(self.B, self.K, width)
        rtg, rew = torch.zeros(self.B, self.K), torch.zeros(self.B, self.K)
        for b, h in enumerate(self.rows):
            for i, (v, g, r) in enumerate(h):
                vec[b, self.K - len(h) + i], rtg[b, self.K - len(h) + i], rew[b, self.K - len(h) + i] = v, float(g), float(r)
        return vec, rtg, rew


def _window(eng):
    w = eng.window()
    torch.cuda.synchronize()
    return w


def _same_window(eng, hist, width, what):
    w = _window(eng)
    assert w.counts == hist.counts, what
    for got, want, n in zip((w.emb, w.rtg, w.reward), hist.tensors_of(width), ("emb", "rtg", "reward")):
        assert torch.equal(bits(got.cpu()), bits(want)), f"{what}: {n} differs from the list model"
    return w


def _parked_state(state, spec, lo):
    """Rows [lo, B) of every exported state tensor (the sLSTM state is [4, B, D])."""
    out, i = [], 0
    for blk in range(spec.n_blocks):
        for w in state_kinds(spec, blk):
            t = state[i]
            out.append(t[:, lo:] if (spec.backbone == "xlstm" and blk in spec.slstm_at and w == 0) else t[lo:])
            i += 1
    return out


def _context_inputs(w, n, pad, pad_vec):
    """What prefill takes for the first n rows of window(): end-aligned behind the pad entry, or left-aligned with NaN behind."""
    K = w.rtg.shape[1]
    emb, rtg, rew = w.emb[:n].cpu().clone(), w.rtg[:n].cpu().clone(), w.reward[:n].cpu().clone()
    if pad == "reference":
        for b in range(n):
            emb[b, :K - w.counts[b]] = pad_vec
        return emb, rtg, rew
    out = [torch.full_like(x, NAN) for x in (emb, rtg, rew)]
    for b in range(n):
        c = w.counts[b]
        for o, x in zip(out, (emb, rtg, rew)):
            o[b, :c] = x[b, K - c:]
    return tuple(out)


def _controls(t, live, counts):
    """Resets, relabels and keeps on live slots: slot t % live restarts every third step, and every fifth step everybody else
    is relabelled by 2 and slot b pruned to b % 3 entries (0: not at all)."""
    reset = [t == 0 or (t % 3 == 2 and b == t % live) for b in range(live)]
    relabel = keep = None
    if t % 5 == 4:
        relabel = [0 if reset[b] else 2 for b in range(live)]
        keep = [b % 3 for b in range(live)]
    return reset, relabel, keep


# ---- 1. parked slots in "own" mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", ["reference", "none"])
@pytest.mark.parametrize("K", [3, 6])
@pytest.mark.parametrize("name", ["xlstm", "mamba"])
def test_own_mode_steps_the_live_prefix_and_leaves_parked_slots_alone(hip_lib, name, K, pad):
    """7 slots, 4 (2 K + 1) steps in four phases of live count 7 -> 4 -> 2 -> 6 with a window swap of a live and a parked slot at
    every change: every position wraps, at its own pace."""
    spec = wc.spec_of(name)
    sd = init_state_dict(spec, seed=3)
    B, D = 7, spec.d_model
    phase = 2 * K + 1
    lives, steps = [7, 4, 2, 6], 4 * phase
    seq = wc.make_steps(B, D, steps, seed=13)
    pad_vec = torch.linspace(-1.0, 1.0, D)
    eng = new_engine(spec, sd, B)
    eng.alloc_window(K)
    eng.set_window_pad(pad_vec.to(DEV), is_embedding=True)
    assert eng.window_slots == "shared"
    eng.set_window_slots("own")
    hist, prev = SlotHistory(B, K), torch.zeros(B)
    for t, (obs, rtg, rew) in enumerate(seq):
        live = lives[t // phase]
        if t % phase == 0 and t > 0:
            eng.set_live(B)
            eng.swap_window_slots([1], [B - 1]), hist.swap([1], [B - 1])      # slot 6 is parked in every phase behind the first
            eng.set_live(live)
        reset, relabel, keep = _controls(t, live, hist.counts)
        w0, s0 = _window(eng), export_state(eng, spec)
        c0 = eng.context_counts()["env_timesteps"]
        act, tok = eng.step_window(*_dev(obs[:live], rtg[:live], prev[:live]), reset=reset, relabel=relabel, keep=keep, pad=pad,
                                   obs_is_embedding=True)
        got = (act.clone(), tok.clone(), _logits(eng))
        assert tuple(act.shape) == (live, spec.act_dim) and got[2].shape[0] == live
        if pad == "reference":
            assert eng.context_counts()["env_timesteps"] - c0 == live * K, t
        hist.step_live(live, obs, rtg, prev, reset=reset, relabel=relabel, keep=keep)
        prev = rew
        what = f"{name} K={K} pad={pad} step {t} live {live}"
        w = _same_window(eng, hist, D, what)
        # parked slots: window, count, state
        assert w.counts[live:] == w0.counts[live:], what
        for x, y in zip((w0.emb, w0.rtg, w0.reward), (w.emb, w.rtg, w.reward)):
            assert torch.equal(bits(x[live:]), bits(y[live:])), f"{what}: a parked window moved"
        same_state(_parked_state(s0, spec, live), _parked_state(export_state(eng, spec), spec, live), f"{what}: parked state")
        # live slots: the stored-context entry over window()'s live rows, on the same engine
        eng.set_context_rows("live")
        ones = torch.ones(live, dtype=torch.uint8, device=DEV)
        ctx = _dev(*_context_inputs(w, live, pad, pad_vec))
        a, k = eng.prefill(*ctx, reset_mask=ones, obs_is_embedding=True, lengths=None if pad == "reference" else w.counts[:live])
        want = (a.clone(), k.clone(), _logits(eng))
        eng.set_context_rows("all")
        for i, n in enumerate(("actions", "tokens", "logits")):
            assert torch.equal(bits(got[i]), bits(want[i][:live])), f"{what}: {n} differ from prefill over the live rows"
        assert bool(got[0].isfinite().all()) and bool((got[1] >= 0).all())
    assert max(hist.counts) == K
    eng.close()


# ---- 2. the update kernel past one workgroup -------------------------------------------------------------------------------------
def test_three_hundred_slots_with_parked_ones_on_both_sides_of_slot_256(hip_lib):
    """300 slots, K = 3: live 300 -> 250 -> 270 -> 300, so slots 250 .. 255 and 256 .. 299 are parked for a while and the slots
    around 256 (the update kernel's second workgroup) wrap at another pace than the rest.  A second engine takes the same steps
    as raw observations: the state Linear at `live` rows, through the scratch rows into every slot's own position -- rtg, reward
    and counts exact, the embeddings against the fp64 Linear (rel_err 1e-5, the bar tests/test_gpu_window.py holds that path to)."""
    spec = wc.spec_of("xlstm")
    sd = init_state_dict(spec, seed=3)
    B, K, D = 300, 3, spec.d_model
    W, bias = sd["embed_state.weight"].double(), sd["embed_state.bias"].double()
    eng, raw = new_engine(spec, sd, B), new_engine(spec, sd, B)
    for e in (eng, raw):
        e.alloc_window(K)
        e.set_window_slots("own")
    lives = [300, 250, 250, 270, 270, 270, 300, 300]
    seq, obs_seq = wc.make_steps(B, D, len(lives), seed=17), wc.make_steps(B, spec.state_dim, len(lives), seed=18)
    hist, hraw, prev = SlotHistory(B, K), SlotHistory(B, K), torch.zeros(B)
    for t, live in enumerate(lives):
        (vec, rtg, rew), obs = seq[t], obs_seq[t][0]
        reset = [t == 0 or (t == 4 and b % 7 == 0) for b in range(live)]
        relabel = [0 if reset[b] else 2 for b in range(live)] if t == 5 else None
        for e in (eng, raw):
            e.set_live(live)
        eng.step_window(*_dev(vec[:live], rtg[:live], prev[:live]), reset=reset, relabel=relabel, pad="none", obs_is_embedding=True)
        raw.step_window(*_dev(obs[:live], rtg[:live], prev[:live]), reset=reset, relabel=relabel, pad="none")
        hist.step_live(live, vec, rtg, prev, reset=reset, relabel=relabel)
        hraw.step_live(live, obs, rtg, prev, reset=reset, relabel=relabel)
        prev = rew
        _same_window(eng, hist, D, f"300 slots, step {t} live {live}")
        w = _window(raw)
        o, g, r = hraw.tensors_of(spec.state_dim)
        assert w.counts == hraw.counts and torch.equal(bits(w.rtg.cpu()), bits(g)) and torch.equal(bits(w.reward.cpu()), bits(r)), t
        want = o.double() @ W.T + bias
        for b, n in enumerate(hraw.counts):
            want[b, :K - n] = 0.0
        err = rel_err(w.emb.cpu(), want)
        assert err < 1e-5, (t, err)
    assert max(hist.counts) == K
    print(f"[window slots] raw observations at {B} slots, parked ones among them: embeddings rel_err {err:.2e} (bar 1e-5)")
    eng.close(), raw.close()


# ---- 3. shared mode is what it was -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", ["reference", "none"])
@pytest.mark.parametrize("name,B,K", [("xlstm", 5, 6), ("mamba", 5, 6)])
def test_switching_to_own_and_back_with_nothing_parked_changes_nothing(hip_lib, name, B, K, pad):
    """The inputs of test_gpu_window.py::test_window_step_is_bit_identical_to_prefill_over_the_history on two engines: one never
    leaves "shared", the other runs the middle third of the steps in "own" -- nobody parked -- and goes back."""
    spec = wc.spec_of(name)
    sd = init_state_dict(spec, seed=3)
    steps = 2 * K + 3
    seq, resets = wc.make_steps(B, spec.d_model, steps, seed=11), wc.reset_schedule(B, steps)
    pad_vec = torch.linspace(-1.0, 1.0, spec.d_model)
    eng, ref = new_engine(spec, sd, B), new_engine(spec, sd, B)
    for e in (eng, ref):
        e.alloc_window(K)
        e.set_window_pad(pad_vec.to(DEV), is_embedding=True)
    prev = torch.zeros(B)
    for t, (obs, rtg, rew) in enumerate(seq):
        if t == steps // 3:
            eng.set_window_slots("own")
        if t == 2 * steps // 3:
            eng.set_window_slots("shared")
        out = []
        for e in (eng, ref):
            act, tok = e.step_window(*_dev(obs, rtg, prev), reset=resets[t], pad=pad, obs_is_embedding=True)
            w = _window(e)
            out.append((act.clone(), tok.clone(), _logits(e), w.emb, w.rtg, w.reward, torch.tensor(w.counts, dtype=torch.int32)))
        prev = rew
        for x, y in zip(*out):
            assert torch.equal(bits(x), bits(y)), (name, pad, t, eng.window_slots)
    assert eng.window_slots == "shared"
    same_state(export_state(eng, spec), export_state(ref, spec), f"{name} pad={pad}: state behind the last step")
    eng.close(), ref.close()


# ---- 4. the movers ---------------------------------------------------------------------------------------------------------------
def _run(eng, hist, seq, t0, t1, live, prev, pad="none"):
    """Steps t0 .. t1 - 1 of seq on the live prefix (slot t % live restarts every third step); returns the next prev_reward."""
    for t in range(t0, t1):
        obs, rtg, rew = seq[t]
        reset = [t == 0 or (t % 3 == 2 and b == t % live) for b in range(live)]
        eng.step_window(*_dev(obs[:live], rtg[:live], prev[:live]), reset=reset, pad=pad, obs_is_embedding=True)
        hist.step_live(live, obs, rtg, prev, reset=reset)
        prev = rew
    return prev


def _mover_engine(spec, sd, B, K, steps, seed, live_to=None):
    eng = new_engine(spec, sd, B)
    eng.alloc_window(K)
    eng.set_window_pad(torch.linspace(-1.0, 1.0, spec.d_model).to(DEV), is_embedding=True)
    eng.set_window_slots("own")
    hist = SlotHistory(B, K)
    seq = wc.make_steps(B, spec.d_model, steps + 2, seed=seed)
    prev = _run(eng, hist, seq, 0, steps, B, torch.zeros(B))
    if live_to is not None:     # two more steps on a prefix: the slots' positions and counts part ways
        eng.set_live(live_to)
        prev = _run(eng, hist, seq, steps, steps + 2, live_to, prev)
    return eng, hist, prev


@pytest.mark.parametrize("name", ["xlstm", "mamba"])
def test_copy_with_fan_out_and_swap_of_a_live_with_a_parked_slot(hip_lib, name):
    spec = wc.spec_of(name)
    sd = init_state_dict(spec, seed=3)
    B, K, D = 6, 3, spec.d_model
    eng, hist, prev = _mover_engine(spec, sd, B, K, steps=4, seed=23, live_to=4)
    s0 = export_state(eng, spec)
    # fan-out: live slot 1 into live slot 3 and parked slot 5
    eng.copy_window_slots([1, 1], [3, 5]), hist.copy([1, 1], [3, 5])
    w = _same_window(eng, hist, D, f"{name}: copy")
    assert w.counts[3] == w.counts[5] == w.counts[1]
    # swap: live slot 0 with parked slot 4
    eng.swap_window_slots([0], [4]), hist.swap([0], [4])
    _same_window(eng, hist, D, f"{name}: swap")
    same_state(s0, export_state(eng, spec), f"{name}: the window movers touch no recurrent state")
    # the state movers leave the ring alone
    eng.copy_slots([2], [5]), eng.swap_slots([0], [4])
    rec = eng.save_slots([1])
    eng.load_slots([3], rec)
    _same_window(eng, hist, D, f"{name}: behind the state movers")
    # the next step: the copies answer as their source does, given the same inputs
    eng.set_live(B)
    obs, rtg, rew = (x.clone() for x in wc.make_steps(B, D, 1, seed=29)[0])
    for d in (3, 5):
        obs[d], rtg[d], prev[d] = obs[1], rtg[1], prev[1]
    act, tok = eng.step_window(*_dev(obs, rtg, prev), pad="reference", obs_is_embedding=True)
    lg = _logits(eng)
    hist.step_live(B, obs, rtg, prev)
    _same_window(eng, hist, D, f"{name}: step behind the movers")
    for d in (3, 5):
        for x in (act, tok, lg):
            assert torch.equal(bits(x[d]), bits(x[1])), (name, d)
    eng.close()


@pytest.mark.parametrize("name", ["xlstm", "mamba"])
def test_records_are_position_free_and_load_into_another_engine(hip_lib, name):
    """Engine one has run 4 + 2 steps, engine two 7 (K = 3: other positions, other counts).  A record is window()'s row and the
    count; loaded into other slots of engine two it shows in window() bit for bit, and the next step there equals the prefill
    over the windows."""
    spec = wc.spec_of(name)
    sd = init_state_dict(spec, seed=3)
    B, K, D = 5, 3, spec.d_model
    one, h1, _ = _mover_engine(spec, sd, B, K, steps=4, seed=31, live_to=3)
    two, h2, prev = _mover_engine(spec, sd, B, K, steps=7, seed=37)
    assert one.window_slot_numel == K * (D + 2) + 1
    slots = [4, 0, 2, 0]                                   # (parked and live ones; a slot may be saved twice)
    rec = one.save_window_slots(slots)
    w1 = _window(one)
    assert tuple(rec.shape) == (4, K * (D + 2) + 1)
    for i, b in enumerate(slots):
        want = torch.cat([w1.emb[b].reshape(-1), w1.rtg[b], w1.reward[b], torch.tensor([float(w1.counts[b])], device=DEV)])
        assert torch.equal(bits(rec[i]), bits(want)), (name, i)
    s2 = export_state(two, spec)
    two.load_window_slots([1, 3, 0], rec[:3])
    for src, dst in ((4, 1), (0, 3), (2, 0)):
        h2.rows[dst] = [[v.clone(), g, r] for v, g, r in h1.rows[src]]
    _same_window(two, h2, D, f"{name}: loaded records")
    same_state(s2, export_state(two, spec), f"{name}: a window load touches no recurrent state")
    # the next step on engine two against the prefill over the history, every env reset
    ref = new_engine(spec, sd, B)
    pad_vec = torch.linspace(-1.0, 1.0, D)
    obs, rtg, rew = wc.make_steps(B, D, 1, seed=41)[0]
    act, tok = two.step_window(*_dev(obs, rtg, prev), pad="reference", obs_is_embedding=True)
    got = (act.clone(), tok.clone(), _logits(two))
    h2.step_live(B, obs, rtg, prev)
    _same_window(two, h2, D, f"{name}: step behind the load")
    a, k = ref.prefill(*_dev(*h2.tensors(pad_vec=pad_vec)), reset_mask=torch.ones(B, dtype=torch.uint8, device=DEV), obs_is_embedding=True)
    for x, y in zip(got, (a.clone(), k.clone(), _logits(ref))):
        assert torch.equal(bits(x), bits(y)), name
    one.close(), two.close(), ref.close()


@pytest.mark.parametrize("name", ["xlstm", "mamba"])
def test_nan_beyond_the_counts_and_in_other_slots_reaches_no_record_and_no_output(hip_lib, name):
    """Every ring row NaN (K + 1 NaN steps), then slot 0 alone restarts with a finite timestep: its ring rows of age >= 1 and every
    other slot are NaN.  Its record, a copy of it and both their next outputs equal those of an engine that never saw a NaN."""
    spec = wc.spec_of(name)
    sd = init_state_dict(spec, seed=3)
    B, K, D = 4, 4, spec.d_model
    seq = wc.make_steps(B, D, 2, seed=43)
    nan, pad_vec = torch.full((B, D), NAN), torch.linspace(-1.0, 1.0, D)
    out = []
    for poison in (True, False):
        eng = new_engine(spec, sd, B)
        eng.alloc_window(K)
        eng.set_window_pad(pad_vec.to(DEV), is_embedding=True)
        eng.set_window_slots("own")
        filler = nan if poison else torch.ones(B, D)
        for _ in range(K + 1):
            eng.step_window(*_dev(filler, filler[:, 0], filler[:, 0]), pad="none", obs_is_embedding=True)
        obs, rtg, _ = seq[0]
        obs, rtg = obs.clone(), rtg.clone()
        obs[1:], rtg[1:] = filler[1:], filler[1:, 0]
        eng.step_window(*_dev(obs, rtg, filler[:, 0]), reset=[True, False, False, False], pad="none", obs_is_embedding=True)
        rec = eng.save_window_slots([0]).clone()
        eng.copy_window_slots([0], [2])
        eng.set_live(3)
        obs, rtg, rew = (x[:3].clone() for x in seq[1])
        obs[1], rtg[1] = filler[1], filler[1, 0]
        obs[2], rtg[2], rew[2] = obs[0], rtg[0], rew[0]
        res = []
        for pad in ("reference", "none"):     # (two more timesteps for slots 0 and 2: counts 2 and 3 of K = 4)
            act, tok = eng.step_window(*_dev(obs, rtg, rew), pad=pad, obs_is_embedding=True)
            lg = _logits(eng)
            res += [act[[0, 2]].clone(), tok[[0, 2]].clone(), lg[[0, 2]].clone()]
            assert torch.equal(bits(act[0]), bits(act[2])) and torch.equal(bits(lg[0]), bits(lg[2])), (name, pad)
        w = _window(eng)
        assert w.counts[0] == w.counts[2] == 3
        out.append([rec] + res + [w.emb[[0, 2]], w.rtg[[0, 2]], w.reward[[0, 2]]])
        assert all(bool(x.isfinite().all()) for x in out[-1] if x.dtype == torch.float32), (name, poison)
        eng.close()
    for x, y in zip(*out):
        assert torch.equal(bits(x), bits(y)), name


def _unchanged(eng, spec, call, err, needle):
    w0, s0 = _window(eng), export_state(eng, spec)
    with pytest.raises(err, match=needle):
        call()
    w1 = _window(eng)
    assert w1.counts == w0.counts, needle
    for x, y in zip((w0.emb, w0.rtg, w0.reward), (w1.emb, w1.rtg, w1.reward)):
        assert torch.equal(bits(x), bits(y)), needle
    same_state(s0, export_state(eng, spec), f"refused ({needle})")


def test_bad_lists_and_bad_calls_are_refused_with_ring_counts_and_state_unchanged(hip_lib):
    spec = wc.spec_of("xlstm")
    sd = init_state_dict(spec, seed=3)
    B, K, D = 5, 3, spec.d_model
    bare = new_engine(spec, sd, B)
    for call in (lambda: bare.set_window_slots("own"), lambda: bare.copy_window_slots([0], [1]), lambda: bare.save_window_slots([0])):
        with pytest.raises(LramError, match="no window ring"):
            call()
    bare.close()
    eng, hist, prev = _mover_engine(spec, sd, B, K, steps=4, seed=47, live_to=3)
    rec = eng.save_window_slots([0, 1])
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)

    def raw(fn, a, b=None, records=None):
        args = [eng._h, i32(a)] + ([i32(b)] if b is not None else []) + [len(a)]
        args += [ctypes.c_void_p(records.data_ptr())] if records is not None else []
        if getattr(eng.lib, fn)(*args, _stream_ptr(eng.device)) != 0:
            raise LramError(eng.lib.lram_last_error().decode())

    # the library's own rules (the Python surface checks the same lists before it calls)
    for fn in ("lram_window_copy_slots", "lram_window_swap_slots"):
        _unchanged(eng, spec, lambda: raw(fn, [0, B], [1, 2]), LramError, "out of range")
        _unchanged(eng, spec, lambda: raw(fn, [0, 1], [-1, 2]), LramError, "out of range")
        _unchanged(eng, spec, lambda: raw(fn, [0, 1], [2, 2]), LramError, "destination slot is listed twice")
        _unchanged(eng, spec, lambda: raw(fn, [0, 1], [1, 2]), LramError, "both source and destination")
    _unchanged(eng, spec, lambda: raw("lram_window_swap_slots", [0, 0], [1, 2]), LramError, "listed twice")
    _unchanged(eng, spec, lambda: raw("lram_window_save_slots", [0, B], records=rec), LramError, "out of range")
    _unchanged(eng, spec, lambda: raw("lram_window_load_slots", [0, 0], records=rec), LramError, "listed twice")
    _unchanged(eng, spec, lambda: raw("lram_window_load_slots", [0, 7], records=rec), LramError, "out of range")
    bad = rec.clone()
    bad[1, -1] = K + 1                                    # a count the ring cannot hold: nothing of either record is written
    _unchanged(eng, spec, lambda: eng.load_window_slots([3, 4], bad), LramError, "count in 0")
    bad[1, -1] = NAN
    _unchanged(eng, spec, lambda: eng.load_window_slots([3, 4], bad), LramError, "count in 0")
    # ... and the Python surface
    _unchanged(eng, spec, lambda: eng.copy_window_slots([0, 1], [1, 2]), ValueError, "both source and destination")
    _unchanged(eng, spec, lambda: eng.swap_window_slots([0, 0], [1, 2]), ValueError, "listed twice")
    _unchanged(eng, spec, lambda: eng.load_window_slots([0, B], rec), ValueError, "out of range")
    with pytest.raises(ValueError, match="unknown mode"):
        eng.set_window_slots("each")
    # the step's other refusals stand in "own" mode, parked slots or not
    obs, rtg, _ = wc.make_steps(B, D, 1, seed=53)[0]
    step = lambda **kw: eng.step_window(*_dev(obs[:3], rtg[:3], prev[:3]), obs_is_embedding=True, **kw)
    eng.set_context_rows("live")
    _unchanged(eng, spec, lambda: step(pad="none"), LramError, "LRAM_CONTEXT_ROWS_ALL")
    eng.set_context_rows("all")
    _unchanged(eng, spec, lambda: step(pad="none", reset=[1, 0, 0], relabel=[1, 0, 0]), ValueError, "reset and relabelled")
    _unchanged(eng, spec, lambda: step(pad="none", discrete="per_slot"), LramError, "slot table")
    # shared mode refuses the parked slots as ever; the mode is host bookkeeping, and alloc_window sets it back
    eng.set_window_slots("shared")
    with pytest.raises(LramError, match="parked"):
        eng.step_window(*_dev(obs, rtg, prev), pad="none", obs_is_embedding=True)
    eng.set_window_slots("own")
    step(pad="none")
    hist.step_live(3, obs, rtg, prev)
    _same_window(eng, hist, D, "behind the refusals")
    assert eng.context_rows == "all" and eng.lib.lram_get_context_rows(eng._h) == 0
    eng.alloc_window(K)
    assert eng.window_slots == "shared" and eng.lib.lram_window_get_slots(eng._h) == 0
    eng.close()


# ---- 5. the agent ----------------------------------------------------------------------------------------------------------------
class _ScriptedEnv:
    """n envs that replay a script, whatever the actions; keeps, per step, the logits and tokens of the rows the agent stepped."""

    def __init__(self, first, steps, agent):
        self.n_envs, self.device = first.shape[0], torch.device(DEV)
        self.first, self.steps, self.t, self.agent, self.seen = first, steps, 0, agent, []

    def reset(self):
        return self.first.clone().to(DEV)

    def step(self, actions):
        eng = self.agent.engine
        lg = _logits(eng).cpu()
        self.seen.append({e: (lg[i], eng._tokens[i].cpu().clone()) for i, e in enumerate(self.agent.active)})
        obs, reward, done = self.steps[self.t]
        self.t += 1
        return obs.clone().to(DEV), reward.clone().to(DEV), done.clone().to(DEV)


@pytest.mark.parametrize("name", ["xlstm", "mamba"])
def test_park_finished_on_a_window_agent_with_its_own_slots(hip_lib, name):
    """Five envs with episodes of 2, 3, 4, 6 and 7 steps, two episodes each, K = 3: an env is parked once it has finished its two.
    Episode rewards, lengths and counts equal those of park_finished=False, fewer env-timesteps are computed, and every env's
    logits of every step it takes in both runs agree under the stored-context bar."""
    from lram_amd.agent import RecurrentAgent
    from lram_amd.rollout import evaluate_policy_batched
    spec = wc.spec_of(name)
    sd = init_state_dict(spec, seed=3)
    lengths, K, n = [2, 3, 4, 6, 7], 3, 5
    g = torch.Generator().manual_seed(59)
    script = [(torch.rand(n, 12, generator=g) * 2 - 1, torch.randint(-2, 7, (n,), generator=g).float() / 4,
               torch.tensor([(t + 1) % L == 0 for L in lengths])) for t in range(14)]
    first = torch.rand(n, 12, generator=g) * 2 - 1
    runs = {}
    for park in (False, True):
        agent = RecurrentAgent(spec, sd, n_envs=n, device=DEV, use_inference_cache=False, eval_context_len=K, window_slots="own")
        env = _ScriptedEnv(first, script, agent)
        agent.engine.context_counts(reset=True)
        rewards, eps, _ = evaluate_policy_batched(agent, env, n_eval_episodes=2 * n, target_return=3.0, reward_scale=2.0,
                                                  return_episode_rewards=True, park_finished=park)
        runs[park] = (rewards, eps, env.t, agent.engine.context_counts()["env_timesteps"], env.seen)
        agent.engine.close()
    assert runs[True][:3] == runs[False][:3] and runs[True][2] == 14
    assert runs[False][3] == 14 * n * K and runs[True][3] == sum(2 * L for L in lengths) * K
    worst = 0.0
    for t, (full, part) in enumerate(zip(runs[False][4], runs[True][4])):
        assert sorted(full) == list(range(n)) and sorted(part) == [e for e in range(n) if t < 2 * lengths[e]], t
        for e, (lg, tok) in part.items():
            lg_full, tok_full = full[e]
            err = rel_err(lg, lg_full)
            worst = max(worst, err)
            assert err < wc.LOGIT_TOL, (name, t, e, err)
            top2 = lg_full.view(spec.act_dim, spec.n_vocab).topk(2, dim=-1).values
            clear = (top2[:, 0] - top2[:, 1]) >= wc.MIN_GAP
            assert torch.equal(tok[clear], tok_full[clear]), (name, t, e)
    print(f"[window slots] {name}: parked run against the full one, worst logits rel_err {worst:.2e} (bar {wc.LOGIT_TOL:.0e})")

    # without window_slots="own" the refusal stands, before the first step
    agent = RecurrentAgent(spec, sd, n_envs=n, device=DEV, use_inference_cache=False, eval_context_len=K)
    env = _ScriptedEnv(first, script, agent)
    with pytest.raises(ValueError, match="park_finished"):
        evaluate_policy_batched(agent, env, n_eval_episodes=2 * n, target_return=3.0, reward_scale=2.0, park_finished=True)
    assert env.t == 0
    agent.engine.close()
