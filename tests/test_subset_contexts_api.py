"""CPU: stored contexts on a subset of the env slots -- the three C ABI entries (lram_set_context_rows, lram_get_context_rows,
lram_context_counts: declared, exported, bound, refusing a null engine), rollout.SlotScheduler.arrange, and the bookkeeping of
RecurrentAgent.prime_contexts / extend_contexts / score_trajectories(envs=...) on a recording stand-in for the engine.  No GPU."""
import ctypes
import os
import random
import re

import pytest
import torch

from lram_amd import engine, preset
from lram_amd.engine import ScoreResult, check_swap_lists
from lram_amd.rollout import SlotScheduler
from tests.stub_engine import StubEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lram_hip.h")
SYMBOLS = ("lram_set_context_rows", "lram_get_context_rows", "lram_context_counts")


# ---- 1. the C ABI surface -------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(hip_lib):
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/lram_hip.h"
        assert name in engine._SYMBOLS, f"{name} is missing from the ctypes table"
        assert getattr(hip_lib, name) is not None
    for k, name in enumerate(("ALL", "LIVE", "STARTED")):
        assert re.search(r"#define\s+LRAM_CONTEXT_ROWS_%s\s+%d\b" % (name, k), raw)
        assert engine.CONTEXT_ROWS[k] == name.lower()
    assert re.search(r"#define\s+LRAM_ABI_VERSION\s+1\b", text)


def test_entries_refuse_a_null_engine(hip_lib):
    out = (ctypes.c_int64 * 4)()
    assert hip_lib.lram_get_context_rows(None) == 0
    assert hip_lib.lram_set_context_rows(None, 1) != 0 and b"null engine" in hip_lib.lram_last_error()
    assert hip_lib.lram_context_counts(None, out, 0) != 0 and b"null argument" in hip_lib.lram_last_error()


# ---- 2. SlotScheduler.arrange ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_arrange_takes_at_most_two_swap_lists(seed):
    rng = random.Random(seed)
    for n in range(1, 41):
        sch = SlotScheduler(n)
        # a scheduler that has seen parking: some permutation, some live count
        perm = list(range(n))
        rng.shuffle(perm)
        sch.env_at, sch.slot_of = list(perm), [perm.index(e) for e in range(n)]
        sch.n_live = rng.randint(1, n)
        k = rng.randint(1, n)
        want = rng.sample(range(n), k)
        before, live = list(sch.env_at), sch.n_live
        lists = sch.arrange(want)
        assert len(lists) <= 2 and sch.n_live == live
        at = list(before)
        for a, b in lists:
            assert a and check_swap_lists(a, b, n) == (a, b)      # all 2n indices distinct and in range
            for sa, sb in zip(a, b):
                at[sa], at[sb] = at[sb], at[sa]
        assert at == sch.env_at and sch.env_at[:k] == want
        assert all(sch.slot_of[e] == s for s, e in enumerate(sch.env_at))
        untouched = set(range(k)) | {before.index(e) for e in want}
        assert all(sch.env_at[s] == before[s] for s in range(n) if s not in untouched), "an uninvolved slot moved"
        for a, b in reversed(lists):                              # the same lists in reverse order undo it
            sch._swap(list(zip(a, b)))
        assert sch.env_at == before
    sch = SlotScheduler(4)
    assert sch.arrange([0, 1]) == [] and sch.arrange([]) == []
    for bad in ([0, 0], [4], [-1]):
        with pytest.raises(ValueError):
            sch.arrange(bad)


# ---- 3. the agent on a recording engine -----------------------------------------------------------------------------------------
class _Engine(StubEngine):
    """tests/stub_engine.StubEngine with Engine's constructor, a live prefix, context rows, and a record of what the agent asks."""

    def __init__(self, spec, state_dict, batch, device=None):
        super().__init__(spec, batch, torch.device("cpu"))
        self.live, self.context_rows, self.calls = batch, "all", []
        self.slot_env = list(range(batch))      # which env's state a slot holds, as the swaps leave it
        self.seen = {}                          # env -> timesteps its state has taken

    def set_live(self, n):
        assert 1 <= n <= self.batch
        self.live = n
        self.calls.append(("set_live", n))

    def set_context_rows(self, mode):
        assert mode in ("all", "live", "started")
        self.context_rows = mode
        self.calls.append(("rows", mode))

    def swap_slots(self, a, b):
        check_swap_lists(a, b, self.batch)
        for sa, sb in zip(a, b):
            self.slot_env[sa], self.slot_env[sb] = self.slot_env[sb], self.slot_env[sa]
        self.calls.append(("swap", list(a), list(b)))

    def _rows(self):
        return self.batch if self.context_rows == "all" else self.live

    def _context(self, kind, obs, rtg, rew, reset_mask, lengths, append):
        B = self._rows()
        assert self.context_rows != "all" or self.live == self.batch, "stored context refused: slots are parked"
        assert obs.shape[0] == rtg.shape[0] == rew.shape[0] == B and (reset_mask is None or reset_mask.shape[0] == B)
        n = [obs.shape[1]] * B if lengths is None else list(lengths)
        assert len(n) == B
        if self.context_rows == "started":
            assert all(x >= y for x, y in zip(n, n[1:])), "mode started needs lengths that do not increase"
        for s in range(B):
            self.seen[self.slot_env[s]] = self.seen.get(self.slot_env[s], 0) + n[s]
        self.calls.append((kind, self.context_rows, B, obs.clone(), rtg.clone(), None if reset_mask is None else reset_mask.clone(),
                           None if lengths is None else n, bool(append)))
        return n

    def prefill(self, obs, rtg, rew, reset_mask=None, discrete=False, obs_is_embedding=False, want_action=True, lengths=None,
                append=False):
        self._context("prefill", obs, rtg, rew, reset_mask, lengths, append)
        act = obs[:, 0, :self.spec.act_dim] + 1.0     # the stub's action: a function of the row's own first observation
        return (act, (act * 64).round().to(torch.int32)) if want_action else (None, None)

    def score(self, obs, rtg, rew, actions=None, reset_mask=None, lengths=None, append=False, want=(), logits=False, **kw):
        n = self._context("score", obs, rtg, rew, reset_mask, lengths, append)
        B, L, A = obs.shape[0], obs.shape[1], self.spec.act_dim
        tok = torch.full((B, L, A), -1, dtype=torch.int32)
        for b in range(B):
            tok[b, :n[b]] = (obs[b, :n[b], :1] * 100).to(torch.int32)
        return ScoreResult(actions=tok.float(), tokens=tok, logp=None, logits=None)

    def set_slot_table(self, *a):
        pass

    def set_sampling(self, *a, **k):
        pass

    def set_sampling_slots(self, *a, **k):
        pass

    def reset(self, mask=None):
        pass


@pytest.fixture
def agent_mod(monkeypatch):
    from lram_amd import agent as mod
    monkeypatch.setattr(mod, "Engine", _Engine)
    return mod


def _contexts(spec, n, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, L, spec.state_dim, generator=g), torch.rand(n, L, generator=g)


def test_an_agent_that_never_parks_makes_the_same_engine_calls(agent_mod):
    spec, n, L = preset("xlstm_tiny"), 6, 5
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n)
    obs, rtg = _contexts(spec, n, L, 1)
    lengths = [5, 0, 3, 5, 1, 2]
    a.prime_contexts(obs, rtg, lengths=lengths)
    a.extend_contexts(obs, rtg, lengths=lengths, restart=[1, 0, 0, 1, 0, 0])
    a.score_trajectories(obs, rtg, lengths=lengths, window=2)
    calls = a.engine.calls
    assert [c[0] for c in calls] == ["prefill", "prefill", "score", "score", "score"], "swaps, live counts or modes on today's path"
    for c in calls:
        assert c[1] == "all" and c[2] == n
    assert torch.equal(calls[0][3], obs) and torch.equal(calls[1][4], rtg) and torch.equal(calls[3][3], obs[:, 2:4])
    assert calls[0][6] == lengths and calls[1][6] == lengths and not calls[0][7] and calls[1][7]
    assert torch.equal(calls[1][5], torch.tensor([1, 0, 0, 1, 0, 0], dtype=torch.uint8))
    assert [c[6] for c in calls[2:]] == [[2, 0, 2, 2, 1, 2], [2, 0, 1, 2, 0, 0], [1, 0, 0, 1, 0, 0]]


def test_listed_envs_are_sorted_gathered_scattered_and_parked_again(agent_mod):
    spec, n, L = preset("xlstm_tiny"), 8, 6
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n)
    a.set_active([1, 4, 5])
    slot_of, active = list(a.scheduler.slot_of), list(a.active)
    held = list(a.engine.slot_env)
    obs, rtg = _contexts(spec, n, L, 2)
    lengths = [0, 3, 0, 0, 2, 0, 6, 0]
    k = len(a.engine.calls)
    act = a.extend_contexts(obs, rtg, lengths=lengths, envs=[1, 4, 6], restart=[0, 1, 0, 0, 0, 0, 1, 0], want_action=True)
    calls = a.engine.calls[k:]
    kinds = [c[0] for c in calls]
    assert kinds.count("prefill") == 1 and kinds.count("swap") <= 4, kinds
    at = kinds.index("prefill")
    assert ("set_live", 3) in calls[:at] and ("rows", "started") in calls[:at]
    assert kinds[at + 1] == "rows" and calls[at + 1] == ("rows", "all") and calls[-1] == ("set_live", 3)
    _, mode, B, o, r, mask, n_call, append = calls[at]
    assert (mode, B, n_call, append) == ("started", 3, [6, 3, 2], True)       # env 6, 1, 4: by descending length
    assert torch.equal(o, obs[[6, 1, 4]]) and torch.equal(r, rtg[[6, 1, 4]]) and mask.tolist() == [1, 1, 0]
    assert a.engine.seen == {6: 6, 1: 3, 4: 2}, "the rows went to slots that hold other envs"
    # back in env-id order, the others' rows 0; slots, live count and mode as before: env 6 is parked again
    want = torch.zeros(n, spec.act_dim)
    want[[6, 1, 4]] = obs[[6, 1, 4], 0, :spec.act_dim] + 1.0
    assert torch.equal(act, want)
    assert list(a.scheduler.slot_of) == slot_of and a.active == active and a.engine.slot_env == held
    assert a.engine.live == 3 and a.engine.context_rows == "all"
    # envs=None: the active envs
    a.engine.seen.clear()
    a.prime_contexts(obs, rtg, lengths=[0, 1, 0, 0, 4, 2, 0, 0])
    assert a.engine.seen == {1: 1, 4: 4, 5: 2} and a.engine.slot_env == held
    # score_trajectories: the fill values in the rows of the others, the windows inside one arrangement
    a.engine.seen.clear()
    k = len(a.engine.calls)
    res = a.score_trajectories(obs, rtg, lengths=lengths, envs=[6, 4], window=4, want=("tokens",))
    assert [c[0] for c in a.engine.calls[k:]].count("score") == 2 and a.engine.seen == {6: 6, 4: 2}
    for e in range(n):
        m = lengths[e] if e in (6, 4) else 0
        assert bool((res.tokens[e, m:] == -1).all())
        assert torch.equal(res.tokens[e, :m], (obs[e, :m, :1] * 100).to(torch.int32).expand(m, spec.act_dim))
    assert a.engine.slot_env == held and a.engine.live == 3
    with pytest.raises(ValueError):
        a.extend_contexts(obs, rtg, lengths=lengths, envs=[1, 1])


def test_every_env_active_under_another_permutation(agent_mod):
    """After a park and a resume env and slot no longer agree: the rows must go to the slot that holds the env."""
    spec, n, L = preset("xlstm_tiny"), 5, 4
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n)
    a.set_active([0, 2, 3, 4])
    a.set_active([0, 1, 2, 3, 4])
    assert not a.scheduler.identity and a.engine.live == n
    obs, rtg = _contexts(spec, n, L, 3)
    lengths = [1, 2, 3, 4, 0]
    a.engine.seen.clear()
    act = a.extend_contexts(obs, rtg, lengths=lengths, want_action=True)
    assert a.engine.seen == {0: 1, 1: 2, 2: 3, 3: 4, 4: 0}
    assert torch.equal(act, obs[:, 0, :spec.act_dim] + 1.0)
    assert a.engine.live == n and a.engine.context_rows == "all"


def test_sorting_falls_back_to_mode_live_where_slots_differ(agent_mod):
    spec, n, L = preset("xlstm_tiny"), 4, 4
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n, a_sample_kwargs={"top_k": 0, "top_p": 0.0})
    a.set_slot_sampling([1], {"temperature": 2.0})
    a.set_active([0, 1, 2])
    obs, rtg = _contexts(spec, n, L, 4)
    k = len(a.engine.calls)
    a.extend_contexts(obs, rtg, lengths=[1, 4, 2, 0])        # sorting would exchange slots 0 and 1, whose temperature differs
    calls = a.engine.calls[k:]
    assert not [c for c in calls if c[0] == "swap"] and ("rows", "live") in calls
    ctx = [c for c in calls if c[0] == "prefill"][0]
    assert ctx[1] == "live" and ctx[6] == [1, 4, 2] and torch.equal(ctx[3], obs[:3])
    with pytest.raises(ValueError, match="per-slot sampling setting"):
        a.extend_contexts(obs, rtg, lengths=[1, 4, 2, 0], envs=[1, 0])   # the given order itself would exchange them
    assert a.engine.live == 3 and a.engine.context_rows == "all"
