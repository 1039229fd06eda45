"""CPU: the bookkeeping of parked envs -- rollout.SlotScheduler, RecurrentAgent.set_active / predict_batch on a recording
stand-in for the engine, evaluate_policy_batched(park_finished=True) -- and the three C ABI entries behind them
(lram_set_live, lram_get_live, lram_state_swap_slots): declared, exported, bound, and refusing a null engine.  No GPU."""
import ctypes
import os
import random
import re

import pytest
import torch

from lram_amd import engine, preset
from lram_amd.engine import check_swap_lists
from lram_amd.rollout import BatchedRollout, SlotScheduler, SyntheticVecEnv, evaluate_policy_batched
from tests.stub_engine import StubEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lram_hip.h")
SYMBOLS = ("lram_set_live", "lram_get_live", "lram_state_swap_slots")


# ---- 1. the C ABI surface -------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/lram_hip.h"
        assert name in engine._SYMBOLS, f"{name} is missing from the ctypes table"
        assert getattr(hip_lib, name) is not None
    assert re.search(r"#define\s+LRAM_ABI_VERSION\s+1\b", text)


def test_entries_refuse_a_null_engine(hip_lib):
    idx = (ctypes.c_int32 * 2)(0, 1)
    assert hip_lib.lram_get_live(None) == 0
    assert hip_lib.lram_set_live(None, 1, None) != 0 and b"state not allocated" in hip_lib.lram_last_error()
    assert hip_lib.lram_state_swap_slots(None, idx, idx, 1, None) != 0 and b"state not allocated" in hip_lib.lram_last_error()


def test_header_says_what_a_parked_slot_is():
    text = open(HEADER).read()
    for needle in ("PARKED", "evaluation.py:184", "stay with the slot INDEX", "lram_encoder_step"):
        assert needle in text, needle


def test_check_swap_lists_rules():
    assert check_swap_lists([0, 1], [2, 3], 4) == ([0, 1], [2, 3])
    assert check_swap_lists([], [], 4) == ([], [])
    for a, b in (([0, 0], [1, 2]), ([0, 1], [2, 2]), ([0, 1], [1, 2]), ([0], [4]), ([-1], [0]), ([0, 1], [2])):
        with pytest.raises(ValueError):
            check_swap_lists(a, b, 4)


# ---- 2. the scheduler under a seeded random walk -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (12, 2), (37, 3)])
def test_scheduler_invariants_under_a_random_walk(n, seed):
    rng = random.Random(seed)
    s = SlotScheduler(n)
    assert s.live_envs() == list(range(n)) and s.identity
    parked = set()
    for _ in range(400):
        live = [e for e in range(n) if e not in parked]
        before = list(s.env_at)
        if rng.random() < 0.5 and len(live) > 1:
            ids = rng.sample(live, rng.randint(1, len(live) - 1))
            a, b, n_live = s.park(ids)
            parked |= set(ids)
        elif parked:
            ids = rng.sample(sorted(parked), rng.randint(1, len(parked)))
            a, b, n_live = s.resume(ids)
            parked -= set(ids)
        else:
            continue
        # the permutation stays a bijection, and is what the swaps make of the one before
        assert sorted(s.env_at) == list(range(n)) and all(s.env_at[s.slot_of[e]] == e for e in range(n))
        for x, y in zip(a, b):
            before[x], before[y] = before[y], before[x]
        assert before == s.env_at
        # live envs are exactly the prefix
        assert n_live == s.n_live == n - len(parked)
        assert set(s.live_envs()) == set(range(n)) - parked and len(s.live_envs()) == n_live
        assert all(s.is_live(e) != (e in parked) for e in range(n))
        # at most one swap per moved env; all indices of the call distinct and in range
        assert len(a) == len(b) <= len(ids)
        assert len(set(a + b)) == 2 * len(a) and all(0 <= x < n for x in a + b)
        moved = {s.env_at[x] for x in a + b}
        assert sum(e in moved for e in ids) == len(a), "a swap that moves no parked / resumed env"
    for bad in ([0, 0], [n + 2], [-1]):
        with pytest.raises(ValueError):
            SlotScheduler(n + 2).park(bad)
    with pytest.raises(ValueError):
        SlotScheduler(3).park([0, 1, 2])        # nobody left
    with pytest.raises(ValueError):
        SlotScheduler(3).resume([1])            # not parked


# ---- 3. the agent on a recording engine ------------------------------------------------------------------------------------------
class _Engine(StubEngine):
    """tests/stub_engine.StubEngine with Engine's constructor, a live prefix, and a record of what the agent asks for."""

    def __init__(self, spec, state_dict, batch, device=None):
        super().__init__(spec, batch, torch.device("cpu"))
        self.live, self.calls, self.rows = batch, [], []
        self._tokens = torch.zeros(batch, spec.act_dim, dtype=torch.int32)

    def set_live(self, n):
        assert 1 <= n <= self.batch
        self.live = n
        self.calls.append(("set_live", n))

    def swap_slots(self, a, b):
        check_swap_lists(a, b, self.batch)
        self.calls.append(("swap", list(a), list(b)))

    def step(self, obs, rtg, reward, reset_mask=None, **kw):
        assert obs.shape[0] == rtg.shape[0] == reward.shape[0] == reset_mask.shape[0] == self.live, "not the live rows"
        self.rows.append(obs.shape[0])
        self.calls.append(("step", obs.clone(), rtg.clone(), obs.data_ptr()))
        return super().step(obs, rtg, reward, reset_mask)

    def copy_slots(self, src, dst):
        self.calls.append(("copy", list(src), list(dst)))

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


def _inputs(spec, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, spec.state_dim, generator=g), torch.rand(n, generator=g),
            (torch.rand(n, generator=g) < 0.3).to(torch.uint8))


def test_predict_batch_gathers_and_scatters_the_right_rows(agent_mod):
    spec, n = preset("xlstm_tiny"), 8
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n)
    eng = a.engine
    obs, rtg, mask = _inputs(spec, n, 1)
    want = obs[:, :spec.act_dim] * 0.5 + rtg.view(-1, 1) + mask.float().view(-1, 1)     # the stub's action of every env
    # every env active, identity permutation: today's path -- the engine is handed the caller's own tensors, no gather
    got = a.predict_batch(obs, rtg, None, mask)
    assert torch.equal(got, want) and a.active == list(range(n))
    assert eng.calls[-1][3] == obs.data_ptr(), "the all-active path copied the observations"
    # park envs 1 and 5: envs 7 and 6 take their slots, six rows are stepped, the parked rows come back as 0
    a.set_active([0, 2, 3, 4, 6, 7])
    assert [c for c in eng.calls if c[0] in ("swap", "set_live")] == [("swap", [1, 5], [6, 7]), ("set_live", 6)]
    assert a.active == [0, 6, 2, 3, 4, 7] and eng.live == 6
    got = a.predict_batch(obs, rtg, None, mask)
    assert eng.rows[-1] == 6 and torch.equal(eng.calls[-1][1], obs[a.active]) and torch.equal(eng.calls[-1][2], rtg[a.active])
    exp = want.clone()
    exp[[1, 5]] = 0.0
    assert got.shape == (n, spec.act_dim) and torch.equal(got, exp)
    # park env 0 and resume env 5 in one call: one swap each
    a.set_active([2, 3, 4, 5, 6, 7])
    assert a.engine.live == 6 and sorted(a.active) == [2, 3, 4, 5, 6, 7]
    got = a.predict_batch(obs, rtg, None, mask)
    exp = want.clone()
    exp[[0, 1]] = 0.0
    assert torch.equal(got, exp)
    # everyone back, but no longer in their own slots: still a gather, full width
    a.set_active(range(n))
    assert eng.live == n and not a.scheduler.identity
    assert torch.equal(a.predict_batch(obs, rtg, None, mask), want) and eng.rows[-1] == n
    for bad in ([], [0, 0], [n]):
        with pytest.raises(ValueError):
            a.set_active(bad)


def test_set_active_refuses_to_exchange_slots_whose_settings_differ(agent_mod):
    spec, n = preset("xlstm_tiny"), 4
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n, a_sample_kwargs={"top_k": 0, "top_p": 0.0})
    a.set_slot_sampling([3], {"temperature": 2.0})
    n_calls = len(a.engine.calls)
    with pytest.raises(ValueError, match="per-slot sampling setting"):
        a.set_active([1, 2, 3])            # env 0 would change places with env 3, whose temperature differs
    assert len(a.engine.calls) == n_calls and a.active == [0, 1, 2, 3], "a refused change did something"
    a.set_active([0, 1, 2])                # env 3 is the tail already: no swap, nothing to refuse
    assert a.engine.live == 3


def test_evaluation_with_parked_envs_returns_what_it_returns_without(agent_mod):
    spec, n = preset("xlstm_tiny"), 6
    out, engines = [], []
    for park in (False, True):
        env = SyntheticVecEnv(n, obs_dim=10, ep_len=8, seed=3)      # staggered: env e ends its first episode at step 8 - e
        a = agent_mod.RecurrentAgent(spec, {}, n_envs=n, target_return=5.0)
        out.append(evaluate_policy_batched(a, env, n_eval_episodes=9, return_episode_rewards=True, park_finished=park))
        engines.append(a.engine)
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and len(out[0][0]) == 9
    assert sorted(out[0][1]) == [3, 4, 5, 6, 7, 8, 8, 8, 8]
    assert set(engines[0].rows) == {n} and len(engines[0].rows) == len(engines[1].rows) == 13
    rows = engines[1].rows
    assert rows == sorted(rows, reverse=True) and rows[0] == n and rows[-1] == 1, rows      # the live count shrinks as envs finish
    assert engines[1].live == 1 and sum(rows) < sum(engines[0].rows)


class _RecEnv(SyntheticVecEnv):
    """SyntheticVecEnv that keeps the actions it is handed."""

    def step(self, actions):
        self.__dict__.setdefault("seen", []).append(actions.clone())
        return super().step(actions)


def test_a_second_evaluation_on_the_same_agent_starts_with_every_env_active(agent_mod):
    """An evaluation with park_finished leaves one env active and the slots permuted.  The next evaluation on that agent -- here
    without parking -- steps all n envs from its first step on, and hands the env the actions a fresh agent hands it."""
    spec, n = preset("xlstm_tiny"), 6

    def run(agent, park):
        env = _RecEnv(n, obs_dim=10, ep_len=8, seed=3)
        out = evaluate_policy_batched(agent, env, n_eval_episodes=9, return_episode_rewards=True, park_finished=park)
        return out[0], out[1], torch.stack(env.seen)

    used = agent_mod.RecurrentAgent(spec, {}, n_envs=n, target_return=5.0)
    run(used, True)
    assert used.engine.live == 1 and len(used.active) == 1 and not used.scheduler.identity
    first = len(used.engine.rows)
    r_used = run(used, False)
    assert used.engine.rows[first:] == [n] * 13, used.engine.rows[first:]      # n rows from the first step of the second run on
    assert sorted(used.active) == list(range(n)) and used.engine.live == n
    r_fresh = run(agent_mod.RecurrentAgent(spec, {}, n_envs=n, target_return=5.0), False)
    assert r_used[0] == r_fresh[0] and r_used[1] == r_fresh[1]
    assert torch.equal(r_used[2], r_fresh[2]), "a reused agent hands the env other actions than a fresh one"
    assert bool((r_fresh[2].abs().sum(-1) > 0).all()), "the stand-in's actions are all zero: the comparison shows nothing"
    # ... and with parking again: what the first parked run returned
    r_again = run(used, True)
    assert r_again[0] == r_fresh[0] and r_again[1] == r_fresh[1] and used.engine.live == 1


def test_set_active_changes_to_a_disjoint_set(agent_mod):
    spec, n = preset("xlstm_tiny"), 4
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n)
    a.set_active([0])
    a.set_active([1])            # never through an empty live set: env 1 is resumed before env 0 is parked
    assert a.active == [1] and a.engine.live == 1
    a.set_active([2, 3])
    assert sorted(a.active) == [2, 3] and a.engine.live == 2


def test_rollout_fork_addresses_the_slots_the_envs_sit_in(agent_mod):
    """BatchedRollout.fork_slots takes env ids, as all of its bookkeeping does; once set_active has exchanged slots the engine is
    handed the slots those envs sit in."""
    spec, n = preset("xlstm_tiny"), 6
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n)
    ro = BatchedRollout(a, SyntheticVecEnv(n, obs_dim=10, ep_len=8, seed=3), target_return=5.0, reward_scale=1.0)
    ro.fork_slots([0], [1])
    assert a.engine.calls[-1] == ("copy", [0], [1])                  # identity: env id = slot
    a.set_active([0, 2, 3, 4, 5])                                    # env 1 parks: env 5 takes slot 1, env 1 slot 5
    assert a.scheduler.slot_of[5] == 1 and a.scheduler.slot_of[1] == 5
    ro.fork_slots([5, 0], [1, 2])
    assert a.engine.calls[-1] == ("copy", [1, 0], [5, 2])
