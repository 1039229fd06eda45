"""CPU: context-window inference with a ring position per env slot -- what RecurrentAgent(window_slots="own") and
evaluate_policy_batched(park_finished=True) ask of an engine, on the recording stand-in tests/window_slots_stub_engine.py (no GPU,
no library), and the names of the slots mode."""
import dataclasses

import pytest
import torch

from lram_amd import preset
from lram_amd.engine import WINDOW_SLOTS, _SYMBOLS
from tests.window_slots_stub_engine import WindowSlotsStubEngine


@pytest.fixture
def agent_mod(monkeypatch):
    from lram_amd import agent as mod
    monkeypatch.setattr(mod, "Engine", WindowSlotsStubEngine)
    return mod


def _spec(state_dim=20, act_dim=4):
    return dataclasses.replace(preset("mamba_tiny"), state_dim=state_dim, act_dim=act_dim)


def _own(agent_mod, n, K=4, **kw):
    return agent_mod.RecurrentAgent(_spec(), {}, n_envs=n, use_inference_cache=False, eval_context_len=K, window_slots="own", **kw)


def test_the_slots_mode_has_its_names_and_symbols():
    assert WINDOW_SLOTS == ("shared", "own")      # LRAM_WINDOW_SLOTS_SHARED = 0, LRAM_WINDOW_SLOTS_OWN = 1
    for name in ("set_slots", "get_slots", "copy_slots", "swap_slots", "slot_numel", "save_slots", "load_slots"):
        assert f"lram_window_{name}" in _SYMBOLS


def test_own_mode_is_set_on_the_engine_and_belongs_to_window_mode(agent_mod):
    a = _own(agent_mod, 3)
    assert a.window_slots == "own" and a.engine.window_slots == "own" and a.engine.K == 4
    assert agent_mod.RecurrentAgent(_spec(), {}, n_envs=2, use_inference_cache=False).engine.window_slots == "shared"
    with pytest.raises(ValueError, match="window_slots"):
        agent_mod.RecurrentAgent(_spec(), {}, n_envs=2, window_slots="own")                # (the cached path has no windows)
    with pytest.raises(ValueError, match="window_slots"):
        agent_mod.RecurrentAgent(_spec(), {}, n_envs=2, use_inference_cache=False, window_slots="each")


def test_set_active_parks_through_the_scheduler_and_exchanges_the_windows(agent_mod):
    n = 4
    a = _own(agent_mod, n)
    eng = a.engine
    obs, rtg = torch.rand(n, 12), torch.rand(n)
    a.predict_batch(obs, rtg, None, torch.ones(n, dtype=torch.uint8), None)
    first = [h[0][0].clone() for h in eng.hist.rows]          # env b's first entry, in slot b
    a.set_active([1, 3])
    swaps = [m for m in eng.moves if m[0] == "swap_slots"]
    assert swaps and [("swap_window_slots",) + m[1:] for m in swaps] == [m for m in eng.moves if m[0] == "swap_window_slots"]
    assert eng.moves[-1] == ("set_live", 2) and eng.live == 2
    assert sorted(a.active) == [1, 3]
    for e in range(n):    # every env's window sits in the slot the scheduler gives the env
        assert torch.equal(eng.hist.rows[a.scheduler.slot_of[e]][0][0], first[e]), e
    a.set_active(range(n))
    assert eng.live == n and len(a.active) == n
    for e in range(n):
        assert torch.equal(eng.hist.rows[a.scheduler.slot_of[e]][0][0], first[e]), e


def test_predict_batch_gathers_the_control_arrays_into_live_slot_order(agent_mod):
    n = 5
    a = _own(agent_mod, n, K=6)
    eng = a.engine
    a.predict_batch(torch.rand(n, 12), torch.rand(n), None, torch.ones(n, dtype=torch.uint8), None)
    a.predict_batch(torch.rand(n, 12), torch.rand(n), None, None, None, prev_rewards=torch.rand(n))
    a.set_active([4, 0, 2])
    order = a.active                                        # env ids in engine slot order
    assert sorted(order) == [0, 2, 4]
    obs, rtg, prev = torch.rand(n, 12), torch.rand(n), torch.rand(n)
    reset, relabel, keep = [0, 1, 0, 1, 0], [2, 0, 1, 0, 2], [0, 5, 1, 7, 3]
    counts0 = list(eng.hist.counts)
    act = a.predict_batch(obs, rtg, None, torch.tensor(reset, dtype=torch.uint8), None, prev_rewards=prev, relabel=relabel, keep=keep)
    call = eng.calls[-1]
    assert call["live"] == 3
    assert call["reset"] == [reset[e] for e in order] and call["relabel"] == [relabel[e] for e in order]
    assert call["keep"] == [keep[e] for e in order]
    assert torch.equal(call["prev_reward"], prev[order]) and torch.equal(call["rtg"], rtg[order])
    assert torch.equal(call["obs"][:, :12], obs[order])
    # results: env-id order, parked rows 0
    assert tuple(act.shape) == (n, _spec().act_dim)
    want = obs[:, :4] * 0.5 + rtg.view(-1, 1)
    for e in range(n):
        assert torch.equal(act[e], want[e] if e in order else torch.zeros(4)), e
    # a parked env's window did not move
    for e in (1, 3):
        assert eng.hist.counts[a.scheduler.slot_of[e]] == counts0[a.scheduler.slot_of[e]] == 2
    with pytest.raises(ValueError, match="relabel"):      # the lists stay full-width
        a.predict_batch(obs, rtg, None, None, None, relabel=[0, 0, 0])


def test_fork_save_and_load_address_the_windows(agent_mod):
    n = 4
    a = _own(agent_mod, n)
    eng = a.engine
    for t in range(3):
        a.predict_batch(torch.rand(n, 12), torch.rand(n), None, torch.ones(n, dtype=torch.uint8) if t == 0 else None, None)
    a.fork_slots([0, 0], [2, 3])
    assert eng.moves[-1] == ("copy_window_slots", [0, 0], [2, 3])
    assert all(torch.equal(eng.hist.rows[d][i][0], eng.hist.rows[0][i][0]) for d in (2, 3) for i in range(3))
    rec = a.save_slots([1])
    assert eng.moves[-1] == ("save_window_slots", [1]) and tuple(rec.shape) == (1, eng.window_slot_numel) and float(rec[0, -1]) == 3.0
    a.load_slots([2], rec)
    assert eng.moves[-1] == ("load_window_slots", [2])
    assert all(torch.equal(eng.hist.rows[2][i][0], eng.hist.rows[1][i][0]) for i in range(3))
    with pytest.raises(ValueError, match="both source and destination"):
        a.fork_slots([0, 1], [1, 2])


def test_the_default_window_agent_still_refuses(agent_mod):
    from lram_amd.rollout import evaluate_policy_batched
    a = agent_mod.RecurrentAgent(_spec(), {}, n_envs=3, use_inference_cache=False, eval_context_len=3)
    with pytest.raises(ValueError, match="parked"):
        a.set_active([0, 1])
    for call in (lambda: a.fork_slots([0], [1]), lambda: a.save_slots([0]), lambda: a.load_slots([0], torch.zeros(1, 1))):
        with pytest.raises(RuntimeError, match="window on the device ring"):
            call()
    with pytest.raises(ValueError, match="park_finished"):
        evaluate_policy_batched(a, _Env(*_script([2, 2, 2], 4, seed=1)), n_eval_episodes=3, target_return=1.0, reward_scale=1.0,
                                park_finished=True)
    assert a.engine.calls == [] and a.engine.moves == []


class _Env:
    """n envs that replay a script, whatever the actions: reset() -> obs; step(actions) -> (obs, reward, done)."""

    def __init__(self, first, steps):
        self.n_envs, self.device = first.shape[0], torch.device("cpu")
        self.first, self.steps, self.t = first, steps, 0

    def reset(self):
        return self.first.clone()

    def step(self, actions):
        obs, reward, done = self.steps[self.t]
        self.t += 1
        return obs.clone(), reward.clone(), done.clone()


def _script(lengths, steps, seed):
    g = torch.Generator().manual_seed(seed)
    n, out = len(lengths), []
    for t in range(steps):
        done = torch.tensor([(t + 1) % L == 0 for L in lengths])
        out.append((torch.rand(n, 6, generator=g), torch.randint(-2, 7, (n,), generator=g).float() / 4, done))
    return torch.rand(n, 6, generator=g), out


@pytest.mark.parametrize("persist", [False, True])
def test_park_finished_steps_fewer_rows_and_reports_the_same_episodes(agent_mod, persist):
    """Four envs with episodes of 2, 3, 5 and 7 steps, two episodes each: the short envs finish early and are parked."""
    from lram_amd.rollout import evaluate_policy_batched
    lengths, out = [2, 3, 5, 7], {}
    for park in (False, True):
        a = _own(agent_mod, 4, K=5, persist_context=persist)
        env = _Env(*_script(lengths, 40, seed=5))
        rewards, eps, _ = evaluate_policy_batched(a, env, n_eval_episodes=8, target_return=3.0, reward_scale=2.0,
                                               return_episode_rewards=True, park_finished=park)
        out[park] = (rewards, eps, a.engine.rows_stepped, env.t)
    assert out[True][:2] == out[False][:2] and out[True][3] == out[False][3] == 14
    assert out[False][2] == 14 * 4 and out[True][2]== 4 + 6 + 10 + 14      # env b is stepped for 2 L_b steps
