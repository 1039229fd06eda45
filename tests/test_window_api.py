"""CPU: the host side of context-window inference -- Engine's host checks, RecurrentAgent(use_inference_cache=False) and
BatchedRollout in window mode on a recording stand-in engine (tests/window_stub_engine.py), and that stand-in's windows against
the executed reference (tests/golden/window_trace.npz, made by tests/golden/make_window_golden.py)."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from lram_amd import preset
from lram_amd.engine import check_window_controls, check_window_timesteps
from lram_amd.rollout import BatchedRollout
from tests import window_cases as wc
from tests.window_stub_engine import WindowStubEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_trace.npz")


# ---- 1. the host checks ------------------------------------------------------------------------------------------------------------
def test_window_controls_are_checked_on_the_host():
    assert check_window_controls(None, None, None, 3) == (None, None, None)
    r, m, k = check_window_controls([True, False, 0], torch.tensor([0, 2, 9]), np.array([0, 0, 4]), 3)
    assert (r, m, k) == ([1, 0, 0], [0, 2, 9], [0, 0, 4])
    assert check_window_controls(torch.tensor([1, 0], dtype=torch.uint8), None, [1, 1], 2)[0] == [1, 0]
    for bad, needle in ((dict(reset=[1, 0]), "expected 3 entries"), (dict(relabel=[0, -1, 0]), "negative"),
                        (dict(keep=[0, 0, -2]), "negative"), (dict(reset=[0, 2, 0]), "neither 0 nor 1"),
                        (dict(relabel=[0.5, 0, 0]), "integer"), (dict(reset=[0, 1, 0], relabel=[0, 3, 0]), "reset and relabelled")):
        kw = dict(reset=None, relabel=None, keep=None)
        kw.update(bad)
        with pytest.raises(ValueError, match=needle):
            check_window_controls(batch=3, **kw)
    assert check_window_controls([0, 1, 0], [2, 0, 0], None, 3)[1] == [2, 0, 0]    # a relabel beside somebody else's reset is fine


def test_window_timesteps_are_checked_on_the_host():
    assert check_window_timesteps(50, 1024, 512) == 50 and check_window_timesteps(0, 4, 128) == 0
    for K, needle in ((-1, "integer >= 1"), (2.5, "integer >= 1"), (True, "integer >= 1"), ((1 << 29) // (4 * 128) + 1, "2 GiB")):
        with pytest.raises(ValueError, match=needle):
            check_window_timesteps(K, 4, 128)
    with pytest.raises(ValueError, match="multiple of 4"):
        check_window_timesteps(3, 4, 66)


def test_the_oracle_leaves_out_at_most_one_percent_of_the_rows():
    """The committed seed of the GPU oracle comparison (window_cases.ORACLE_SEED), judged with the oracle alone."""
    for name in ("xlstm", "mamba"):
        for pad in ("reference", "none"):
            frac, n = wc.left_out_fraction(wc.oracle_windows(name, pad))
            print(f"[window] {name} pad={pad}: {frac * n:.0f} of {n} rows below the {wc.MIN_GAP:.0e} gap")
            assert n == 300 and frac <= 0.01, (name, pad, frac)


# ---- 2. the agent and the rollout on the recording engine ------------------------------------------------------------------------
@pytest.fixture
def agent_mod(monkeypatch):
    from lram_amd import agent as mod
    monkeypatch.setattr(mod, "Engine", WindowStubEngine)
    return mod


class ScriptedEnv:
    """n envs that replay a script: reset() -> obs [n, d]; step(actions) -> (obs, reward, done) of the next scripted step."""

    def __init__(self, first, steps):
        self.n_envs, self.device = first.shape[0], torch.device("cpu")
        self.first, self.steps, self.t = first, steps, 0

    def reset(self):
        return self.first.clone()

    def step(self, actions):
        obs, reward, done = self.steps[self.t]
        self.t += 1
        return obs.clone(), reward.clone(), done.clone()


def _spec(state_dim=20, act_dim=4):
    return dataclasses.replace(preset("mamba_tiny"), state_dim=state_dim, act_dim=act_dim)


def test_agent_allocates_the_ring_and_routes_predict_batch(agent_mod):
    spec, n = _spec(), 3
    mean, std = torch.linspace(-1, 1, spec.state_dim), torch.linspace(0.5, 2, spec.state_dim)
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n, state_mean=mean, state_std=std, use_inference_cache=False, eval_context_len=7)
    eng = a.engine
    assert eng.K == 7 and a.eval_context_len == 7 and a.use_inference_cache is False
    pad, is_emb = eng.pad
    assert not is_emb and torch.equal(pad, (torch.zeros(spec.state_dim) - mean) / std)       # (0 - mean) / std
    obs, rtg, prev = torch.rand(n, 12), torch.rand(n), torch.rand(n)
    act = a.predict_batch(obs, rtg, None, torch.tensor([1, 0, 0], dtype=torch.uint8), None, prev_rewards=prev, relabel=None, keep=[0, 2, 0])
    call = eng.calls[-1]
    assert call["reset"] == [1, 0, 0] and call["relabel"] is None and call["keep"] == [0, 2, 0] and call["pad"] == "reference"
    assert torch.equal(call["prev_reward"], prev) and tuple(act.shape) == (n, spec.act_dim)
    want = (torch.cat([obs, torch.zeros(n, spec.state_dim - 12)], 1) - mean) / std
    assert torch.equal(call["states"][:, -1], want) and torch.equal(call["states"][:, 0], pad.expand(n, -1))
    # what the mode refuses
    with pytest.raises(ValueError, match="parked"):
        a.set_active([0, 1])
    with pytest.raises(RuntimeError, match="predict_batch"):
        a.get_action_pred(None, obs[:1].view(1, 1, -1), None, None, rtg[:1].view(1, 1, 1), None, None, True, None)
    # the configuration's flag is honoured; the cached agent takes none of the window arguments
    off = agent_mod.RecurrentAgent(dataclasses.replace(spec, use_inference_cache=False, max_length=5), {}, n_envs=2)
    assert off.use_inference_cache is False and off.engine.K == 5
    on = agent_mod.RecurrentAgent(spec, {}, n_envs=2)
    assert on.use_inference_cache is True and on.engine.K == 0
    with pytest.raises(ValueError, match="use_inference_cache=False"):
        on.predict_batch(obs[:2], rtg[:2], None, None, None, prev_rewards=prev[:2])


def test_agent_refuses_slot_tables_in_window_mode(agent_mod):
    """A table that mixes vector and image slots, and -- until per-slot heads over the ring are wired -- every other one."""
    from lram_amd.domains import Domain, SlotTable
    spec = _spec()
    for table in (SlotTable([Domain("vec", False, 4), Domain("img", True, 1, image=True)], [1, 1]),
                  SlotTable([Domain("vec", False, 4), Domain("disc", True, 1)], [1, 1])):
        with pytest.raises(ValueError, match="slot tables are not served.*mixes vector and image slots"):
            agent_mod.RecurrentAgent(spec, {}, n_envs=2, slot_table=table, use_inference_cache=False)


def test_park_finished_is_refused_before_the_first_step_in_window_mode(agent_mod):
    from lram_amd.rollout import evaluate_policy_batched
    a = agent_mod.RecurrentAgent(_spec(), {}, n_envs=2, use_inference_cache=False, eval_context_len=3)
    first, script = _vec_script([2, 2], 4, seed=1)
    env = ScriptedEnv(first, script)
    with pytest.raises(ValueError, match="park_finished"):
        evaluate_policy_batched(a, env, n_eval_episodes=2, target_return=1.0, reward_scale=1.0, park_finished=True)
    assert env.t == 0 and a.engine.calls == []


def _vec_script(lengths, steps, seed):
    """A script for len(lengths) envs: env b's episodes all have lengths[b] steps; rewards are multiples of 0.25."""
    g = torch.Generator().manual_seed(seed)
    n, out = len(lengths), []
    for t in range(steps):
        done = torch.tensor([(t + 1) % L == 0 for L in lengths])
        out.append((torch.rand(n, 6, generator=g), torch.randint(-2, 7, (n,), generator=g).float() / 4, done))
    return torch.rand(n, 6, generator=g), out


@pytest.mark.parametrize("persist,sps", [(False, 1), (True, 1), (True, 2), (True, 3)])
def test_rollout_hands_over_rewards_resets_relabels_and_keeps(agent_mod, persist, sps):
    """Three envs with episodes of 2, 5 and 9 steps (9 > K = 6), 20 steps: per step the exact (prev_reward, reset, relabel, keep)."""
    spec, K, lengths, scale = _spec(), 6, [2, 5, 9], 2.0
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=3, use_inference_cache=False, eval_context_len=K, persist_context=persist)
    a.replay_buffer.seqs_per_sample = sps
    first, script = _vec_script(lengths, 20, seed=3)
    ro = BatchedRollout(a, ScriptedEnv(first, script), target_return=12.0, reward_scale=scale, persist_context=persist)
    for _ in script:
        ro.step()
    calls = a.engine.calls
    assert len(calls) == 20
    done_before = [torch.zeros(3, dtype=torch.bool)] + [s[2] for s in script[:-1]]
    for t, call in enumerate(calls):
        prev = torch.zeros(3) if t == 0 else script[t - 1][1] / scale
        assert torch.equal(call["prev_reward"], prev), t
        ended = done_before[t].tolist()
        if t == 0:
            assert call["reset"] == [1, 1, 1] and call["relabel"] is None and call["keep"] is None
        elif not persist:
            assert call["reset"] == [int(e) for e in ended] and call["relabel"] is None and call["keep"] is None, t
        elif not any(ended):
            assert call["reset"] == [0, 0, 0] and call["relabel"] is None and call["keep"] is None, t
        else:
            assert call["reset"] == [0, 0, 0], t
            n_ended = [t // L for L in lengths]      # episodes env b has finished by now
            want_keep = [(min(L * min(sps - 1, n_ended[b]), K) if sps > 1 else K) if ended[b] else 0 for b, L in enumerate(lengths)]
            assert call["relabel"] == [L if ended[b] else 0 for b, L in enumerate(lengths)], t
            assert call["keep"] == want_keep, (t, call["keep"], want_keep)
    if not persist:     # every episode starts from an empty window
        assert calls[2]["counts"][0] == 1 and calls[5]["counts"][1] == 1 and calls[9]["counts"][2] == 1
    assert max(max(c["counts"]) for c in calls) == K


# ---- 3. the stand-in's windows against the executed reference --------------------------------------------------------------------
def _replay(agent_mod, g, persist, sps):
    meta = json.loads(bytes(g["meta"]).decode())
    spec = _spec(meta["state_dim"], meta["act_dim"])
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=1, state_mean=torch.from_numpy(g["state_mean"]), state_std=torch.from_numpy(g["state_std"]),
                                 use_inference_cache=False, eval_context_len=meta["context_len"], persist_context=persist)
    a.replay_buffer.seqs_per_sample = sps
    script = [(torch.from_numpy(o).view(1, -1), torch.tensor([float(r)]), torch.tensor([bool(d)]))
              for o, r, d in zip(g["obs"], g["reward"], g["done"])]
    ro = BatchedRollout(a, ScriptedEnv(torch.from_numpy(g["first_obs"]).view(1, -1), script), meta["target_return"], meta["reward_scale"],
                        env_act_dim=meta["act_dim"], persist_context=persist)
    for _ in script:
        ro.step()
    return meta, a.engine.calls


@pytest.mark.parametrize("name,persist,sps", [("plain", False, 1), ("persist_sps2", True, 2)])
def test_windows_equal_the_reference_step_by_step(agent_mod, name, persist, sps):
    """The plain loop, and persist_context with seqs_per_sample = 2 (the window is pruned to the episode finished last).
    Every step of the scripted three-episode trace: the padded (states, returns_to_go, rewards) the reference's predict hands
    its model, bit for bit (every number of the trace is exact in float32)."""
    g = np.load(GOLDEN)
    meta, calls = _replay(agent_mod, g, persist, sps)
    assert len(calls) == len(g["obs"]) == sum(meta["episodes"])
    for t, call in enumerate(calls):
        assert call["counts"] == [int(g[name + "_attention_mask"][t].sum())], (name, t)
        for key in ("states", "returns_to_go", "rewards"):
            assert np.array_equal(call[key][0].numpy(), g[f"{name}_{key}"][t]), (name, t, key)


@pytest.mark.parametrize("sps", [1, 3])
def test_windows_that_span_older_episodes_and_where_the_reference_sums_across_them(agent_mod, sps):
    """seqs_per_sample = 1 keeps eval_context_len timesteps across episode ends, 3 those of the last two episodes.  States, rewards, counts and the returns-to-go of
    every timestep of the episode under way and of the one finished last equal the reference's.  The returns-to-go of OLDER
    episodes' timesteps differ by design: the reference re-runs discount_cumsum over every stored reward at each episode end
    (evaluation.py:219-222), so an older episode's entries also collect the returns of the episodes behind it; lram_step_window
    relabels the finished episode alone (relabel = its length), which leaves older entries at their own episode's returns."""
    g = np.load(GOLDEN)
    name = f"persist_sps{sps}"
    meta, calls = _replay(agent_mod, g, True, sps)
    K, ends = meta["context_len"], np.cumsum(meta["episodes"])
    differing = 0
    for t, call in enumerate(calls):
        assert call["counts"] == [int(g[name + "_attention_mask"][t].sum())], t
        for key in ("states", "rewards"):
            assert np.array_equal(call[key][0].numpy(), g[f"{name}_{key}"][t]), (t, key)
        done_eps = [e for e in ends if e <= t]                        # episodes finished before step t
        recent = t - (done_eps[-2] if len(done_eps) >= 2 else 0) + 1    # timesteps of the current and the last finished episode
        got, want = call["returns_to_go"][0].numpy(), g[name + "_returns_to_go"][t]
        same = np.equal(got, want)
        assert same[max(0, K - recent):].all(), (t, got, want)
        differing += int((~same).sum())
    assert differing > 0, "the trace no longer reaches the case the docstring describes"
