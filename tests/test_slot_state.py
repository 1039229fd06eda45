"""State of individual env slots (lram_state_copy_slots / save / load), the parts that need no GPU: the C surface is declared,
exported and bound; every entry refuses a NULL engine with a message; the host-side list rules; the rollout driver's fork
bookkeeping on a recording stand-in agent.  The device side is held to the engine in tests/test_gpu_slot_state.py."""
import ctypes
import os
import re

import pytest
import torch

from lram_amd import engine
from lram_amd.engine import check_slot_lists
from lram_amd.rollout import BatchedRollout, SyntheticVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lram_hip.h")
SYMBOLS = ("lram_slot_state_numel", "lram_state_copy_slots", "lram_state_save_slots", "lram_state_load_slots")


def test_symbols_are_declared_exported_and_bound(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/lram_hip.h"
        assert name in engine._SYMBOLS, f"{name} is missing from the ctypes table"
        assert getattr(hip_lib, name) is not None
    assert re.search(r"#define\s+LRAM_ABI_VERSION\s+1\b", text)
    assert hip_lib.lram_abi_version() == 1 == engine.LRAM_ABI_VERSION


def test_header_documents_the_record_and_what_is_not_moved():
    text = open(HEADER).read()
    for needle in ("C [NH, DH, DH], n [NH, DH], m [NH], conv [K, inner]", "slstm_state [4, D] (y, c, n, m), conv [K, D]",
                   "ssm_state [d_inner, d_state], conv_state [d_inner, d_conv]", "NOT moved"):
        assert needle in text, needle


def test_every_entry_refuses_a_null_engine_with_a_message(hip_lib):
    idx = (ctypes.c_int32 * 2)(0, 1)
    assert hip_lib.lram_slot_state_numel(None) == 0
    assert b"null engine" in hip_lib.lram_last_error()
    for call in (lambda: hip_lib.lram_state_copy_slots(None, idx, idx, 1, None),
                 lambda: hip_lib.lram_state_save_slots(None, idx, 1, None, None),
                 lambda: hip_lib.lram_state_load_slots(None, idx, 1, None, None)):
        hip_lib.lram_lazy_peek(None, 0, 0, None, None)          # (another failing call: the message below must be the entry's own)
        assert call() != 0
        msg = hip_lib.lram_last_error()
        assert b"lram_state_" in msg and b"_slots" in msg, msg
    assert hip_lib.lram_destroy(None) == 0 and hip_lib.lram_last_error() == b""   # (a succeeding call clears the text again)


def test_check_slot_lists_rules():
    assert check_slot_lists([0, 1], [2, 3], 4) == ([0, 1], [2, 3])
    assert check_slot_lists([0, 0, 0], [1, 2, 3], 4) == ([0, 0, 0], [1, 2, 3])          # a repeated source: fan-out
    assert check_slot_lists([], [], 4) == ([], [])                                      # n = 0: a no-op
    assert check_slot_lists(torch.tensor([1]), torch.tensor([0], dtype=torch.int32), 2) == ([1], [0])
    for src, dst in (([4], [0]), ([-1], [0]), ([0], [4]), ([0], [-1])):                 # out of range
        with pytest.raises(ValueError, match="out of range"):
            check_slot_lists(src, dst, 4)
    with pytest.raises(ValueError, match="twice"):                                      # a duplicate destination
        check_slot_lists([0, 1], [2, 2], 4)
    with pytest.raises(ValueError, match="both source and destination"):                # dst and src intersect
        check_slot_lists([0, 1], [1, 2], 4)
    with pytest.raises(ValueError, match="both source and destination"):
        check_slot_lists([0], [0], 4)
    with pytest.raises(ValueError, match="same length"):
        check_slot_lists([0, 1], [2], 4)
    with pytest.raises(ValueError, match="integer"):
        check_slot_lists([0.5], [1], 4)
    # one list (load_slots): in range and unique
    assert check_slot_lists([3, 1], None, 4) == ([3, 1], None)
    with pytest.raises(ValueError, match="twice"):
        check_slot_lists([1, 1], None, 4)


class _RecordingAgent:
    def __init__(self, n):
        self.n, self.forks, self.steps = n, [], 0

    def predict_batch(self, obs, rtg, rewards, reset_mask, env_act_dim):
        self.steps += 1
        return torch.zeros(self.n, 1)

    def fork_slots(self, src, dst):
        self.forks.append((list(src), list(dst)))


def test_rollout_fork_copies_bookkeeping_env_and_calls_the_agent_once():
    n = 6
    env = SyntheticVecEnv(n, obs_dim=5, ep_len=4, seed=3)      # staggered: env e starts e % 4 steps into its episode
    agent = _RecordingAgent(n)
    ro = BatchedRollout(agent, env, target_return=10.0, reward_scale=2.0)
    for _ in range(3):
        ro.step()
    assert len({int(x) for x in env.t}) > 1 and int(env.episodes.max()) > int(env.episodes.min())
    before = {k: getattr(ro, k).clone() for k in ("obs", "rtg", "timestep", "ep_return", "reset_mask")}
    t0, ep0 = env.t.clone(), env.episodes.clone()
    ro.reset_mask[:] = 1
    src, dst = [0, 0, 3], [1, 2, 5]
    ro.fork_slots(src, dst)
    assert agent.forks == [(src, dst)]
    for s, d in zip(src, dst):
        for k in ("obs", "rtg", "timestep", "ep_return"):
            assert torch.equal(getattr(ro, k)[d], before[k][s]), (k, s, d)
        assert int(ro.reset_mask[d]) == 0
        assert int(env.t[d]) == int(t0[s]) and int(env.episodes[d]) == int(ep0[s])
    for b in (0, 3, 4):                                         # sources and unlisted slots keep everything
        for k in ("obs", "rtg", "timestep", "ep_return"):
            assert torch.equal(getattr(ro, k)[b], before[k][b]), (k, b)
        assert int(ro.reset_mask[b]) == 1
        assert int(env.t[b]) == int(t0[b]) and int(env.episodes[b]) == int(ep0[b])
    with pytest.raises(ValueError):
        ro.fork_slots([0], [0])
    with pytest.raises(ValueError):
        ro.fork_slots([0, 1], [2, 2])
    ro.fork_slots([], [])
    assert len(agent.forks) == 1                                # refused and empty calls never reach the agent
    ro.step()                                                   # the driver goes on
    assert agent.steps == 4


def test_agent_surface_exists():
    from lram_amd.agent import RecurrentAgent
    for name in ("fork_slots", "save_slots", "load_slots"):
        assert callable(getattr(RecurrentAgent, name))
    for name in ("copy_slots", "save_slots", "load_slots"):
        assert callable(getattr(engine.Engine, name))
    assert isinstance(engine.Engine.slot_state_numel, property)
