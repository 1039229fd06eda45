"""Mixed-domain batches, host side (no GPU): the C ABI entries of the slot table, `lram_amd.domains`, per-slot
`BatchedRollout` arithmetic and `RecurrentAgent(slot_table=...)` with the engine replaced by a recorder."""
import os
import re

import pytest
import torch

from lram_amd import engine, preset
from lram_amd.domains import Domain, SlotTable
from lram_amd.rollout import BatchedRollout, SyntheticVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lram_hip.h")
NEW_SYMBOLS = ("lram_set_slot_table", "lram_get_slot_table", "lram_step_slots", "lram_pad_obs_slots")


def _header():
    return open(HEADER).read()


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m is not None, f"{name} is not declared in include/lram_hip.h"
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_header_symbols_and_library_agree_on_the_slot_entries(hip_lib):
    import ctypes
    text = _header()
    for macro, value in (("LRAM_HEAD_PER_SLOT", 2), ("LRAM_SLOT_DISCRETE", 1), ("LRAM_SLOT_IMAGE", 2)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)", text)
        assert m is not None and int(m.group(1)) == value == getattr(engine, macro), macro
    assert re.search(r"#define\s+LRAM_ABI_VERSION\s+1\b", text) and engine.LRAM_ABI_VERSION == 1   # lram_config is unchanged
    for name in NEW_SYMBOLS:
        args = _declaration(name)
        restype, argtypes = engine._SYMBOLS[name]
        assert restype is ctypes.c_int32 and len(argtypes) == len(args), name
        for decl, ct in zip(args, argtypes):   # every pointer is a void* / typed pointer, every int32_t a c_int32
            if "*" in decl:
                assert ct is engine._VP or issubclass(ct, ctypes._Pointer), (name, decl)
            else:
                assert decl.startswith("int32_t") and ct is ctypes.c_int32, (name, decl)
        fn = getattr(hip_lib, name)
        assert fn.restype is ctypes.c_int32 and list(fn.argtypes) == list(argtypes)
    # argument validation that needs no device: a NULL engine / NULL buffers are refused with a message
    assert hip_lib.lram_set_slot_table(None, None, None) != 0 and b"lram_set_slot_table" in hip_lib.lram_last_error()
    assert hip_lib.lram_step_slots(None, None, None, 0, 0, 0, None, None, None, None, None, None) != 0
    assert b"lram_step_slots" in hip_lib.lram_last_error()
    assert hip_lib.lram_pad_obs_slots(None, 3, None, None, None, None, 1, None, 2, 4, None) != 0
    assert b"lram_pad_obs_slots" in hip_lib.lram_last_error()
    assert hip_lib.lram_destroy(None) == 0 and hip_lib.lram_last_error() == b""   # (a call that succeeds clears the text)
    assert engine._head_mode(False) == 0 and engine._head_mode(True) == 1 and engine._head_mode("per_slot") == 2
    with pytest.raises(ValueError):
        engine._head_mode("per-slot")


ATARI = Domain("atari", discrete=True, act_dim=1, image=True, reward_scale=20.0, target_return=90.0)
METAWORLD = Domain("metaworld", discrete=False, act_dim=4, reward_scale=200.0, target_return=1500.0)
DMC = Domain("dmcontrol", discrete=False, act_dim=6, reward_scale=100.0, target_return=1000.0,
             inv_index=[-1, 0, 1, -1, 2, -1, -1, -1])


def test_slot_table_layout():
    tab = SlotTable.from_domains([(ATARI, 3), (METAWORLD, 2), (DMC, 4)], max_act_dim=8)
    assert tab.n_slots == 9 and tab.ranges == [(0, 3), (3, 5), (5, 9)]
    d, a, i = tab.engine_arrays()
    assert d.tolist() == [True] * 3 + [False] * 6 and d.dtype == torch.bool
    assert a.tolist() == [1] * 3 + [4] * 2 + [6] * 4
    assert i.tolist() == [True] * 3 + [False] * 6
    assert tab.n_image == 3 and tab.image_slots.tolist() == [0, 1, 2] and tab.vector_slots.tolist() == [3, 4, 5, 6, 7, 8]
    assert list(tab.slots_of("metaworld")) == [3, 4] and tab.domain_of(8) is DMC and tab.find("atari") is ATARI and tab.find(1) is METAWORLD
    # per-slot rtg0 = float(target) / float(scale), rounded to fp32 once (what BatchedRollout computes for one domain)
    want = [90.0 / 20.0] * 3 + [1500.0 / 200.0] * 2 + [1000.0 / 100.0] * 4
    assert tab.rtg0.dtype == torch.float32 and tab.rtg0.tolist() == torch.tensor(want, dtype=torch.float32).tolist()
    assert tab.reward_scale.tolist() == [20.0] * 3 + [200.0] * 2 + [100.0] * 4
    third = SlotTable.from_domains([(Domain("x", False, 1, reward_scale=3.0, target_return=0.1), 2)])
    assert third.rtg0.tolist() == torch.tensor([0.1 / 3.0] * 2, dtype=torch.float32).tolist()
    rows, inv = tab.pad_tables(8)
    assert rows.dtype == torch.int32 and rows.tolist() == [0] * 3 + [1] * 2 + [2] * 4
    assert inv.shape == (3, 8) and inv[0].tolist() == [-1] * 8 and inv[1].tolist() == list(range(8)) and inv[2].tolist() == list(DMC.inv_index)
    # interleaved domains: image slots in ascending order whatever the layout
    tab2 = SlotTable.from_domains([(METAWORLD, 1), (ATARI, 2), (DMC, 1), (Domain("procgen", True, 1, image=True), 1)])
    assert tab2.image_slots.tolist() == [1, 2, 4]


def test_slot_table_validation():
    with pytest.raises(ValueError):
        Domain("bad", discrete=True, act_dim=2)            # a discrete domain has one action column
    with pytest.raises(ValueError):
        Domain("bad", discrete=False, act_dim=0)
    with pytest.raises(ValueError):
        Domain("bad", discrete=False, act_dim=2, reward_scale=0.0)
    with pytest.raises(ValueError):
        Domain("bad", discrete=True, act_dim=1, image=True, inv_index=[0, 1])
    with pytest.raises(ValueError):
        SlotTable.from_domains([])
    with pytest.raises(ValueError):
        SlotTable.from_domains([(ATARI, 0)])
    with pytest.raises(ValueError):
        SlotTable.from_domains([(ATARI, 2), (ATARI, 1)])   # one range per domain
    with pytest.raises(ValueError):
        SlotTable.from_domains([(DMC, 2)], max_act_dim=4)  # 6 action dims on a 4-dim model
    with pytest.raises(TypeError):
        SlotTable.from_domains([("atari", 2)])
    with pytest.raises(ValueError):
        SlotTable.from_domains([(DMC, 2)]).pad_tables(9)   # inv_index row of the wrong width
    with pytest.raises(KeyError):
        SlotTable.from_domains([(DMC, 2)]).find("atari")


class _StubAgent:
    def __init__(self):
        self.calls = []

    def predict_batch(self, obs, rtg, rewards, reset_mask, env_act_dim):
        self.calls.append((rtg.clone(), reset_mask.clone()))
        return torch.zeros(rtg.shape[0], 1)


# BatchedRollout(stub agent, SyntheticVecEnv(4, obs_dim=3, act_dim=1, ep_len=3, seed=7), target_return=7.5, reward_scale=3.0)
# run on the commit before per-slot tensors existed: the bit patterns of `rtg` (fp32), `reset_mask` and `timestep` after each of
# six steps.  The float path must keep producing exactly these.
PARENT_TRAJECTORY = [
    ([1074440875, 1074440875, 1075838976, 1074440875], [0, 0, 1, 0], [1, 1, 0, 1]),
    ([1072343723, 1075838976, 1074440875, 1072343723], [0, 1, 0, 0], [2, 0, 1, 2]),
    ([1075838976, 1074440875, 1072343723, 1075838976], [1, 0, 0, 1], [0, 1, 2, 0]),
    ([1074440875, 1072343723, 1075838976, 1074440875], [0, 0, 1, 0], [1, 2, 0, 1]),
    ([1072343723, 1075838976, 1074440875, 1072343723], [0, 1, 0, 0], [2, 0, 1, 2]),
    ([1075838976, 1074440875, 1072343723, 1075838976], [1, 0, 0, 1], [0, 1, 2, 0]),
]


def test_rollout_with_floats_keeps_the_recorded_trajectory():
    env = SyntheticVecEnv(4, obs_dim=3, act_dim=1, ep_len=3, seed=7, stagger=True)
    ro = BatchedRollout(_StubAgent(), env, target_return=7.5, reward_scale=3.0)
    assert isinstance(ro.rtg0, float) and isinstance(ro.reward_scale, float)
    for rtg_bits, mask, ts in PARENT_TRAJECTORY:
        ro.step()
        assert ro.rtg.dtype == torch.float32 and ro.rtg.view(torch.int32).tolist() == rtg_bits
        assert ro.reset_mask.tolist() == mask and ro.timestep.tolist() == ts


def test_rollout_with_per_slot_tensors_equals_one_slot_rollouts():
    """Slot b of a rollout with [B] tensors follows rtg - r / reward_scale[b] and restarts at target[b] / reward_scale[b]: bit
    for bit the one-slot rollout with that slot's floats."""
    targets, scales = [7.5, 90.0, 0.1, 1500.0, 33.0], [3.0, 20.0, 7.0, 200.0, 0.3]
    B, steps, ep_len = len(targets), 9, 4

    class OneSlotEnv(SyntheticVecEnv):     # slot b of the wide env: the same episode phase
        def __init__(self, b):
            super().__init__(1, obs_dim=3, act_dim=1, ep_len=ep_len, seed=7, stagger=False)
            self.t = torch.tensor([b % ep_len])

    agent = _StubAgent()
    wide = BatchedRollout(agent, SyntheticVecEnv(B, obs_dim=3, act_dim=1, ep_len=ep_len, seed=7, stagger=True),
                          target_return=torch.tensor(targets, dtype=torch.float64), reward_scale=torch.tensor(scales, dtype=torch.float64))
    assert wide.rtg0.dtype == torch.float32 and wide.reward_scale.dtype == torch.float32
    singles = [BatchedRollout(_StubAgent(), OneSlotEnv(b), target_return=targets[b], reward_scale=scales[b]) for b in range(B)]
    assert wide.rtg.view(torch.int32).tolist() == [int(s.rtg.view(torch.int32)[0]) for s in singles]
    ends = 0
    for _ in range(steps):
        wide.step()
        for s in singles:
            s.step()
        assert wide.rtg.view(torch.int32).tolist() == [int(s.rtg.view(torch.int32)[0]) for s in singles]
        assert wide.reset_mask.tolist() == [int(s.reset_mask[0]) for s in singles]
        assert wide.timestep.tolist() == [int(s.timestep[0]) for s in singles]
        ends += int(wide.last_done.sum())
    assert ends >= 2 * B - 2                       # every slot went through episode ends
    # what the agent was handed: the per-slot rtg of the step before, and the first call resets every slot
    assert bool(agent.calls[0][1].all()) and agent.calls[0][0].tolist() == wide.rtg0.tolist()
    # the table's tensors go straight in
    tab = SlotTable.from_domains([(Domain(f"d{b}", False, 1, reward_scale=scales[b], target_return=targets[b]), 1) for b in range(B)])
    via_table = BatchedRollout(_StubAgent(), SyntheticVecEnv(B, obs_dim=3, ep_len=ep_len, seed=7), tab.target_return, tab.reward_scale)
    assert via_table.rtg0.view(torch.int32).tolist() == tab.rtg0.view(torch.int32).tolist()
    assert via_table.rtg0.tolist() == [float(torch.tensor(t / sc, dtype=torch.float32)) for t, sc in zip(targets, scales)]
    with pytest.raises(ValueError):
        BatchedRollout(_StubAgent(), SyntheticVecEnv(B, obs_dim=3), torch.zeros(B + 1), 1.0)


def test_agent_with_slot_table_drives_step_slots():
    """RecurrentAgent(slot_table=...) with the engine replaced by a recorder: what reaches Engine.step_slots (padded and
    normalised vector rows, frames as they are, per-slot rtg, reward token 0, reset mask) and what comes back."""
    from lram_amd.agent import RecurrentAgent, _InferenceParams
    spec = preset("xlstm_tiny")
    A, S = spec.act_dim, spec.state_dim
    tab = SlotTable.from_domains([(Domain("procgen", True, 1, image=True, reward_scale=10.0, target_return=40.0), 2),
                                  (Domain("metaworld", False, min(A, 3), reward_scale=200.0, target_return=1500.0), 3)],
                                 max_act_dim=A)
    canned = torch.arange(5 * A, dtype=torch.float32).reshape(5, A)

    class Recorder:
        def __init__(self):
            self.calls, self.tables, self.device = [], [], torch.device("cpu")

        def set_slot_table(self, discrete, act_dim, image):
            self.tables.append((discrete.tolist(), act_dim.tolist(), image.tolist()))

        def step_slots(self, obs, images, rtg, reward, reset_mask=None, out_actions=None, out_tokens=None):
            self.calls.append((obs, images, rtg, reward, reset_mask))
            return canned, None

        def step(self, *a, **k):
            raise AssertionError("a slot-table agent must not call Engine.step")

        step_images = step

    agent = object.__new__(RecurrentAgent)
    agent.spec, agent.slot_table = spec, tab
    agent.engine, agent.device, agent.n_envs, agent.is_discrete = Recorder(), torch.device("cpu"), 5, False
    agent.policy, agent.has_image_encoder = agent, True
    agent.state_mean, agent.state_std = torch.full((S,), 0.5), torch.full((S,), 2.0)
    agent._zero_reward = torch.zeros(5)
    agent.target_return, agent.reward_scale = 1.25, 8.0
    agent.inference_params = _InferenceParams(agent)
    agent._apply_slot_table()
    assert agent.engine.tables == [([True, True, False, False, False], [1, 1, 3, 3, 3] if A >= 3 else [1, 1] + [A] * 3,
                                    [True, True, False, False, False])]
    assert agent.slot_is_discrete.tolist() == [True, True, False, False, False]
    vec = torch.rand(5, 7, generator=torch.Generator().manual_seed(3))
    frames = torch.randint(0, 256, (2, 3, 8, 8), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    mask = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    out = agent.predict_batch((vec, frames), tab.rtg0, None, mask, env_act_dim=2)
    obs, images, rtg, reward, reset_mask = agent.engine.calls[0]
    assert obs.shape == (5, S) and obs.dtype == torch.float32 and obs.is_contiguous()
    padded = torch.cat([vec, torch.zeros(5, S - 7)], dim=1)
    assert torch.equal(obs, (padded - 0.5) / 2.0)                       # pad_inputs, then (x - mean) / std
    assert images.dtype == torch.uint8 and torch.equal(images, frames)
    assert rtg.tolist() == [4.0, 4.0, 7.5, 7.5, 7.5] and reward.tolist() == [0.0] * 5 and torch.equal(reset_mask, mask)
    assert out.dtype == torch.float32 and out.shape == (5, A) and torch.equal(out, canned)   # every column, whatever env_act_dim says
    # per-domain lookups (decision_transformer_sb3.py:373-382,542-559); without a name the agent's own scalars
    assert agent.get_reward_scale_for_env("procgen") == 10.0 and agent.get_reward_scale_for_env(1) == 200.0
    assert agent.get_reward_scale_for_env(None) == 8.0
    assert agent.compute_target_return_val(task_id="metaworld") == 7.5 and agent.compute_target_return_val(task_id=0) == 4.0
    assert agent.compute_target_return_val(task_id=None) == 1.25
    # shape errors: the frame count is the table's image count, observations come as a pair
    with pytest.raises(ValueError):
        agent.predict_batch((vec, frames[:1]), tab.rtg0, None, mask)
    with pytest.raises(ValueError):
        agent.predict_batch(vec, tab.rtg0, None, mask)
    with pytest.raises(ValueError):
        agent.predict_batch((None, frames), tab.rtg0, None, mask)
    # without a table the surface is what it was
    plain = object.__new__(RecurrentAgent)
    plain.n_envs, plain.is_discrete, plain.target_return, plain.reward_scale = 3, True, 2.0, 5.0
    assert plain.slot_is_discrete.tolist() == [True] * 3
    assert plain.compute_target_return_val(task_id=7) == 2.0 and plain.get_reward_scale_for_env("x") == 5.0
