"""CPU: per-slot sampling settings and the log-probability under the drawn distribution -- the host side and the reference
the GPU tests lean on.

  * tests/sampling_slots_ref.row_logp (float64 numpy, on sampling_ref.row_probs / argmax_rule): its exp() reproduces the
    probabilities recorded from the reference's sample_from_logits (tests/golden/sampling_reference.npz) to 1e-12, the bound
    test_sampling.py holds row_probs to; its edge rules; the seeded rows of the GPU test exercise both classes of answer;
  * the library exports and binds the four new entries, and refuses a null engine with a text naming the entry;
  * Domain(a_sample_kwargs=...) -> SlotTable.sample_settings -> RecurrentAgent -> Engine.set_sampling / set_sampling_slots."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from lram_amd import build, engine, preset
from lram_amd.domains import Domain, SlotTable
from tests import sampling_ref as sr
from tests import sampling_slots_ref as ssr
from tests.stub_engine import StubEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_reference.npz")
NEW_SYMBOLS = ("lram_set_sampling_slots", "lram_get_sampling_slots", "lram_score_last_sampled", "lram_sample_rows")
NEG_INF = float("-inf")


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------
def test_row_logp_reproduces_the_recorded_reference_probabilities():
    g = np.load(GOLDEN)
    for c in range(len(g["n"])):
        n, t, k, p = int(g["n"][c]), float(g["temperature"][c]), int(g["top_k"][c]), float(g["top_p"][c])
        want = g["probs"][c, :n]
        lp = np.array([ssr.row_logp(g["logits"][c, :n], tok, 1, t, k, p) for tok in range(n)])
        assert np.array_equal(lp == NEG_INF, want == 0), g["name"][c]          # the same support
        assert np.abs(np.exp(lp) - want).max() <= 1e-12, (g["name"][c], np.abs(np.exp(lp) - want).max())
        assert abs(np.exp(lp).sum() - 1.0) < 1e-12


def test_row_logp_edge_rules():
    row = np.array([0.5, 2.0, -1.0, 2.0, 0.25], dtype=np.float32)
    assert ssr.row_logp(row, 1, 1, 1.0, 1, 0.0) == 0.0                 # a support of one entry: exactly 0 (the tie: lowest index)
    assert ssr.row_logp(row, 3, 1, 1.0, 1, 0.0) == NEG_INF
    assert ssr.row_logp(row, 1, 1, 3.0, 2, 0.0) == np.log(0.5) and ssr.row_logp(row, 3, 1, 3.0, 2, 0.0) == np.log(0.5)
    for tok in (-2, 5, 2 ** 31 - 1):                                    # outside 0 .. n - 1
        assert ssr.row_logp(row, tok, 1, 1.0, 0, 0.0) == NEG_INF
    assert ssr.row_logp(row, -1, 1, 1.0, 0, 0.0) == 0.0 and ssr.row_logp(row, -1, 0) == 0.0   # the fill value
    assert ssr.row_logp(row, 1, 0, 0.5, 3, 0.5) == 0.0 and ssr.row_logp(row, 3, 0, 0.5, 3, 0.5) == NEG_INF   # greedy
    nan = np.array([0.0, np.nan, 7.0, np.nan], dtype=np.float32)         # the argmax rule: NaN is the maximum, first index
    assert [ssr.row_logp(nan, t, 1, 1.0, 0, 0.5) for t in range(4)] == [NEG_INF, 0.0, NEG_INF, NEG_INF]
    inf = np.array([0.0, np.inf, 1.0, np.inf], dtype=np.float32)
    assert [ssr.row_logp(inf, t) for t in range(4)] == [NEG_INF, 0.0, NEG_INF, NEG_INF]
    assert ssr.row_logp(np.full(4, -np.inf, dtype=np.float32), 0) == 0.0
    hole = np.array([1.0, -np.inf, 0.0], dtype=np.float32)             # a -inf logit has probability 0
    assert ssr.row_logp(hole, 1) == NEG_INF and np.isclose(ssr.row_logp(hole, 0), -np.log1p(np.exp(-1.0)), rtol=0, atol=1e-15)
    # unfiltered: log_softmax(t * x)
    x = np.array([0.3, -1.2, 2.5, 0.0], dtype=np.float32)
    want = torch.log_softmax(0.75 * torch.tensor(x, dtype=torch.float64), -1).numpy()
    got = np.array([ssr.row_logp(x, t, 1, 0.75, 0, 0.0) for t in range(4)])
    assert np.abs(got - want).max() <= 1e-15


@pytest.mark.parametrize("n", [18, 274, 512])
def test_seeded_rows_exercise_both_classes(n):
    """The inputs of the GPU row test: scored at the drawn token on even rows and at a random token on odd rows, at least 10 %
    of the entries are finite and at least 10 % are -inf; the drawn tokens score finite, greedy rows 0."""
    c = ssr.rows_case(n)
    s = (c["mode"], c["temperature"], c["top_k"], c["top_p"])
    assert set(c["top_k"][:-ssr.N_EDGE]) >= {0, 1, 5} and set(c["top_p"]) >= {0.0, 0.5, 1.0}
    assert c["temperature"].min() == 0.25 and c["temperature"].max() == 4.0 and (c["mode"] == 0).sum() >= 10
    drawn = ssr.sample_rows(c["logits"], c["uniform"], *s)
    at_drawn = ssr.rows_logp(c["logits"], drawn, *s)
    assert np.isfinite(at_drawn).all()
    assert (at_drawn[c["mode"] == 0] == 0).all()
    lp = ssr.rows_logp(c["logits"], ssr.scored_tokens(c, drawn), *s)
    assert not np.isnan(lp).any()
    assert np.isfinite(lp).mean() >= 0.10 and (lp == NEG_INF).mean() >= 0.10, (np.isfinite(lp).mean(), (lp == NEG_INF).mean())
    assert ((lp < 0) & np.isfinite(lp)).mean() >= 0.10


# ---- 2. the library -----------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_per_slot_entries(hip_lib):
    header = open(os.path.join(build.CSRC, "..", "..", "include", "lram_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in engine._SYMBOLS and getattr(hip_lib, name).argtypes == engine._SYMBOLS[name][1]
        assert re.search(r"\b%s\s*\(" % name, header)
    assert hip_lib.lram_abi_version() == 1
    assert hip_lib.lram_set_sampling_slots(None, None, None, None, None) != 0
    assert b"lram_set_sampling_slots" in hip_lib.lram_last_error()
    assert hip_lib.lram_get_sampling_slots(None, None, None, None, None, None) != 0
    assert b"lram_get_sampling_slots" in hip_lib.lram_last_error()
    assert hip_lib.lram_score_last_sampled(None, None, None, None) != 0
    assert b"lram_score_last_sampled" in hip_lib.lram_last_error()
    assert hip_lib.lram_sample_rows(None, 1, 18, 18, None, None, None, None, None, None, None, None, None) != 0
    assert b"lram_sample_rows" in hip_lib.lram_last_error()
    for name in ("set_sampling_slots", "sampling_slots"):
        assert hasattr(engine.Engine, name)
    assert callable(engine.sample_rows)
    with pytest.raises(ValueError):
        engine.slot_setting_arrays(4, temperature=[1.0, 2.0])
    with pytest.raises(ValueError):
        engine.slot_setting_arrays(4, top_k=2.5)
    cols = engine.slot_setting_arrays(3, temperature=0.5, top_k=[1, 2, 3], greedy=[True, False, False])
    assert cols["temperature"].tolist() == [0.5] * 3 and cols["top_k"].dtype == torch.int32 and cols["top_p"].tolist() == [0.0] * 3
    assert cols["greedy"].tolist() == [True, False, False]


# ---- 3. Domain -> SlotTable -> RecurrentAgent -> the engine ---------------------------------------------------------------------
class _Engine(StubEngine):
    """tests/stub_engine.StubEngine with Engine's constructor and a record of what the agent sets."""
    made = []

    def __init__(self, spec, state_dict, batch, device=None):
        super().__init__(spec, batch, torch.device("cpu"))
        self.calls, self.closed = [], False
        _Engine.made.append(self)

    def set_sampling(self, temperature=1.0, top_k=0, top_p=0.0, seed=0, slot_base=0):
        self.calls.append(("set_sampling", None if temperature is None else
                           dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, slot_base=slot_base)))

    def set_sampling_slots(self, temperature=1.0, top_k=0, top_p=0.0, greedy=False):
        if temperature is None:
            self.calls.append(("set_sampling_slots", None))
            return
        cols = engine.slot_setting_arrays(self.batch, temperature, top_k, top_p, greedy)
        self.calls.append(("set_sampling_slots", {k: v.tolist() for k, v in cols.items()}))

    def set_slot_table(self, *a):
        self.calls.append(("set_slot_table", None))

    def last_logp(self, tokens, over="selectable", temperature=1.0):
        self.calls.append(("last_logp", over))
        return torch.zeros(self.batch, self.spec.act_dim)

    def close(self):
        self.closed = True

    _tokens = None


@pytest.fixture
def agent_mod(monkeypatch):
    from lram_amd import agent as mod
    monkeypatch.setattr(mod, "Engine", _Engine)
    return mod


def _last(eng, name):
    return [c[1] for c in eng.calls if c[0] == name][-1]


def test_domain_settings_reach_the_engine_per_slot(agent_mod):
    spec = preset("xlstm_tiny")
    assert spec.n_discrete < 40 <= spec.n_vocab
    atari = Domain("atari", True, 1, a_sample_kwargs={"top_k": 5, "temperature": 0.5})
    mw = Domain("metaworld", False, 3, a_sample_kwargs={"top_k": 40})
    dmc = Domain("dmc", False, 2, a_sample_kwargs="greedy")
    plain = Domain("mimicgen", False, 2)
    assert plain.a_sample_kwargs is None and Domain("x", False, 1, False, 1.0, 0.0, None, "greedy").a_sample_kwargs == "greedy"
    tab = SlotTable.from_domains([(atari, 2), (mw, 3), (dmc, 1), (plain, 2)], spec.act_dim)
    cols = tab.sample_settings(spec.n_discrete, spec.n_vocab)
    assert cols["top_k"].tolist() == [5, 5, 40, 40, 40, 0, 0, 0] and cols["top_k"].dtype == torch.int32
    assert cols["temperature"].tolist() == [0.5, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert cols["top_p"].tolist() == [0.5] * 5 + [0.0] * 3                     # completed with sample_from_logits' defaults
    assert cols["greedy"].tolist() == [False] * 5 + [True] * 3               # "greedy", and None without an agent setting
    assert SlotTable.from_domains([(plain, 2)]).sample_settings(spec.n_discrete, spec.n_vocab, {"top_k": 3}) is None

    # a mixed table: the discrete domain no longer caps the continuous domain's top_k
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=8, slot_table=tab, sample_seed=11, sample_slot_base=64)
    eng = a.engine
    assert _last(eng, "set_sampling") == dict(temperature=1.0, top_k=0, top_p=0.0, seed=11, slot_base=64)
    assert _last(eng, "set_sampling_slots") == {k: v.tolist() for k, v in cols.items()}
    mode = a.trajectory_mode
    assert mode["a_sample_kwargs"] == {"seed": 11, "slot_base": 64}
    assert mode["a_sample_slots"] == [
        {"slots": [(0, 2)], "setting": {"temperature": 0.5, "top_k": 5, "top_p": 0.5}},
        {"slots": [(2, 5)], "setting": {"temperature": 1.0, "top_k": 40, "top_p": 0.5}},
        {"slots": [(5, 8)], "setting": "greedy"}]
    # the agent-level setting serves the domains without their own, checked against each one's head
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=8, slot_table=tab, a_sample_kwargs={"top_k": 40, "top_p": 0.0})
    got = _last(a.engine, "set_sampling_slots")
    assert got["top_k"] == [5, 5, 40, 40, 40, 0, 40, 40] and got["greedy"] == [False] * 5 + [True] + [False] * 2
    assert _last(a.engine, "set_sampling")["top_k"] == 40
    # ... and survives the trip through a pickle as plain data
    a.set_slot_sampling([7], {"temperature": 2.0})
    first = a.engine
    a.make_pickleable()
    b = pickle.loads(pickle.dumps(a))
    b.reinit_cuda_kernels()
    assert b.engine is not first and _last(b.engine, "set_sampling_slots")["temperature"][7] == 2.0
    assert _last(b.engine, "set_sampling_slots")["top_k"][:7] == got["top_k"][:7]

    with pytest.raises(ValueError):      # the agent-level top_k falls back on a discrete domain: its 18-logit head refuses it
        agent_mod.RecurrentAgent(spec, {}, n_envs=3, a_sample_kwargs={"top_k": 40},
                                 slot_table=SlotTable.from_domains([(Domain("atari", True, 1), 1), (mw, 2)], spec.act_dim))
    with pytest.raises(ValueError):      # a domain's own top_k against its own head
        agent_mod.RecurrentAgent(spec, {}, n_envs=1, slot_table=SlotTable.from_domains(
            [(Domain("atari", True, 1, a_sample_kwargs={"top_k": spec.n_discrete + 1}), 1)], spec.act_dim))
    agent_mod.RecurrentAgent(spec, {}, n_envs=1, slot_table=SlotTable.from_domains(
        [(Domain("atari", True, 1, a_sample_kwargs={"top_k": spec.n_discrete}), 1)], spec.act_dim))
    with pytest.raises(KeyError):
        agent_mod.RecurrentAgent(spec, {}, n_envs=1, slot_table=SlotTable.from_domains(
            [(Domain("mw", False, 2, a_sample_kwargs={"temp": 1.0}), 1)], spec.act_dim))
    for bad in ({"temperature": 0.0}, {"temperature": float("nan")}, {"top_p": 1.5}, {"top_k": -1}, {"top_k": spec.n_vocab + 1},
                {"top_k": 2.5}):
        with pytest.raises(ValueError):
            agent_mod.RecurrentAgent(spec, {}, n_envs=1, slot_table=SlotTable.from_domains(
                [(Domain("mw", False, 2, a_sample_kwargs=bad), 1)], spec.act_dim))
    with pytest.raises(ValueError):
        Domain("mw", False, 2, a_sample_kwargs="argmax")


def test_nothing_set_is_todays_agent(agent_mod):
    spec = preset("xlstm_tiny")
    tab = SlotTable.from_domains([(Domain("atari", True, 1), 2), (Domain("mw", False, 3), 2)], spec.act_dim)
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=4, slot_table=tab)
    assert [c[0] for c in a.engine.calls] == ["set_slot_table"] and "a_sample_slots" not in a.trajectory_mode
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=4, slot_table=tab, a_sample_kwargs={"top_k": 10})
    assert [c[0] for c in a.engine.calls] == ["set_sampling", "set_slot_table"]      # the engine-wide setting alone
    assert a.trajectory_mode["a_sample_kwargs"]["top_k"] == 10 and "a_sample_slots" not in a.trajectory_mode


def test_set_slot_sampling_ladder_without_a_slot_table(agent_mod):
    spec = preset("xlstm_tiny")
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=8, sample_seed=3)
    assert a.engine.calls == []
    temps = [0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0]
    a.set_slot_sampling(range(8), [{"temperature": t, "top_p": 0.0} for t in temps])
    assert [c[0] for c in a.engine.calls] == ["set_sampling", "set_sampling_slots"]      # the first sampled slot arms
    assert _last(a.engine, "set_sampling")["seed"] == 3
    got = _last(a.engine, "set_sampling_slots")
    assert got["temperature"] == temps and got["greedy"] == [False] * 8 and got["top_p"] == [0.0] * 8
    assert len(a.trajectory_mode["a_sample_slots"]) == 8
    a.set_slot_sampling([0, 1], "greedy")
    assert _last(a.engine, "set_sampling_slots")["greedy"] == [True, True] + [False] * 6
    assert [c[0] for c in a.engine.calls].count("set_sampling") == 1                     # armed once: the draw count is kept
    a.set_slot_sampling(range(8), None)                                                     # nothing left: the argmax agent again
    assert a.engine.calls[-1] == ("set_sampling", None) and "a_sample_slots" not in a.trajectory_mode
    # beside an agent-level setting: unlisted slots keep it, None returns a slot to it
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=4, a_sample_kwargs={"temperature": 0.75, "top_k": 10})
    a.set_slot_sampling([2], "greedy")
    got = _last(a.engine, "set_sampling_slots")
    assert got["greedy"] == [False, False, True, False] and got["top_k"][:2] == [10, 10] and got["top_p"][0] == 0.5
    a.set_slot_sampling([2], None)
    assert a.engine.calls[-1] == ("set_sampling_slots", None)
    a.action_log_prob(over="sampled")
    assert a.engine.calls[-1] == ("last_logp", "sampled")
    # the slot's own head width bounds top_k
    d = agent_mod.RecurrentAgent(spec, {}, n_envs=2, discrete=True)
    with pytest.raises(ValueError):
        d.set_slot_sampling([0], {"top_k": spec.n_discrete + 1})
    with pytest.raises(KeyError):
        d.set_slot_sampling([0], {"temp": 1.0})
    with pytest.raises(IndexError):
        d.set_slot_sampling([2], "greedy")
    with pytest.raises(ValueError):
        d.set_slot_sampling([0, 1], ["greedy"])
    assert d.engine.calls == []
