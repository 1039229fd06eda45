"""CPU: the append entries of the stored-context path (lram_prefill_append, lram_score_append) are declared, bound and refuse bad
calls with a message, and the agent calls built on them -- RecurrentAgent.score_trajectories(window=...) and extend_contexts --
route what they should: per-window lengths, the reset on window 0 only, append=True, one ScoreResult of the full shape.  The
engine is a stand-in defined here (no GPU): its score() answers with a fixed function of the call's inputs."""
import ctypes
import os
import re

import pytest
import torch

from lram_amd import agent as agent_mod
from lram_amd import engine, preset
from lram_amd.rollout import score_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lram_hip.h")
ENTRIES = ("lram_prefill_append", "lram_score_append")


def _declarations():
    """name -> number of parameters, for every function the header declares (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(lram_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_header_declares_both_entries_and_the_abi_version_stays():
    decl = _declarations()
    for name in ENTRIES:
        assert name in decl, name
    # the argument lists of the ragged entries
    assert decl["lram_prefill_append"] == decl["lram_prefill_ragged"] == 12
    assert decl["lram_score_append"] == decl["lram_score_ragged"] == 19
    text = open(HEADER).read()
    assert re.search(r"#define\s+LRAM_ABI_VERSION\s+1\b", text) and engine.LRAM_ABI_VERSION == 1
    # the replace entries no longer list a continuing context as out of scope
    assert "a SHORTER context that CONTINUES a slot's state (needs length-aware state kernels)" not in text


def test_engine_binds_them_like_their_ragged_twins():
    for name, twin in zip(ENTRIES, ("lram_prefill_ragged", "lram_score_ragged")):
        assert name in engine._SYMBOLS, name
        assert engine._SYMBOLS[name] == engine._SYMBOLS[twin], name
        assert len(engine._SYMBOLS[name][1]) == _declarations()[name]
    src = open(os.path.join(ROOT, "lram_amd", "engine.py")).read()
    for name in ENTRIES:   # ... and Engine.prefill / Engine.score call them
        assert re.search(r"lib\.%s\b" % name, src), name
    assert src.count("append: bool = False") == 2


def test_null_engine_and_null_lengths_are_refused_with_a_message(hip_lib):
    null = ctypes.c_void_p()
    assert hip_lib.lram_prefill_append(null, null, 0, null, null, 4, null, null, 0, null, null, null) != 0
    assert b"lram_prefill_append" in hip_lib.lram_last_error()
    assert hip_lib.lram_score_append(null, null, 0, null, null, 4, null, null, 0, null, null, null, 0, 1.0, null, null, null, null,
                                     null) != 0
    assert b"lram_score_append" in hip_lib.lram_last_error()
    # ... as every stored-context entry does (one check for the eight of them, in their shared body), and the three env-step
    # entries (step_entry); every argument null / 0, a temperature of 1
    for name in ("lram_prefill", "lram_score", "lram_prefill_ragged", "lram_score_ragged", "lram_prefill_append",
                 "lram_score_append", "lram_prefill_frames", "lram_score_frames", "lram_step", "lram_step_images",
                 "lram_step_slots"):
        args = [1.0 if t is ctypes.c_double else 0 if t is ctypes.c_int32 else null for t in engine._SYMBOLS[name][1]]
        assert getattr(hip_lib, name)(*args) != 0, name
        assert name.encode() + b":" in hip_lib.lram_last_error(), name
        if name not in ("lram_step", "lram_step_images", "lram_step_slots"):
            assert hip_lib.lram_last_error() == b"lram: " + name.encode() + b": null engine", name
    # (the library is shared by the session: a call that succeeds clears the thread's last error again)
    starts, n = (ctypes.c_int32 * 4)(), ctypes.c_int32()
    assert hip_lib.lram_context_plan(4, 2, (ctypes.c_int32 * 1)(4), 1, starts, 4, ctypes.byref(n)) == 0 and n.value == 2
    assert hip_lib.lram_last_error() == b""
    # NULL lengths: the Python wrapper's own check names them before the library is reached ...
    with pytest.raises((ValueError, TypeError)):
        engine.check_context_lengths(None, 3, 4)
    # ... and the library's check is the ragged entries' (RaggedCall::check), first thing behind the pointer checks
    src = open(os.path.join(ROOT, "lram_amd", "csrc", "engine_context.hip")).read()
    assert 'LRAM_REQUIRE(lengths != nullptr, w + ": host_lengths is NULL")' in src
    assert "if (c.ragged) rc.check(c.in.emb);" in src
    # the append entries describe their call as kAppend, which is what sets Call::append (and makes the lengths mandatory)
    for name in ENTRIES:
        assert 'const Call c = vector_call("%s", kAppend, ' % name in src, name
    assert "c.ragged = kind != kDense, c.host_lengths = host_lengths, c.append = kind == kAppend;" in src
    assert "RaggedCall rc{e, w, c.in.L, c.host_lengths, c.append != 0, {}};" in src


# ---- the agent calls, against a stand-in engine ------------------------------------------------------------------------------------
class StandInEngine:
    """Records every score() / prefill() call and answers score() with a fixed function of the call's inputs: row [b, l] of a
    call holds rtg[b, l] (actions), the window-local l (tokens) and -rtg[b, l] (logp) where l < lengths[b], the engine's fill
    values elsewhere."""

    def __init__(self, spec, state_dict, batch, device=None):
        self.spec, self.batch, self.device = spec, batch, torch.device("cpu")
        self.calls = []
        self._actions = torch.zeros(batch, spec.act_dim)
        self._tokens = torch.zeros(batch, spec.act_dim, dtype=torch.int32)

    def __getattr__(self, name):   # whatever else the agent sets up on its engine
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None

    def score(self, obs, rtg, rew, *, actions=None, reset_mask=None, lengths=None, append=False, want=(), logits=False, **kw):
        B, L = rtg.shape
        A = self.spec.act_dim
        self.calls.append(dict(kind="score", L=L, lengths=None if lengths is None else list(lengths), append=append,
                               reset=None if reset_mask is None else reset_mask.tolist(), obs=obs.clone(), rtg=rtg.clone(),
                               target=None if actions is None else actions.clone()))
        n = torch.tensor([L] * B if lengths is None else list(lengths))
        live = (torch.arange(L).view(1, L) < n.view(B, 1)).view(B, L, 1)
        clean = torch.nan_to_num(rtg, nan=0.0).view(B, L, 1).expand(B, L, A)
        local = torch.arange(L, dtype=torch.int32).view(1, L, 1).expand(B, L, A)
        return engine.ScoreResult(
            actions=torch.where(live, clean, torch.zeros(())) if "actions" in want else None,
            tokens=torch.where(live, local, torch.full((), -1, dtype=torch.int32)) if "tokens" in want else None,
            logp=torch.where(live, -clean, torch.zeros(())) if "logp" in want else None,
            logits=torch.where(live.unsqueeze(-1), clean.unsqueeze(-1).expand(B, L, A, self.spec.n_vocab), torch.zeros(()))
            if logits else None)

    def prefill(self, obs, rtg, rew, reset_mask=None, discrete=False, obs_is_embedding=False, want_action=True, lengths=None,
                append=False):
        self.calls.append(dict(kind="prefill", L=rtg.shape[1], lengths=None if lengths is None else list(lengths), append=append,
                               reset=None if reset_mask is None else reset_mask.tolist(), want_action=want_action,
                               obs=obs.clone()))
        return (self._actions, self._tokens) if want_action else (None, None)


@pytest.fixture()
def agent(monkeypatch):
    monkeypatch.setattr(agent_mod, "Engine", StandInEngine)
    spec = preset("xlstm_tiny")
    return agent_mod.RecurrentAgent(spec, {}, n_envs=4, device="cpu")


def _trajectories(spec, B=4, L=10, n_obs=5, n_act=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand(B, L, n_obs, generator=g)
    rtg = torch.arange(B * L, dtype=torch.float32).view(B, L) + 1.0    # every (env, timestep) has its own value
    rec = torch.rand(B, L, n_act, generator=g) * 2 - 1
    return obs, rtg, rec


def test_windowed_scoring_routes_lengths_reset_and_append(agent):
    spec, eng = agent.spec, agent.engine
    B, L, W = 4, 10, 4
    lengths = [10, 7, 0, 3]
    obs, rtg, rec = _trajectories(spec)
    for b, n in enumerate(lengths):   # padded positions hold NaN
        obs[b, n:], rtg[b, n:] = float("nan"), float("nan")
    res = agent.score_trajectories(obs, rtg, actions=rec, lengths=lengths, window=W, logits=True)
    calls = [c for c in eng.calls if c["kind"] == "score"]
    assert len(calls) == 3 == -(-max(lengths) // W)                      # ceil(max(lengths) / W)
    assert [c["L"] for c in calls] == [4, 4, 2]                           # rows [kW, (k + 1) W) of the trajectory
    assert [c["lengths"] for c in calls] == [[4, 4, 0, 3], [4, 3, 0, 0], [2, 0, 0, 0]]   # clamp(n_b - kW, 0, W)
    assert all(c["append"] is True for c in calls)
    assert calls[0]["reset"] == [1] * B and calls[1]["reset"] is None and calls[2]["reset"] is None   # reset on window 0 only
    for k, c in enumerate(calls):   # every call got its own rows of the observations and of the recorded actions
        lo, hi = k * W, min((k + 1) * W, L)
        assert torch.equal(torch.nan_to_num(c["obs"][..., :5]), torch.nan_to_num(obs[:, lo:hi]))
        assert torch.equal(c["target"][..., :2], rec[:, lo:hi]) and bool((c["target"][..., 2:] == 0).all())
    # one result of the full [B, L, ...] shape, the windows in their places
    A = spec.act_dim
    assert res.actions.shape == res.logp.shape == (B, L, A) and res.tokens.shape == (B, L, A)
    assert res.logits.shape == (B, L, A, spec.n_vocab)
    for b, n in enumerate(lengths):
        want = torch.nan_to_num(rtg[b, :n]).view(n, 1).expand(n, A)
        assert torch.equal(res.actions[b, :n], want) and torch.equal(res.logp[b, :n], -want), b
        assert torch.equal(res.tokens[b, :n, 0], (torch.arange(n) % W).to(torch.int32)), b
        assert bool((res.actions[b, n:] == 0).all()) and bool((res.tokens[b, n:] == -1).all()), b
        assert bool((res.logp[b, n:] == 0).all()) and bool((res.logits[b, n:] == 0).all()), b
    # rollout.score_loss takes the result as it takes a single call's
    valid = torch.arange(L).view(1, L) < torch.tensor(lengths).view(B, 1)
    loss = score_loss(res, valid, reduction="mean")
    assert torch.allclose(loss, torch.nan_to_num(rtg)[valid].mean())


def test_windowed_scoring_without_reset_and_the_single_call(agent):
    eng = agent.engine
    obs, rtg, rec = _trajectories(agent.spec)
    lengths = [10, 7, 0, 3]
    # reset=False: nobody restarts on any window (appended contexts never replace a state, so shorter lengths are accepted)
    agent.score_trajectories(obs, rtg, actions=rec, lengths=lengths, reset=False, window=5)
    calls = [c for c in eng.calls if c["kind"] == "score"]
    assert [c["reset"] for c in calls] == [None, None] and [c["lengths"] for c in calls] == [[5, 5, 0, 3], [5, 2, 0, 0]]
    # no lengths: every env has all L timesteps, the last window is the remainder
    del eng.calls[:]
    agent.score_trajectories(obs, rtg, window=4)
    calls = [c for c in eng.calls if c["kind"] == "score"]
    assert [c["lengths"] for c in calls] == [[4] * 4, [4] * 4, [2] * 4] and all(c["append"] for c in calls)
    # window=None, and a window that holds the whole trajectory: today's single call
    for window in (None, 10, 64):
        del eng.calls[:]
        res = agent.score_trajectories(obs, rtg, actions=rec, lengths=lengths, window=window)
        assert len(eng.calls) == 1 and eng.calls[0]["append"] is False and eng.calls[0]["lengths"] == lengths, window
        assert eng.calls[0]["L"] == 10 and eng.calls[0]["reset"] == [1] * 4 and res.actions.shape[:2] == (4, 10)
    with pytest.raises(ValueError):      # the single call still refuses a replace without a reset
        agent.score_trajectories(obs, rtg, actions=rec, lengths=lengths, reset=False)
    with pytest.raises(ValueError):
        agent.score_trajectories(obs, rtg, window=0)


def test_extend_contexts_appends_and_restarts_only_who_is_named(agent):
    eng = agent.engine
    obs, rtg, _ = _trajectories(agent.spec)
    assert agent.extend_contexts(obs, rtg, lengths=[10, 7, 0, 3]) is None
    c = eng.calls[-1]
    assert c["kind"] == "prefill" and c["append"] is True and c["lengths"] == [10, 7, 0, 3] and c["reset"] is None
    assert c["want_action"] is False and c["obs"].shape == (4, 10, agent.spec.state_dim)   # padded as prime_contexts pads
    assert torch.equal(c["obs"][..., :5], obs) and bool((c["obs"][..., 5:] == 0).all())
    act = agent.extend_contexts(obs, rtg, lengths=torch.tensor([1, 0, 2, 10]), restart=torch.tensor([False, True, False, True]),
                                want_action=True)
    c = eng.calls[-1]
    assert c["reset"] == [0, 1, 0, 1] and c["lengths"] == [1, 0, 2, 10] and c["append"] is True and c["want_action"] is True
    assert act.shape == (4, agent.spec.act_dim)
    agent.extend_contexts(obs, rtg)                       # no lengths: the dense call, still through the append route
    assert eng.calls[-1]["lengths"] is None and eng.calls[-1]["append"] is True
    with pytest.raises(ValueError):
        agent.extend_contexts(obs, rtg, restart=[True, False])
    with pytest.raises(ValueError):
        agent.extend_contexts(obs, rtg, lengths=[11, 0, 0, 0])


# ---- the HOLD instances of the state kernels ---------------------------------------------------------------------------------------
# (file, HOLD instances it must hold): the hold rule is a compile-time switch, one HOLD twin per instance a stored-context chunk
# with a held env can launch -- whole timesteps of three tokens (T = 3, 6, 9, 12) -- and none of them may use scratch memory that
# its parent instance does not use (nor more of it): a state kernel that spills beside a read pass costs every call, not only these.
_HOLD_INSTANCES = {"xlstm_kernels.hip": 66, "mlstm_chunk.hip": 3, "slstm_seq.hip": 10, "mamba_kernels.hip": 7}


@pytest.mark.parametrize("src", sorted(_HOLD_INSTANCES))
def test_hold_instances_use_no_scratch_their_parents_do_not_use(src):
    from tests.test_kernel_resources import _resources
    res = _resources(src)
    hold = sorted(k for k in res if "Lb1EEEv" in k)          # HOLD is every state kernel's last template argument
    assert len(hold) == _HOLD_INSTANCES[src], (src, len(hold))
    for name in hold:
        parent = name.replace("Lb1EEEv", "Lb0EEEv")
        assert parent in res, name
        key = "ScratchSize [bytes/lane]"
        assert res[name][key] <= res[parent][key], (name, res[name][key], res[parent][key])
