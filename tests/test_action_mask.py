"""CPU: per-slot allowed-action sets -- the numpy restatement (tests/action_mask_ref.py), the host helpers of lram_amd.engine
(pack / unpack / check_action_mask), Domain / SlotTable.action_mask, the agent's plumbing on a stub engine, and the conditions
on the seeded fixture that keep tests/test_gpu_action_mask.py from passing by accident."""
import pickle

import numpy as np
import pytest
import torch

from lram_amd import engine, preset
from lram_amd.domains import Domain, SlotTable
from lram_amd.engine import check_action_mask, check_swap_lists, pack_action_mask, unpack_action_mask
from tests import action_mask_ref as amr
from tests import sampling_ref as sr
from tests import sampling_slots_ref as ssr
from tests.stub_engine import StubEngine

NEG_INF = float("-inf")
PONG = (0, 1, 3, 4, 11, 12)
SIZES = (18, 274, 512)


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    c = amr.mask_rows_case(request.param)
    s = (c["mode"], c["temperature"], c["top_k"], c["top_p"])
    want = amr.masked_sample_rows(c["logits"], c["uniform"], c["allow"], *s)
    return c, s, want


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_everything_allowed_is_the_unmasked_restatement(n):
    c = ssr.rows_case(n)
    s = (c["mode"], c["temperature"], c["top_k"], c["top_p"])
    R = len(c["uniform"])
    full = np.ones((R, n), dtype=bool)
    want = ssr.sample_rows(c["logits"], c["uniform"], *s)
    assert np.array_equal(amr.masked_sample_rows(c["logits"], c["uniform"], full, *s), want)
    tokens = ssr.scored_tokens(c, want)
    a, b = amr.masked_rows_logp(c["logits"], tokens, full, *s), ssr.rows_logp(c["logits"], tokens, *s)
    assert np.array_equal(a, b, equal_nan=True)
    for r in range(R):
        assert amr.masked_argmax(c["logits"][r], full[r]) == sr.argmax_rule(c["logits"][r])
        p = amr.masked_row_probs(c["logits"][r], full[r], s[1][r], s[2][r], s[3][r])
        q = sr.row_probs(c["logits"][r], s[1][r], s[2][r], s[3][r])
        assert (p is None) == (q is None) and (p is None or np.array_equal(p, q))


def test_the_score_restatement_is_log_softmax_of_the_sub_row():
    g = torch.Generator().manual_seed(3)
    row = (torch.randn(82, generator=g) * 3).numpy()
    allow = np.zeros(82, dtype=bool)
    allow[[0, 1, 3, 4, 11, 12, 40, 81]] = True
    sub = torch.log_softmax(0.5 * torch.tensor(row[[0, 1, 3, 4, 11, 12]], dtype=torch.float64), -1)
    for i, t in enumerate((0, 1, 3, 4, 11, 12)):
        assert amr.masked_score_logp(row, t, allow, 18, "selectable", 0.5) == pytest.approx(float(sub[i]), rel=1e-14, abs=1e-14)
    for t in (2, 17, 40, 81, -1, 82):                       # disallowed, allowed but outside the range, outside the row
        assert amr.masked_score_logp(row, t, allow, 18, "selectable") == NEG_INF
    whole = torch.log_softmax(torch.tensor(row, dtype=torch.float64), -1)
    assert amr.masked_score_logp(row, 2, allow, 18, "vocab") == pytest.approx(float(whole[2]), rel=1e-14)
    assert amr.masked_score_logp(row, 82, allow, 18, "vocab") == NEG_INF
    row[2] = np.nan                                          # a disallowed NaN is invisible to the sub-row, not to the vocabulary
    assert np.isfinite(amr.masked_score_logp(row, 3, allow, 18, "selectable")) and amr.masked_argmax(row, allow, 18) != 2
    assert np.isnan(amr.masked_score_logp(row, 3, allow, 18, "vocab"))
    row[3] = np.nan
    assert np.isnan(amr.masked_score_logp(row, 4, allow, 18, "selectable")) and amr.masked_argmax(row, allow, 18) == 3


# ---- 2. the fixture -------------------------------------------------------------------------------------------------------------
def test_fixture_classes_and_word_boundaries(case):
    c, s, want = case
    allow, logits = c["allow"], c["logits"]
    R, n = allow.shape
    e = R - ssr.N_EDGE
    plain = np.array([sr.argmax_rule(ssr.rows_case(n)["logits"][r]) for r in range(R)])
    for r in range(e):
        k, sub = r % 8, logits[r][allow[r]]
        assert allow[r].any()
        if k == 0:
            assert allow[r].all()
        elif k == 1:
            assert allow[r].sum() == 1 and not allow[r, plain[r]]
        elif k == 2:
            assert allow[r].sum() == n - 1 and not allow[r, plain[r]]
        elif k == 3:
            assert np.array_equal(allow[r], np.arange(n) % 2 == (r // 8) % 2)
        elif k == 4:
            assert np.array_equal(np.flatnonzero(allow[r]), np.arange(32, 64) if n > 32 else np.arange(n))
        elif k == 5:
            assert (sub == NEG_INF).all()
        elif k == 6:
            assert not np.isnan(sub).any() and np.isnan(logits[r][~allow[r]]).sum() == 1
        else:
            assert np.isnan(sub).sum() == 1 and not np.isnan(logits[r][~allow[r]]).any()
    assert not allow[e, 5] and np.isnan(logits[e, 5]) and not allow[e + 1, 3] and not allow[e + 3, 2] and not allow[e + 5, 0]
    assert amr.masked_argmax(logits[e + 1], allow[e + 1]) == 7 and amr.masked_argmax(logits[e + 5], allow[e + 5]) == 1
    kept = np.flatnonzero(amr.masked_row_probs(logits[e + 3], allow[e + 3], 1.0, 2, 0.0) > 0)
    assert kept.tolist() == [9, n - 1]                       # the lowest maximum is disallowed: the next two stay
    # set and cleared bits on both sides of every word boundary, in the partial last word, and at bit n - 1
    for b in list(range(32, n, 32)) + [n]:
        for bit in (b - 1, min(b, n - 1)):
            assert allow[:, bit].any() and not allow[:, bit].all(), (n, bit)
    sampled = c["mode"] == 1
    assert ((c["top_k"] > allow.sum(1)) & sampled).any(), "no sampled row has top_k above its m"


def test_fixture_conditions_of_the_gpu_test(case):
    c, s, want = case
    allow, logits = c["allow"], c["logits"]
    R, n = allow.shape
    rows = np.arange(R)
    assert allow[rows, want].all(), "the restatement returned a disallowed token"
    greedy = np.array([amr.masked_argmax(logits[r], allow[r]) for r in range(R)])
    plain = np.array([sr.argmax_rule(logits[r]) for r in range(R)])
    assert (greedy != plain).mean() >= 0.20
    sampled = c["mode"] == 1
    unmasked = ssr.sample_rows(logits, c["uniform"], *s)
    assert (~allow[rows, unmasked])[sampled].mean() >= 0.10
    ref = amr.masked_rows_logp(logits, ssr.scored_tokens(c, want), allow, *s)
    assert np.isfinite(ref).mean() >= 0.10 and (ref == NEG_INF).mean() >= 0.10
    # two fp64 evaluations of a CDF differ by a few 1e-16 per term over <= 512 terms: at 1e-9 rounding cannot flip a token
    assert amr.cdf_margin(c).min() >= 1e-9
    assert np.array_equal(amr.masked_rows_logp(logits, np.full(R, -1), allow, *s), np.zeros(R))
    assert np.isfinite(amr.masked_rows_logp(logits, want, allow, *s)).all(), "a drawn token scores -inf"


# ---- 3. the host helpers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 18, 32, 33, 64, 65, 274, 512, 518])
def test_pack_and_unpack_round_trip(n):
    g = torch.Generator().manual_seed(n)
    m = torch.rand(5, n, generator=g) < 0.5
    m[0], m[1] = True, False
    m[2] = torch.arange(n) == n - 1
    w = pack_action_mask(m)
    assert w.dtype == torch.int32 and tuple(w.shape) == (5, (n + 31) // 32) and w.is_contiguous()
    assert torch.equal(unpack_action_mask(w, n), m)
    assert torch.equal(pack_action_mask(m.numpy()), w) and torch.equal(pack_action_mask(m.to(torch.uint8)), w)
    u = w.to(torch.int64) & 0xFFFFFFFF
    for t in (0, n // 2, n - 1):                             # bit t & 31 of word t >> 5
        assert torch.equal((u[:, t >> 5] >> (t & 31)) & 1, m[:, t].to(torch.int64))
    if n % 32:
        assert int((u[:, -1] >> (n % 32)).sum()) == 0        # nothing at or above n
    assert int(u[2, (n - 1) >> 5]) == 1 << ((n - 1) & 31) and int(u[2].sum()) == 1 << ((n - 1) & 31)
    with pytest.raises(ValueError):
        unpack_action_mask(w[:, :-1] if w.shape[1] > 1 else torch.zeros(5, 2, dtype=torch.int32), n)
    with pytest.raises(ValueError):
        pack_action_mask(torch.rand(5, n))
    with pytest.raises(ValueError):
        pack_action_mask(torch.zeros(n, dtype=torch.bool))


def test_check_action_mask_refusals():
    B, V, ND = 4, 82, 18
    ok = torch.ones(B, V, dtype=torch.bool)
    assert torch.equal(check_action_mask(ok, B, V, ND), ok)
    assert check_action_mask(ok.numpy().astype(np.uint8), B, V, ND).dtype == torch.bool
    for bad in (torch.ones(B - 1, V, dtype=torch.bool), torch.ones(B, V + 1, dtype=torch.bool), torch.ones(B * V, dtype=torch.bool)):
        with pytest.raises(ValueError, match="expected bool"):
            check_action_mask(bad, B, V, ND)
    with pytest.raises(ValueError, match="expected bools"):
        check_action_mask(torch.full((B, V), 0.5), B, V, ND)
    with pytest.raises(ValueError, match="expected bools"):
        check_action_mask(torch.full((B, V), 2), B, V, ND)
    empty = ok.clone()
    empty[2] = False
    with pytest.raises(ValueError, match="slot 2 allows nothing"):
        check_action_mask(empty, B, V, ND)
    cont = ok.clone()
    cont[1, :ND] = False                                     # nothing below n_discrete: fine until the slot is discrete
    check_action_mask(cont, B, V, ND)
    check_action_mask(cont, B, V, ND, slot_discrete=[True, False, False, True])
    with pytest.raises(ValueError, match="slot 1 allows nothing"):
        check_action_mask(cont, B, V, ND, slot_discrete=[False, True, False, False])
    only_disc = torch.zeros(B, V, dtype=torch.bool)
    only_disc[:, 3] = True                                   # one action: inside both ranges
    check_action_mask(only_disc, B, V, ND, slot_discrete=[True] * B)
    check_action_mask(only_disc, B, V, ND)
    with pytest.raises(ValueError, match="slot_discrete"):
        check_action_mask(ok, B, V, ND, slot_discrete=[True] * (B + 1))
    with pytest.raises(ValueError, match="n_discrete >= 1"):
        check_action_mask(ok, B, V, 0, slot_discrete=[True] * B)


def test_engine_surface(hip_lib):
    for name in ("set_action_mask", "action_mask"):
        assert hasattr(engine.Engine, name)
    for name in ("lram_set_action_mask", "lram_get_action_mask", "lram_sample_rows_masked", "lram_score_tokens_masked"):
        assert name in engine._SYMBOLS and getattr(hip_lib, name) is not None
    assert engine.LRAM_ABI_VERSION == 1
    # null pointers are refused with a text, without a GPU
    assert hip_lib.lram_sample_rows_masked(None, 1, 18, 18, None, None, None, None, None, None, None, None, None, 1, None) != 0
    assert b"lram_sample_rows_masked" in hip_lib.lram_last_error()
    assert hip_lib.lram_set_action_mask(None, None, 0) != 0 and b"lram_set_action_mask" in hip_lib.lram_last_error()
    # each score entry names itself, though the two share their body
    assert hip_lib.lram_score_tokens_masked(None, 1, 1, 18, 18, 1, -1.0, 1.0, 0, None, None, None, 0, 1.0, None, None, None, None, 1,
                                            None) != 0
    assert hip_lib.lram_last_error().startswith(b"lram: lram_score_tokens_masked:"), hip_lib.lram_last_error()
    assert hip_lib.lram_score_tokens(None, 1, 1, 18, 18, 1, -1.0, 1.0, 0, None, None, None, 0, 1.0, None, None, None, None) != 0
    assert hip_lib.lram_last_error().startswith(b"lram: lram_score_tokens:"), hip_lib.lram_last_error()
    # (a call that succeeds clears the error text: the tests behind this one find the library as a fresh process does)
    import ctypes
    starts, lengths, n = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 1)(4), ctypes.c_int32(0)
    assert hip_lib.lram_context_plan(4, 4, lengths, 1, starts, 4, ctypes.byref(n)) == 0, hip_lib.lram_last_error()
    assert hip_lib.lram_last_error() == b""


# ---- 4. Domain / SlotTable ---------------------------------------------------------------------------------------------------------
def test_domains_state_their_sets():
    V, ND = 274, 18
    procgen = Domain("procgen", True, 1, image=True, allowed_actions=range(15))
    pong = Domain("pong", True, 1, image=True, allowed_actions=PONG)
    mw = Domain("metaworld", False, 4, allowed_actions=[18, 273, 100])
    dmc = Domain("dmc", False, 2)
    assert procgen.allowed_actions == tuple(range(15)) and pong.allowed_actions == PONG and dmc.allowed_actions is None
    tab = SlotTable.from_domains([(procgen, 2), (dmc, 1), (pong, 3), (mw, 2)], 4)
    m = tab.action_mask(V, ND)
    assert m.dtype == torch.bool and tuple(m.shape) == (8, V)
    assert [torch.nonzero(m[b]).reshape(-1).tolist() for b in (0, 1)] == [list(range(15))] * 2
    assert bool(m[2].all())
    assert all(torch.nonzero(m[b]).reshape(-1).tolist() == list(PONG) for b in (3, 4, 5))
    assert all(torch.nonzero(m[b]).reshape(-1).tolist() == [18, 100, 273] for b in (6, 7))
    check_action_mask(m, 8, V, ND, tab.discrete)
    assert SlotTable.from_domains([(dmc, 2)]).action_mask(V, ND) is None
    for bad in ([], [1, 1], [-1], [0.5], [True]):
        with pytest.raises(ValueError, match="allowed_actions"):
            Domain("x", True, 1, allowed_actions=bad)
    with pytest.raises(ValueError, match=r"allowed_actions \[18\]"):      # a discrete domain's indices are actions below n_discrete
        SlotTable.from_domains([(Domain("x", True, 1, allowed_actions=[3, 18]), 1)]).action_mask(V, ND)
    with pytest.raises(ValueError, match=r"allowed_actions \[274\]"):
        SlotTable.from_domains([(Domain("x", False, 1, allowed_actions=[274]), 1)]).action_mask(V, ND)
    assert pickle.loads(pickle.dumps(pong)) == pong


# ---- 5. the agent on a recording engine ----------------------------------------------------------------------------------------------
class _Engine(StubEngine):
    """tests/stub_engine.StubEngine with Engine's constructor, set_action_mask with Engine's checks, and a record of the calls."""

    def __init__(self, spec, state_dict, batch, device=None):
        super().__init__(spec, batch, torch.device("cpu"))
        self.calls, self.mask, self.discrete, self.live = [], None, None, batch
        self._tokens = torch.zeros(batch, spec.act_dim, dtype=torch.int32)

    def set_slot_table(self, discrete=None, act_dim=None, image=None):
        self.discrete = None if discrete is None else torch.as_tensor(discrete).bool()
        self.calls.append(("set_slot_table",))

    def set_action_mask(self, allowed):
        if allowed is not None:
            allowed = check_action_mask(allowed, self.batch, self.spec.n_vocab, self.spec.n_discrete, self.discrete).clone()
        self.mask = allowed
        self.calls.append(("set_action_mask", None if allowed is None else allowed.clone()))

    def set_live(self, n):
        self.live = n
        self.calls.append(("set_live", n))

    def swap_slots(self, a, b):
        check_swap_lists(a, b, self.batch)
        self.calls.append(("swap", list(a), list(b)))

    def set_sampling(self, *a, **k):
        pass

    def set_sampling_slots(self, *a, **k):
        pass

    def close(self):
        pass


@pytest.fixture
def agent_mod(monkeypatch):
    from lram_amd import agent as mod
    monkeypatch.setattr(mod, "Engine", _Engine)
    return mod


def _sets(mask):
    return [torch.nonzero(r).reshape(-1).tolist() for r in mask]


def test_the_slot_tables_sets_reach_the_engine(agent_mod):
    spec = preset("xlstm_tiny")
    V, ND = spec.n_vocab, spec.n_discrete
    pong = Domain("pong", True, 1, allowed_actions=PONG)
    procgen = Domain("procgen", True, 1, allowed_actions=range(15))
    dmc = Domain("dmc", False, 2)
    tab = SlotTable.from_domains([(pong, 2), (dmc, 2), (procgen, 2)], spec.act_dim)
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=6, slot_table=tab)
    eng = a.engine
    assert [c[0] for c in eng.calls] == ["set_slot_table", "set_action_mask"]
    assert torch.equal(eng.mask, tab.action_mask(V, ND))
    assert a.trajectory_mode["a_allowed"] == [{"slots": [(0, 2)], "allowed": list(PONG)}, {"slots": [(2, 4)], "allowed": "all"},
                                              {"slots": [(4, 6)], "allowed": list(range(15))}]
    # a table without sets: the engine is never asked, the record stays as it was
    b = agent_mod.RecurrentAgent(spec, {}, n_envs=2, slot_table=SlotTable.from_domains([(dmc, 2)], spec.act_dim))
    assert [c[0] for c in b.engine.calls] == ["set_slot_table"] and "a_allowed" not in b.trajectory_mode
    assert "a_allowed" not in agent_mod.RecurrentAgent(spec, {}, n_envs=2).trajectory_mode
    # a set outside its domain's head is refused when the agent is built
    with pytest.raises(ValueError, match="allowed_actions"):
        agent_mod.RecurrentAgent(spec, {}, n_envs=1, slot_table=SlotTable.from_domains(
            [(Domain("x", True, 1, allowed_actions=[ND]), 1)], spec.act_dim))
    # the sets survive the trip through a pickle and are applied to the fresh engine
    a.set_slot_actions([3], [20, 21])
    a.make_pickleable()
    c = pickle.loads(pickle.dumps(a))
    c.reinit_cuda_kernels()
    assert c.engine is not eng and _sets(c.engine.mask)[3] == [20, 21] and _sets(c.engine.mask)[0] == list(PONG)


def test_set_slot_actions(agent_mod):
    spec = preset("xlstm_tiny")
    V, ND, n = spec.n_vocab, spec.n_discrete, 4
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n, discrete=True)
    eng = a.engine
    assert eng.calls == [] and a.slot_action_mask() is None
    a.set_slot_actions([1, 2], PONG)
    assert _sets(eng.mask) == [list(range(V)), list(PONG), list(PONG), list(range(V))]
    a.set_slot_actions(torch.tensor([2]), [4])
    assert _sets(eng.mask)[1:3] == [list(PONG), [4]]
    assert a.trajectory_mode["a_allowed"] == [{"slots": [(0, 1), (3, 4)], "allowed": "all"}, {"slots": [(1, 2)], "allowed": list(PONG)},
                                              {"slots": [(2, 3)], "allowed": [4]}]
    n_calls = len(eng.calls)
    for bad, exc in (([], ValueError), ([1, 1], ValueError), ([-1], ValueError), ([ND], ValueError), ([0.5], ValueError)):
        with pytest.raises(exc, match="set_slot_actions"):
            a.set_slot_actions([0], bad)
    with pytest.raises(IndexError):
        a.set_slot_actions([n], [0])
    assert len(eng.calls) == n_calls and _sets(a.slot_action_mask())[0] == list(range(V))
    a.set_slot_actions([1], None)                            # back to everything
    assert _sets(eng.mask)[1] == list(range(V)) and _sets(eng.mask)[2] == [4]
    a.set_slot_actions([2], None)                            # no set left: the mask is cleared
    assert eng.calls[-1] == ("set_action_mask", None) and a.slot_action_mask() is None and "a_allowed" not in a.trajectory_mode
    # None restores the DOMAIN's set under a table; a continuous slot takes token ids
    tab = SlotTable.from_domains([(Domain("pong", True, 1, allowed_actions=PONG), 2), (Domain("mw", False, 2), 2)], spec.act_dim)
    b = agent_mod.RecurrentAgent(spec, {}, n_envs=4, slot_table=tab)
    b.set_slot_actions([0], [0, 1])
    b.set_slot_actions([3], [ND, V - 1])
    assert _sets(b.engine.mask) == [[0, 1], list(PONG), list(range(V)), [ND, V - 1]]
    with pytest.raises(ValueError, match="set_slot_actions"):
        b.set_slot_actions([1], [ND])                        # a discrete slot selects among n_discrete logits
    b.set_slot_actions([0], None)
    assert _sets(b.engine.mask)[0] == list(PONG)


def test_set_active_refuses_to_exchange_slots_whose_sets_differ(agent_mod):
    spec, n = preset("xlstm_tiny"), 4
    a = agent_mod.RecurrentAgent(spec, {}, n_envs=n, discrete=True)
    assert a._slots_alike(0, 3) is None
    a.set_slot_actions([3], PONG)
    assert a._slots_alike(0, 3) == "allowed-action set" and a._slots_alike(0, 1) is None
    n_calls = len(a.engine.calls)
    with pytest.raises(ValueError, match="allowed-action set"):
        a.set_active([1, 2, 3])                              # would park env 0 by exchanging slots 0 and 3
    assert len(a.engine.calls) == n_calls and a.active == list(range(n))
    a.set_slot_actions([0], PONG)
    a.set_active([1, 2, 3])                                  # equal sets: the exchange goes through
    assert ("swap", [0], [3]) in a.engine.calls and a.engine.live == 3
