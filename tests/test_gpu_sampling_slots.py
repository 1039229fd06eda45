"""GPU: per-slot sampling settings (lram_set_sampling_slots) and the log-probability under the drawn distribution
(lram_score_last_sampled, lram_sample_rows), through the C ABI.

References: tests/sampling_ref.py / tests/sampling_slots_ref.py (float64 numpy, held on the CPU to the probabilities recorded
from the reference's sample_from_logits) for the row code; for the step the engine's own logits tap fed through
lram_sample_rows with lram_sample_uniforms and the per-row settings, as test_gpu_sampling.py does with lram_sample_tokens;
an engine armed globally (lram_set_sampling alone) for "a table that says the same is the same".

Bounds: drawn tokens equal the restatement's row by row; log-probabilities are held to it by the 2-ulp rule of
test_gpu_score.py (fp64 arithmetic, one fp32 rounding at the store), with the -inf / 0 / NaN classes exact."""
import numpy as np
import pytest
import torch

from lram_amd import init_state_dict, preset
from oracle.dt_ref import minmax_inv_tokenize
from tests import sampling_slots_ref as ssr
from tests.test_gpu_sampling import _inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEG_INF = float("-inf")
TEMPS = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)


def _dev(x, dtype=None):
    return torch.as_tensor(x, dtype=dtype).to(DEV)


def _assert_2ulp(got, ref64, what):
    """got (fp32) against ref64 rounded to fp32: equal (infinities, zeros), both NaN, or within 2 ulps of the result."""
    got, ref = got.detach().cpu(), ref64.detach().cpu().to(torch.float32)
    ulp = torch.nextafter(ref.abs(), torch.full_like(ref, float("inf"))) - ref.abs()
    ok = (got == ref) | (got.isnan() & ref.isnan()) | ((got - ref).abs() <= 2 * ulp)
    worst = ((got - ref).abs() / ulp)[~(got == ref) & ref.isfinite() & got.isfinite()]
    print(f"{what}: {got.numel()} entries, worst {float(worst.max()) if worst.numel() else 0.0:.2f} ulp")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} entries off; first: got {got[~ok][0]!r} want {ref[~ok][0]!r}"


def _assert_logp(got, ref64, what):
    """2 ulps, and the classes exactly: -inf where the reference is -inf, 0 where it is 0, NaN where it is NaN."""
    g, r = got.detach().cpu(), torch.as_tensor(ref64, dtype=torch.float64)
    for name, cls in (("-inf", lambda x: x == NEG_INF), ("0", lambda x: x == 0), ("NaN", lambda x: x.isnan())):
        assert torch.equal(cls(g), cls(r)), f"{what}: the {name} entries differ"
    _assert_2ulp(g, r, what)


def _table(B, discrete=False):
    """Slot b's setting is a function of b; every fifth slot is greedy."""
    b = np.arange(B)
    return {"temperature": np.array([TEMPS[i % 8] for i in b]), "top_k": np.array([(0, 5, 10, 1)[i % 4] for i in b], dtype=np.int32),
            "top_p": np.array([(0.5, 0.0, 0.25)[i % 3] for i in b]), "greedy": b % 5 == 4}


def _set(eng, cols):
    eng.set_sampling_slots(temperature=cols["temperature"], top_k=cols["top_k"], top_p=cols["top_p"], greedy=cols["greedy"])


def _check_step(eng, spec, a, tok, discrete, cols, seed, base, d, what):
    """tokens == lram_sample_rows(logits tap of this step, lram_sample_uniforms(seed, base, ., ., d), the slots' settings);
    actions de-tokenised; greedy slots hold the argmax of their tap row.  Returns the number of sampled tokens off the argmax."""
    from lram_amd.engine import sample_rows, sample_uniforms
    B, A, V = eng.batch, spec.act_dim, spec.n_vocab
    torch.cuda.synchronize()
    _, _, logits = eng.taps()
    u = sample_uniforms(seed, base, B, A, d, device=DEV)
    greedy = torch.as_tensor(cols["greedy"])
    lg = logits.view(B, A, V)
    if discrete:
        want, _ = sample_rows(logits[:, : spec.n_discrete], uniform=u[:, 0].contiguous(), temperature=cols["temperature"],
                              top_k=cols["top_k"], top_p=cols["top_p"], greedy=cols["greedy"])
        assert torch.equal(tok[:, 0], want), f"{what}: discrete tokens vs sample_rows(own logits, uniforms of draw {d})"
        assert torch.equal(a[:, 0], want.float()), f"{what}: discrete actions"
        assert bool(((want >= 0) & (want < spec.n_discrete)).all())
        am = lg[:, 0, : spec.n_discrete].argmax(-1).to(torch.int32)
        assert torch.equal(tok[greedy.to(DEV), 0], am[greedy.to(DEV)]), f"{what}: a greedy slot is off its argmax"
        return int((tok[:, 0] != am).sum())
    rep = {k: np.repeat(np.asarray(v), A) for k, v in cols.items()}
    want, _ = sample_rows(logits.view(B * A, V), uniform=u.view(-1), temperature=rep["temperature"], top_k=rep["top_k"],
                          top_p=rep["top_p"], greedy=rep["greedy"])
    assert torch.equal(tok, want.view(B, A)), f"{what}: tokens vs sample_rows(own logits, uniforms of draw {d})"
    assert torch.equal(a, minmax_inv_tokenize(tok.long(), spec.action_channels, spec.n_discrete)), f"{what}: actions"
    am = lg.argmax(-1).to(torch.int32)
    assert torch.equal(tok[greedy.to(DEV)], am[greedy.to(DEV)]), f"{what}: a greedy slot is off its argmax"
    return int((tok != am).sum())


def _ref_logp(logits, tok, cols, n):
    """rows_logp over [B, A] tokens with the slots' settings (numpy, float64) -> [B, A]."""
    B, A = tok.shape
    lg = logits.cpu().numpy().reshape(B, A, -1)[:, :, :n]
    t = tok.cpu().numpy()
    mode = 1 - np.asarray(cols["greedy"]).astype(np.uint8)
    out = np.zeros((B, A))
    for j in range(A):
        out[:, j] = ssr.rows_logp(lg[:, j], t[:, j], mode, cols["temperature"], cols["top_k"], cols["top_p"])
    return out


def _uniform_cols(B, temperature=1.0, top_k=0, top_p=0.0, greedy=False):
    return {"temperature": np.full(B, float(temperature)), "top_k": np.full(B, int(top_k), dtype=np.int32),
            "top_p": np.full(B, float(top_p)), "greedy": np.full(B, bool(greedy))}


# ---- 1. the row code on caller data -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [18, 274, 512])
def test_rows_draw_and_score_with_a_setting_per_row(hip_lib, n):
    from lram_amd.engine import sample_rows
    c = ssr.rows_case(n)
    s = (c["mode"], c["temperature"], c["top_k"], c["top_p"])
    kw = dict(temperature=c["temperature"], top_k=c["top_k"], top_p=c["top_p"], greedy=c["mode"] == 0)
    want = ssr.sample_rows(c["logits"], c["uniform"], *s)
    tokens = ssr.scored_tokens(c, want)
    ref = ssr.rows_logp(c["logits"], tokens, *s)
    assert np.isfinite(ref).mean() >= 0.10 and (ref == NEG_INF).mean() >= 0.10
    logits = _dev(c["logits"])
    drawn, logp = sample_rows(logits, uniform=_dev(c["uniform"]), tokens=_dev(tokens), **kw)
    assert drawn.dtype == torch.int32 and np.array_equal(drawn.cpu().numpy(), want), np.flatnonzero(drawn.cpu().numpy() != want)[:5]
    _assert_logp(logp, ref, f"rows of {n}")
    # either half alone gives the same; a drawn token never scores -inf; token -1 is the fill value
    only_drawn, none = sample_rows(logits, uniform=_dev(c["uniform"]), **kw)
    assert none is None and torch.equal(only_drawn, drawn)
    none, at_drawn = sample_rows(logits, tokens=drawn, **kw)
    assert none is None and bool(torch.isfinite(at_drawn).all())
    _assert_logp(at_drawn, ssr.rows_logp(c["logits"], want, *s), f"rows of {n} at the drawn tokens")
    _, fill = sample_rows(logits, tokens=torch.full_like(drawn, -1), **kw)
    assert bool((fill == 0).all())
    _, outside = sample_rows(logits, tokens=torch.full_like(drawn, n), **kw)
    assert bool((outside == NEG_INF).all())


# ---- 2. the step, one env slice and two --------------------------------------------------------------------------------------
@pytest.mark.parametrize("discrete", [False, True], ids=["continuous", "discrete"])
@pytest.mark.parametrize("slots", [12, 512])
def test_step_draws_every_slot_with_its_own_setting(hip_lib, slots, discrete):
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    eng = Engine(spec, init_state_dict(spec, seed=0), slots, device=DEV)
    seed, base = 20261018 + slots, 2 ** 32 - 8 if slots == 12 else 4096
    eng.set_sampling(temperature=1.0, top_k=0, top_p=0.0, seed=seed, slot_base=base)
    assert eng.sampling_slots is None
    cols = _table(slots)
    _set(eng, cols)
    back = eng.sampling_slots
    for k in cols:
        assert np.array_equal(back[k].numpy(), cols[k]), k
    g = torch.Generator(device=DEV).manual_seed(slots)
    off = 0
    for t in range(4):
        obs, rtg, rew, mask = _inputs(spec, slots, t, g)
        a, tok = eng.step(obs, rtg, rew, mask, discrete=discrete)
        off += _check_step(eng, spec, a, tok, discrete, cols, seed, base, t, f"{slots} slots step {t}")
    assert eng.sampling["draws"] == 4
    assert off > 0, "every sampled token was the argmax: nothing was drawn"
    eng.close()
    torch.cuda.empty_cache()


# ---- 3. a table that says what the engine-wide settings say --------------------------------------------------------------------
def test_table_slots_equal_engines_armed_globally(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_tiny")
    sd = init_state_dict(spec, seed=3)
    B, seed, base = 12, 77, 40
    S = [dict(temperature=0.75, top_k=10, top_p=0.5), dict(temperature=2.0, top_k=0, top_p=0.25)]
    engs = {name: Engine(spec, sd, B, device=DEV) for name in ("table", "s0", "s1", "plain", "same")}
    engs["table"].set_sampling(seed=seed, slot_base=base)
    alt = np.arange(B) % 2
    _set(engs["table"], {"temperature": np.array([S[i]["temperature"] for i in alt]), "top_k": np.array([S[i]["top_k"] for i in alt]),
                         "top_p": np.array([S[i]["top_p"] for i in alt]), "greedy": np.zeros(B, dtype=bool)})
    engs["s0"].set_sampling(seed=seed, slot_base=base, **S[0])
    engs["s1"].set_sampling(seed=seed, slot_base=base, **S[1])
    engs["plain"].set_sampling(seed=seed, slot_base=base, **S[0])
    engs["same"].set_sampling(seed=seed, slot_base=base, **S[0])
    engs["same"].set_sampling_slots(**S[0])
    g = torch.Generator(device=DEV).manual_seed(B)
    differ = 0
    for t in range(3):
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        out = {k: tuple(x.clone() for x in e.step(obs, rtg, rew, mask)) for k, e in engs.items()}
        torch.cuda.synchronize()
        for i in (0, 1):
            sel = torch.as_tensor(alt == i).to(DEV)
            assert torch.equal(out["table"][1][sel], out[f"s{i}"][1][sel]), f"step {t}: slots on setting {i}: tokens"
            assert torch.equal(out["table"][0][sel].view(torch.int32), out[f"s{i}"][0][sel].view(torch.int32)), f"step {t}: actions"
        differ += int((out["s0"][1] != out["s1"][1]).sum())
        for k in (0, 1):   # the table repeating the engine-wide settings: bit-identical to no table
            assert torch.equal(out["same"][k].view(torch.int32), out["plain"][k].view(torch.int32)), f"step {t}"
    assert differ > 0, "the two settings drew the same tokens everywhere: the comparison shows nothing"
    for e in engs.values():
        e.close()


# ---- 4. a mixed batch -----------------------------------------------------------------------------------------------------------
def test_mixed_batch_top_k_is_per_slot(hip_lib):
    from lram_amd.engine import Engine, LramError
    spec = preset("xlstm_tiny")
    B, A, V, ND = 12, spec.act_dim, spec.n_vocab, spec.n_discrete
    assert ND < 19 <= 40 <= V
    kinds = [[(0, A), (1, 1), (0, 2), (1, 1), (0, 1), (0, min(3, A))][b % 6] for b in range(B)]   # (discrete, act_dim)
    disc = np.array([k[0] for k in kinds], dtype=bool)
    eng = Engine(spec, init_state_dict(spec, seed=5), B, device=DEV)
    eng.set_slot_table(disc.tolist(), [k[1] for k in kinds], [False] * B)
    eng.set_sampling(top_k=ND, seed=9)
    cols = {"temperature": np.full(B, 1.0), "top_k": np.where(disc, 5, 40).astype(np.int32), "top_p": np.zeros(B),
            "greedy": np.zeros(B, dtype=bool)}
    _set(eng, cols)
    g = torch.Generator(device=DEV).manual_seed(B)
    for t in range(3):
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        a, tok = eng.step_slots(obs, None, rtg, rew, mask) if t % 2 == 0 else eng.step(obs, rtg, rew, mask, discrete="per_slot")
        torch.cuda.synchronize()
        lg = eng.taps()[2].view(B, A, V).cpu()
        lp = eng.last_logp(tok, over="sampled").cpu()
        a, tok = a.cpu(), tok.cpu()
        for b, (d, n_act) in enumerate(kinds):
            n, k = (ND, 5) if d else (V, 40)
            for j in range(A):
                if j >= n_act:
                    assert int(tok[b, j]) == -1 and float(a[b, j]) == 0.0 and float(lp[b, j]) == 0.0, (t, b, j)
                    continue
                row = lg[b, j, :n]
                kth = torch.topk(row, k).values[-1]
                assert 0 <= int(tok[b, j]) < n and float(row[int(tok[b, j])]) >= float(kth), (t, b, j, int(tok[b, j]))
                assert np.isfinite(float(lp[b, j]))
        _assert_logp(lp, _ref_logp_mixed(lg, tok, cols, kinds, ND, V), f"mixed step {t}")
    assert eng.sampling["draws"] == 3
    # a discrete slot with top_k = 19: accepted by the table (n_vocab bounds it), refused by the call that gives it 18 logits
    cols["top_k"][1] = ND + 1
    _set(eng, cols)
    hid = eng.taps()[1].clone()
    for call in (lambda: eng.step_slots(obs, None, rtg, rew, mask), lambda: eng.step(obs, rtg, rew, mask, discrete="per_slot")):
        with pytest.raises(LramError, match=r"top_k 19 of slot 1 "):
            call()
    with pytest.raises(LramError, match=r"top_k 40 of slot 0 "):      # the discrete head for every slot: the largest top_k is named
        eng.step(obs, rtg, rew, mask, discrete=True)
    torch.cuda.synchronize()
    assert eng.sampling["draws"] == 3 and torch.equal(eng.taps()[1], hid)        # refused before anything was launched
    eng.step(obs, rtg, rew, mask, discrete=False)                                 # 19 of 274 logits: fine
    cols["greedy"][1] = True                                                       # a greedy slot's top_k binds nothing
    _set(eng, cols)
    eng.step_slots(obs, None, rtg, rew, mask)
    assert eng.sampling["draws"] == 5
    eng.close()


def _ref_logp_mixed(lg, tok, cols, kinds, ND, V):
    B, A = tok.shape
    out = np.zeros((B, A))
    for b, (d, n_act) in enumerate(kinds):
        for j in range(n_act):
            out[b, j] = ssr.row_logp(lg[b, j, : ND if d else V].numpy(), int(tok[b, j]), 0 if cols["greedy"][b] else 1,
                                     cols["temperature"][b], cols["top_k"][b], cols["top_p"][b])
    return out


# ---- 5. the log-probability of what was drawn ----------------------------------------------------------------------------------
@pytest.mark.parametrize("discrete", [False, True], ids=["continuous", "discrete"])
def test_last_logp_over_sampled(hip_lib, discrete):
    from lram_amd.engine import Engine, LramError
    spec = preset("xlstm_tiny")
    B, A, V = 12, spec.act_dim, spec.n_vocab
    n = spec.n_discrete if discrete else V
    eng = Engine(spec, init_state_dict(spec, seed=8), B, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(B)
    zeros = torch.zeros(B, A, dtype=torch.int32, device=DEV)
    eng.set_sampling(top_p=0.5, seed=4)                     # sample_from_logits' own defaults
    with pytest.raises(LramError, match="no logits"):
        eng.last_logp(zeros, over="sampled")
    used = slice(0, 1) if discrete else slice(None)

    def step(t):
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        _, tok = eng.step(obs, rtg, rew, mask, discrete=discrete)
        torch.cuda.synchronize()
        return tok.clone(), eng.taps()[2].clone()

    tok, logits = step(0)
    lp = eng.last_logp(tok, over="sampled")
    assert bool(torch.isfinite(lp).all()) and bool((lp[:, used] < 0).any())
    ref = _ref_logp(logits, tok[:, used], _uniform_cols(B, 1.0, 0, 0.5), n)
    _assert_logp(lp[:, used], ref, "reference defaults")
    if discrete:
        assert bool((lp[:, 1:] == 0).all())
    # half of every row is outside the support of top_p = 0.5: the row's smallest logit scores -inf
    low = eng.taps()[2].view(B, A, V)[:, :, :n].argmin(-1).to(torch.int32)
    assert bool((eng.last_logp(low.contiguous(), over="sampled")[:, used] == NEG_INF).all())
    assert eng.sampling["draws"] == 1                       # scoring draws nothing
    with pytest.raises(ValueError):
        eng.last_logp(tok, over="sampled", temperature=0.75)
    # a table: greedy slots score exactly 0 at their token, the others by their own settings
    cols = _table(B)
    _set(eng, cols)
    tok, logits = step(1)
    lp = eng.last_logp(tok, over="sampled")
    gr = torch.as_tensor(cols["greedy"]).to(DEV)
    assert bool((lp[gr] == 0).all()) and bool(torch.isfinite(lp).all())
    _assert_logp(lp[:, used], _ref_logp(logits, tok[:, used], cols, n), "per-slot table")
    # no filter: the unfiltered softmax of lram_score_last
    eng.set_sampling(temperature=0.75, top_k=0, top_p=0.0, seed=4)
    tok, logits = step(2)
    rnd = torch.randint(0, n, (B, A), generator=g, device=DEV, dtype=torch.int32)
    for what, tk in (("drawn", tok), ("random", rnd)):
        _assert_2ulp(eng.last_logp(tk, over="sampled")[:, used],
                     eng.last_logp(tk, over="selectable", temperature=0.75)[:, used].double(), f"unfiltered, {what} tokens")
    assert eng.sampling["draws"] == 1
    eng.set_sampling(None)
    with pytest.raises(LramError, match="not armed"):
        eng.last_logp(tok, over="sampled")
    eng.close()


# ---- 6. a temperature ladder over the forks of one context -----------------------------------------------------------------------
def test_ladder_over_forks(hip_lib):
    from lram_amd.agent import RecurrentAgent
    from lram_amd.engine import sample_rows, sample_uniforms
    spec = preset("xlstm_tiny")
    B, A, V, L = 8, spec.act_dim, spec.n_vocab, 5
    agent = RecurrentAgent(spec, init_state_dict(spec, seed=2), n_envs=B, device=DEV, sample_seed=123, sample_slot_base=16)
    eng = agent.engine
    g = torch.Generator(device=DEV).manual_seed(B)
    ctx = torch.rand(B, L, spec.state_dim, generator=g, device=DEV) * 2 - 1        # a different context in every slot
    eng.prefill(ctx, torch.full((B, L), 4.5, device=DEV), torch.zeros(B, L, device=DEV),
                reset_mask=torch.ones(B, dtype=torch.uint8, device=DEV), want_action=False)
    agent.fork_slots([0] * 7, list(range(1, 8)))
    agent.set_slot_sampling(range(B), [{"temperature": t, "top_k": 0, "top_p": 0.5} for t in TEMPS])
    assert eng.sampling["draws"] == 0 and eng.sampling_slots["temperature"].tolist() == list(TEMPS)
    obs = (torch.rand(1, spec.state_dim, generator=g, device=DEV) * 2 - 1).expand(B, -1).contiguous()
    a, tok = eng.step(obs, torch.full((B,), 4.4, device=DEV), torch.zeros(B, device=DEV), None)
    torch.cuda.synchronize()
    logits = eng.taps()[2].view(B, A * V)
    assert torch.equal(logits.view(torch.int32), logits[:1].expand(B, -1).contiguous().view(torch.int32)), "the forks' logits differ"
    u = sample_uniforms(123, 16, B, A, 0, device=DEV)
    want, _ = sample_rows(logits.view(B * A, V), uniform=u.view(-1), temperature=np.repeat(TEMPS, A), top_p=0.5)
    assert torch.equal(tok, want.view(B, A))
    assert len({tuple(r) for r in tok.tolist()}) > 1, "every rung drew the same tokens"
    lp = agent.action_log_prob(over="sampled")
    assert bool(torch.isfinite(lp).all())
    _assert_logp(lp, _ref_logp(logits, tok, _uniform_cols(B, 1.0, 0, 0.5) | {"temperature": np.array(TEMPS)}, V), "ladder")
    assert len(agent.trajectory_mode["a_sample_slots"]) == B
    eng.close()


# ---- 7. lifecycle ---------------------------------------------------------------------------------------------------------------
def test_clearing_and_disarming(hip_lib):
    from lram_amd.engine import Engine, LramError
    spec = preset("xlstm_tiny")
    sd = init_state_dict(spec, seed=6)
    B = 12
    kw = dict(temperature=0.75, top_k=10, top_p=0.5)
    ea, eb = Engine(spec, sd, B, device=DEV), Engine(spec, sd, B, device=DEV)
    with pytest.raises(LramError, match="not armed"):
        _set(ea, _table(B))
    ea.set_sampling(seed=21, slot_base=3, **kw)
    eb.set_sampling(seed=21, slot_base=3, **kw)
    _set(ea, _table(B))
    g = torch.Generator(device=DEV).manual_seed(B)
    differ = 0
    for t in range(4):
        if t == 2:
            ea.set_sampling_slots(None)
            assert ea.sampling_slots is None
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        xa = tuple(x.clone() for x in ea.step(obs, rtg, rew, mask))
        xb = tuple(x.clone() for x in eb.step(obs, rtg, rew, mask))
        torch.cuda.synchronize()
        if t < 2:
            differ += int((xa[1] != xb[1]).sum())
        else:   # cleared: the engine-wide behaviour, bit for bit (the draw count ran on under the table)
            for k in (0, 1):
                assert torch.equal(xa[k].view(torch.int32), xb[k].view(torch.int32)), f"step {t} after clearing"
    assert differ > 0 and ea.sampling["draws"] == 4
    # refused tables name the slot and leave the one in effect
    _set(ea, _table(B))
    for key, bad, at in (("temperature", 0.0, 3), ("temperature", float("nan"), 0), ("top_p", 1.5, 11), ("top_k", -1, 7),
                         ("top_k", spec.n_vocab + 1, 5)):
        cols = _table(B)
        cols[key] = cols[key].copy()
        cols[key][at] = bad
        with pytest.raises(LramError, match=rf"lram_set_sampling_slots.*\(slot {at}\)"):
            _set(ea, cols)
        assert np.array_equal(ea.sampling_slots["top_k"].numpy(), _table(B)["top_k"])
    with pytest.raises(ValueError):
        ea.set_sampling_slots(temperature=[1.0] * (B - 1))
    # arming and disarming both clear the table
    ea.set_sampling(seed=1, **kw)
    assert ea.sampling_slots is None
    _set(ea, _table(B))
    ea.set_sampling(None)
    assert ea.sampling_slots is None and ea.sampling is None
    ea.set_sampling(seed=1, **kw)
    assert ea.sampling_slots is None
    # the settings stay with the slot index: reset, copy, save and load move none of them
    _set(ea, _table(B))
    ea.reset(torch.ones(B, dtype=torch.uint8, device=DEV))
    ea.copy_slots([0, 1], [5, 6])
    ea.load_slots([2], ea.save_slots([9]))
    assert np.array_equal(ea.sampling_slots["temperature"].numpy(), _table(B)["temperature"])
    ea.close(), eb.close()


def test_graph_replays_draw_afresh_under_a_table(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    B = 8
    eng = Engine(spec, init_state_dict(spec, seed=0), B, device=DEV)
    eng.set_graph_mode(True)
    eng.set_sampling(seed=31, slot_base=16)
    cols = _table(B)
    _set(eng, cols)
    g = torch.Generator(device=DEV).manual_seed(8)
    obs, rtg, rew, _ = _inputs(spec, B, 0, g)
    mask = torch.zeros(B, dtype=torch.uint8, device=DEV)
    toks = []
    for t in range(4):      # identical inputs and buffers: step 0 captures, the later ones replay
        a, tok = eng.step(obs, rtg, rew, mask)
        _check_step(eng, spec, a, tok, False, cols, 31, 16, t, f"graph step {t}")
        toks.append(tok.cpu().clone())
    assert eng.sampling["draws"] == 4
    assert any(not torch.equal(toks[0], x) for x in toks[1:])
    eng.close()


def test_mamba_repeated_forwards_share_one_draw_under_a_table(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("mamba_48m")
    B = 12
    eng = Engine(spec, init_state_dict(spec, seed=0), B, device=DEV)
    eng.set_compat_mode(4, True)
    eng.set_sampling(seed=77, slot_base=8)
    cols = _table(B)
    _set(eng, cols)
    g = torch.Generator(device=DEV).manual_seed(12)
    for t in range(4):
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        a, tok = eng.step(obs, rtg, rew, mask)
        _check_step(eng, spec, a, tok, False, cols, 77, 8, t, f"compat step {t}")   # every column
    assert eng.sampling["draws"] == 4     # once per env-step, not once per forward
    eng.close()
