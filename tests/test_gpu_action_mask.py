"""GPU: per-slot allowed-action sets (lram_set_action_mask, lram_sample_rows_masked, lram_score_tokens_masked) through the C ABI.

The rule under test (include/lram_hip.h): a column works on the sub-row of its slot's allowed entries below its selectable range,
as if the reference's function had been handed that sub-row, and maps the answer back.  References: tests/action_mask_ref.py
(float64 numpy, built on the restatements tests/test_sampling.py holds to the reference's sample_from_logits) for the row code;
for the step the engine's own logits tap fed through the masked row entry with lram_sample_uniforms, as test_gpu_sampling_slots.py
does without masks; an engine without a mask for "everything allowed is no mask".

Bounds, the existing ones: tokens equal the restatement row by row; actions are the de-tokenised tokens bit for bit;
log-probabilities obey _assert_logp of test_gpu_sampling_slots.py (2 ulps; the -inf / 0 / NaN classes exact)."""
import numpy as np
import pytest
import torch

from lram_amd import init_state_dict, preset
from lram_amd.domains import Domain, SlotTable
from oracle.dt_ref import minmax_inv_tokenize
from tests import action_mask_ref as amr
from tests import head_cases as hc
from tests import sampling_slots_ref as ssr
from tests.test_gpu_sampling import _inputs
from tests.test_gpu_sampling_slots import _assert_logp, _dev, _table

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEG_INF = float("-inf")
PONG = (0, 1, 3, 4, 11, 12)


def _slot_sets(B, V, ND):
    """Slot b's allowed set is a function of b (six kinds): bool [B, V], non-empty below ND and from ND on."""
    t = np.arange(V)
    allow = np.zeros((B, V), dtype=bool)
    for b in range(B):
        k = b % 6
        if k == 0:
            allow[b] = True
        elif k == 1:                                   # Pong's minimal set; every other bin
            allow[b, [a for a in PONG if a < ND]] = True
            allow[b, ND:] = t[ND:] % 2 == 1
        elif k == 2:                                   # Procgen's 15 actions; tokens 32 .. 63 and the top of the vocabulary
            allow[b, :min(15, ND)] = True
            allow[b] |= ((t >= 32) & (t < 64)) | (t >= max(ND, V - 74))
        elif k == 3:                                   # one action, one bin
            allow[b, min(5, ND - 1)] = True
            allow[b, V - 1] = True
        elif k == 4:                                   # everything but action 0; every third bin
            allow[b, 1:ND] = True
            allow[b, ND:] = t[ND:] % 3 == b % 3
        else:                                          # the last action; the first bins
            allow[b, ND - 1] = True
            allow[b, ND:min(V, ND + 32)] = True
    return allow


def _kinds(B, A, discrete):
    return [(1, 1) if discrete else (0, A)] * B


def _sel(cols, idx, rep=1):
    if cols is None:
        return dict(greedy=True)
    return {k: np.repeat(np.asarray(v)[idx], rep) for k, v in cols.items()}


def _expected(lg, u, kinds, allow, cols, ND):
    """The tokens of a step from its own logits tap lg [B, A, V] and uniforms u [B, A] through the masked row entry, one call for
    the discrete slots (rows of ND logits) and one for the others; -1 in the columns a slot does not use."""
    from lram_amd.engine import sample_rows
    B, A, V = lg.shape
    want = torch.full((B, A), -1, dtype=torch.int32, device=lg.device)
    d = [b for b, k in enumerate(kinds) if k[0]]
    c = [b for b, k in enumerate(kinds) if not k[0]]
    if d:
        w, _ = sample_rows(lg[d, 0, :ND].contiguous(), uniform=u[d, 0].contiguous(), mask=allow[d][:, :ND], **_sel(cols, d))
        want[d, 0] = w
    if c:
        w, _ = sample_rows(lg[c].reshape(len(c) * A, V).contiguous(), uniform=u[c].reshape(-1).contiguous(),
                           mask=np.repeat(allow[c], A, axis=0), **_sel(cols, c, A))
        w = w.view(len(c), A)
        for i, b in enumerate(c):
            want[b, :kinds[b][1]] = w[i, :kinds[b][1]]
    return want


def _check(eng, spec, a, tok, kinds, allow, cols, u, what, fill=True):
    """One masked step (or prefill): tokens against the masked row entry on the call's own logits, actions de-tokenised, every
    token allowed, fill columns (fill=False: a discrete call without a slot table leaves columns j >= 1 alone), and last_logp
    in every mode against the restatement."""
    A, V, ND = spec.act_dim, spec.n_vocab, spec.n_discrete
    torch.cuda.synchronize()
    n = tok.shape[0]
    lg = eng.taps()[2].view(n, A, V)
    want = _expected(lg, u, kinds, allow, cols, ND)
    in_use = want >= 0
    assert torch.equal(tok[in_use], want[in_use]), f"{what}: tokens vs the masked row entry on the step's own logits"
    tk, ac, lgc = tok.cpu(), a.cpu(), lg.cpu().numpy()
    used = torch.zeros(n, A, dtype=torch.bool)
    for b, (d, n_act) in enumerate(kinds):
        used[b, :n_act] = True
        for j in range(n_act):
            assert allow[b, int(tk[b, j])] and int(tk[b, j]) < (ND if d else V), f"{what}: slot {b} dim {j} took a disallowed token"
        if d:
            assert float(ac[b, 0]) == float(tk[b, 0]), what
        else:
            assert torch.equal(ac[b, :n_act], minmax_inv_tokenize(tk[b, :n_act].long(), spec.action_channels, ND)), what
    assert bool(used.to(in_use.device).eq(in_use).all())
    if fill:
        assert bool((tk[~used] == -1).all()) and bool((ac[~used] == 0).all()), f"{what}: fill columns"
    # log-probabilities at the returned tokens and at tokens shifted by one (mostly outside the sets)
    for shift in (0, 1):
        t_in = torch.where(used.to(tok.device), (tok + shift) % V, tok)
        t_np = t_in.cpu().numpy()
        modes = ("vocab", "selectable") + (("sampled",) if cols is not None else ())
        for over in modes:
            got = eng.last_logp(t_in.contiguous(), over=over)
            ref = np.zeros((n, A))
            for b, (d, n_act) in enumerate(kinds):
                nb = ND if d else V
                for j in range(n_act):
                    if over == "sampled":
                        ref[b, j] = amr.masked_row_logp(lgc[b, j, :nb], t_np[b, j], allow[b, :nb], 0 if cols["greedy"][b] else 1,
                                                        cols["temperature"][b], cols["top_k"][b], cols["top_p"][b])
                    else:
                        ref[b, j] = amr.masked_score_logp(lgc[b, j], t_np[b, j], allow[b], nb, over)
            _assert_logp(got, ref, f"{what}: last_logp over={over} shift={shift}")
            if shift == 0 and over != "vocab":
                assert bool(torch.isfinite(got).all()), f"{what}: a returned token scores -inf over={over}"


# ---- 1. the row code on caller data ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [18, 274, 512])
def test_rows_draw_and_score_on_the_sub_row(hip_lib, n):
    from lram_amd.engine import sample_rows
    c = amr.mask_rows_case(n)
    s = (c["mode"], c["temperature"], c["top_k"], c["top_p"])
    kw = dict(temperature=c["temperature"], top_k=c["top_k"], top_p=c["top_p"], greedy=c["mode"] == 0, mask=c["allow"])
    want = amr.masked_sample_rows(c["logits"], c["uniform"], c["allow"], *s)
    tokens = ssr.scored_tokens(c, want)
    ref = amr.masked_rows_logp(c["logits"], tokens, c["allow"], *s)
    logits = _dev(c["logits"])
    drawn, logp = sample_rows(logits, uniform=_dev(c["uniform"]), tokens=_dev(tokens), **kw)
    got = drawn.cpu().numpy()
    assert drawn.dtype == torch.int32 and np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    assert c["allow"][np.arange(len(got)), got].all()
    _assert_logp(logp, ref, f"masked rows of {n}")
    # greedy rows: the argmax of the sub-row
    R = len(want)
    g_tok, _ = sample_rows(logits, uniform=_dev(c["uniform"]), greedy=True, mask=c["allow"])
    assert np.array_equal(g_tok.cpu().numpy(), [amr.masked_argmax(c["logits"][r], c["allow"][r]) for r in range(R)])
    # either half alone gives the same; a drawn token never scores -inf; a token outside the set does; token -1 is the fill value
    only_drawn, none = sample_rows(logits, uniform=_dev(c["uniform"]), **kw)
    assert none is None and torch.equal(only_drawn, drawn)
    none, at_drawn = sample_rows(logits, tokens=drawn, **kw)
    assert none is None and bool(torch.isfinite(at_drawn).all())
    _assert_logp(at_drawn, amr.masked_rows_logp(c["logits"], want, c["allow"], *s), f"masked rows of {n} at the drawn tokens")
    _, fill = sample_rows(logits, tokens=torch.full_like(drawn, -1), **kw)
    assert bool((fill == 0).all())
    has_out = ~c["allow"].all(1)
    out_tok = np.where(has_out, (~c["allow"]).argmax(1), n).astype(np.int32)     # a disallowed token (past the row where all are allowed)
    _, outside = sample_rows(logits, tokens=_dev(out_tok), **kw)
    assert bool((outside == NEG_INF).all())
    # everything allowed: the unmasked entry, bit for bit
    full = dict(kw, mask=np.ones_like(c["allow"]))
    plain = {k: v for k, v in kw.items() if k != "mask"}
    d1, l1 = sample_rows(logits, uniform=_dev(c["uniform"]), tokens=_dev(tokens), **full)
    d0, l0 = sample_rows(logits, uniform=_dev(c["uniform"]), tokens=_dev(tokens), **plain)
    assert torch.equal(d1, d0) and torch.equal(l1.view(torch.int32), l0.view(torch.int32))


# ---- 2. the score row code on caller data ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["mt_disc", "over512"])
def test_score_tokens_on_the_sub_row(hip_lib, cid):
    from lram_amd.engine import score_tokens
    spec = hc.case_spec(cid, "xlstm")
    A, V, ND, R = spec.act_dim, spec.n_vocab, spec.n_discrete, 13
    g = torch.Generator().manual_seed(V)
    lg = torch.randn(R, A, V, generator=g) * 3.0
    allow = _slot_sets(R, V, ND)
    lg[3, :, V - 1] = float("nan")                              # slot kind 3 allows V - 1: a NaN inside a continuous sub-row
    lg[4, :, 0] = float("nan")                                  # kind 4 disallows 0: invisible to the discrete sub-row
    tok = torch.randint(0, V, (R, A), generator=g, dtype=torch.int32)
    lg_np = lg.numpy()
    for discrete in (False, True):
        nsel, cols = (ND, 1) if discrete else (V, A)
        greedy = torch.tensor([[amr.masked_argmax(lg_np[r, j], allow[r], nsel) for j in range(cols)] for r in range(R)])
        inside = torch.tensor([[int(np.flatnonzero(allow[r, :nsel])[(r + j) % allow[r, :nsel].sum()]) for j in range(A)] for r in range(R)],
                              dtype=torch.int32)
        for what, targets in (("random", tok), ("inside", inside)):
            t_np = targets.numpy()
            for over in ("vocab", "selectable"):
                for temp in (1.0, 0.37):
                    res = score_tokens(lg.to(DEV), spec, tokens=targets.to(DEV), discrete=discrete, over=over, temperature=temp,
                                       mask=allow)
                    torch.cuda.synchronize()
                    name = f"{cid} discrete={discrete} over={over} t={temp} {what}"
                    ref = np.array([[amr.masked_score_logp(lg_np[r, j], t_np[r, j], allow[r], nsel, over, temp) for j in range(cols)]
                                    for r in range(R)])
                    _assert_logp(res.logp[:, :cols], ref, name)
                    assert torch.equal(res.tokens[:, :cols].cpu().long(), greedy), name
                    if discrete:
                        assert torch.equal(res.actions[:, 0].cpu(), greedy[:, 0].float()), name
                        assert bool((res.tokens[:, 1:] == -1).all()) and bool((res.logp[:, 1:] == 0).all()), name
                    else:
                        assert torch.equal(res.actions.cpu(), minmax_inv_tokenize(greedy, spec.action_channels, ND)), name
                    if over == "vocab":                          # the normalisation ignores the mask: bit-identical
                        bare = score_tokens(lg.to(DEV), spec, tokens=targets.to(DEV), discrete=discrete, over=over, temperature=temp)
                        assert torch.equal(res.logp.view(torch.int32), bare.logp.view(torch.int32)), name
                        assert not torch.equal(res.tokens, bare.tokens), name
                    elif what == "inside":
                        ok = ~torch.as_tensor(ref).isnan()
                        assert bool((res.logp[:, :cols].cpu()[ok] > NEG_INF).all()), name
    # everything allowed equals no mask
    full = score_tokens(lg.to(DEV), spec, tokens=tok.to(DEV), over="selectable", mask=np.ones((R, V), dtype=bool))
    bare = score_tokens(lg.to(DEV), spec, tokens=tok.to(DEV), over="selectable")
    for k in ("actions", "tokens", "logp"):
        assert torch.equal(getattr(full, k).view(torch.int32), getattr(bare, k).view(torch.int32)), k


# ---- 3. the step --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("micro", [1, 2])
@pytest.mark.parametrize("name", ["xlstm_tiny", "mamba_tiny"])
def test_step_obeys_every_slots_own_set(hip_lib, name, micro):
    from lram_amd.engine import Engine, sample_uniforms
    spec = preset(name)
    B, A, V, ND = 12, spec.act_dim, spec.n_vocab, spec.n_discrete
    eng = Engine(spec, init_state_dict(spec, seed=4), B, device=DEV)
    eng.set_micro_batches(micro)
    allow = _slot_sets(B, V, ND)
    assert eng.action_mask is None
    eng.set_action_mask(allow)
    assert np.array_equal(eng.action_mask.numpy(), allow)
    g = torch.Generator(device=DEV).manual_seed(B)
    zeros = torch.zeros(B, A, dtype=torch.float64, device=DEV)
    seed, base = 99, 2 ** 32 - 5
    t = 0

    def step(discrete, kinds, cols, what, fn=None):
        nonlocal t
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        d = eng.sampling["draws"] if cols is not None else 0
        a, tok = fn(obs, rtg, rew, mask) if fn else eng.step(obs, rtg, rew, mask, discrete=discrete)
        u = sample_uniforms(seed, base, B, A, d, device=DEV) if cols is not None else zeros
        _check(eng, spec, a, tok, kinds, allow, cols, u, f"{name} micro {micro} {what}", fill=discrete is not True)
        t += 1
        return tok.clone()

    unmasked = []
    for discrete in (False, True):                       # greedy
        tok = step(discrete, _kinds(B, A, discrete), None, f"greedy discrete={discrete}")
        lg = eng.taps()[2].view(B, A, V)
        unmasked.append(int((tok[:, 0] != lg[:, 0, : ND if discrete else V].argmax(-1)).sum()))
    assert min(unmasked) > 0, "every masked greedy token was the plain argmax: the masks bound nothing"
    eng.set_sampling(temperature=0.75, top_k=10, top_p=0.25, seed=seed, slot_base=base)       # armed globally
    glob = {"temperature": np.full(B, 0.75), "top_k": np.full(B, 10, dtype=np.int32), "top_p": np.full(B, 0.25),
            "greedy": np.zeros(B, dtype=bool)}
    for discrete in (False, True):
        step(discrete, _kinds(B, A, discrete), glob, f"armed discrete={discrete}")
    cols = _table(B)                                     # a per-slot table
    eng.set_sampling_slots(temperature=cols["temperature"], top_k=cols["top_k"], top_p=cols["top_p"], greedy=cols["greedy"])
    for discrete in (False, True):
        step(discrete, _kinds(B, A, discrete), cols, f"table discrete={discrete}")
    # a mixed slot table from domains that state their sets; slots outside them keep the sets of set_action_mask's array
    atari = Domain("pong", True, 1, allowed_actions=PONG)
    procgen = Domain("procgen", True, 1, allowed_actions=range(15))
    mw = Domain("metaworld", False, 3, allowed_actions=range(ND + 40, V, 3))
    dmc = Domain("dmc", False, A)
    tab = SlotTable.from_domains([(atari, 3), (mw, 4), (procgen, 2), (dmc, 3)], A)
    eng.set_action_mask(None)
    eng.set_slot_table(*tab.engine_arrays())
    allow = tab.action_mask(V, ND).numpy()
    eng.set_action_mask(allow)
    kinds = [(int(tab.discrete[b]), int(tab.act_dim[b])) for b in range(B)]
    step("per_slot", kinds, cols, "mixed table, step")
    step(None, kinds, cols, "mixed table, step_slots", fn=lambda o, r, w, m: eng.step_slots(o, None, r, w, m))
    eng.set_sampling(None)
    step("per_slot", kinds, None, "mixed table, greedy")
    eng.close()


# ---- 4. everything allowed equals no mask --------------------------------------------------------------------------------------
def test_everything_allowed_is_no_mask_and_clearing_restores_it(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_tiny")
    B, V, ND = 12, spec.n_vocab, spec.n_discrete
    sd = init_state_dict(spec, seed=6)
    ea, eb = Engine(spec, sd, B, device=DEV), Engine(spec, sd, B, device=DEV)
    for e in (ea, eb):
        e.set_sampling(temperature=1.5, top_k=10, top_p=0.25, seed=5, slot_base=7)
    ea.set_action_mask(np.ones((B, V), dtype=bool))
    g = torch.Generator(device=DEV).manual_seed(B)

    def both(t, discrete=False):
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        out = []
        for e in (ea, eb):
            a, tok = e.step(obs, rtg, rew, mask, discrete=discrete)
            lps = [e.last_logp(tok, over=o) for o in ("vocab", "selectable", "sampled")]
            out.append([a.clone(), tok.clone()] + lps)
        torch.cuda.synchronize()
        return out

    for t in range(5):
        xa, xb = both(t, discrete=t == 3)
        for k, (x, y) in enumerate(zip(xa, xb)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"step {t}: output {k} differs under an all-true mask"
    ea.set_action_mask(_slot_sets(B, V, ND))
    xa, xb = both(5)
    assert not torch.equal(xa[1], xb[1]), "the sets bound nothing"
    ea.set_action_mask(None)
    assert ea.action_mask is None
    for t in (6, 7):
        xa, xb = both(t)
        for k, (x, y) in enumerate(zip(xa, xb)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"step {t}: output {k} differs after clearing"
    ea.set_action_mask(_slot_sets(B, V, ND))
    ea.alloc(B)
    assert ea.action_mask is None, "alloc() keeps the mask"
    ea.close(), eb.close()


# ---- 5. stored contexts -------------------------------------------------------------------------------------------------------
def test_prefill_and_score_obey_the_sets(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_tiny")
    B, A, V, ND, L = 12, spec.act_dim, spec.n_vocab, spec.n_discrete, 9
    eng = Engine(spec, init_state_dict(spec, seed=9), B, device=DEV)
    allow = _slot_sets(B, V, ND)
    eng.set_action_mask(allow)
    g = torch.Generator(device=DEV).manual_seed(L)
    obs = torch.rand(B, L, spec.state_dim, generator=g, device=DEV) * 2 - 1
    rtg = torch.full((B, L), 4.5, device=DEV)
    rew = torch.zeros(B, L, device=DEV)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    a, tok = eng.prefill(obs, rtg, rew, reset_mask=ones)
    _check(eng, spec, a, tok, _kinds(B, A, False), allow, None, torch.zeros(B, A, dtype=torch.float64, device=DEV), "prefill")
    targets = torch.randint(0, V, (B, L, A), generator=g, device=DEV, dtype=torch.int32)

    def check(res, lengths, what):
        lg, tk, lp = res.logits.cpu().numpy(), res.tokens.cpu(), res.logp.cpu()
        tg = targets.cpu().numpy()
        ref = np.zeros((B, L, A))
        for b in range(B):
            for l in range(L):
                if l >= lengths[b]:
                    assert bool((tk[b, l] == -1).all()) and bool((lp[b, l] == 0).all()), f"{what}: fill row [{b}, {l}]"
                    continue
                for j in range(A):
                    assert int(tk[b, l, j]) == amr.masked_argmax(lg[b, l, j], allow[b]), f"{what}: greedy token [{b}, {l}, {j}]"
                    ref[b, l, j] = amr.masked_score_logp(lg[b, l, j], tg[b, l, j], allow[b], V, "selectable")
        _assert_logp(lp, ref, what)
        assert torch.equal(res.actions.cpu()[tk >= 0], minmax_inv_tokenize(tk.long(), spec.action_channels, ND)[tk >= 0]), what

    kw = dict(tokens=targets, over="selectable", logits=True)
    dense = eng.score(obs, rtg, rew, reset_mask=ones, **kw)
    check(dense, [L] * B, "score dense")
    bare = Engine(spec, init_state_dict(spec, seed=9), B, device=DEV).score(obs, rtg, rew, reset_mask=ones, **kw)
    assert torch.equal(dense.logits.view(torch.int32), bare.logits.view(torch.int32)), "raw logits are altered by the mask"
    lengths = [9, 9, 5, 1, 0] + [3] * (B - 5)
    check(eng.score(obs, rtg, rew, lengths=lengths, **kw), lengths, "score ragged")
    check(eng.score(obs, rtg, rew, lengths=lengths, append=True, **kw), lengths, "score append")
    eng.close()


# ---- 6. live prefix and swaps ---------------------------------------------------------------------------------------------------
def test_the_sets_stay_with_the_slot_index(hip_lib):
    from lram_amd.engine import Engine, sample_uniforms
    spec = preset("xlstm_tiny")
    B, A, V, ND, n_live = 12, spec.act_dim, spec.n_vocab, spec.n_discrete, 5
    eng = Engine(spec, init_state_dict(spec, seed=2), B, device=DEV)
    allow = _slot_sets(B, V, ND)
    eng.set_action_mask(allow)
    eng.set_sampling(temperature=2.0, seed=3, slot_base=11)
    cols = {"temperature": np.full(B, 2.0), "top_k": np.zeros(B, dtype=np.int32), "top_p": np.zeros(B), "greedy": np.zeros(B, dtype=bool)}
    g = torch.Generator(device=DEV).manual_seed(B)
    obs, rtg, rew, mask = _inputs(spec, B, 0, g)
    a, tok = eng.step(obs, rtg, rew, mask)
    _check(eng, spec, a, tok, _kinds(B, A, False), allow, cols, sample_uniforms(3, 11, B, A, 0, device=DEV), "all live")
    eng.set_live(n_live)
    eng.swap_slots([1, 3], [7, 10])                           # across the boundary: slot 1 now holds slot 7's state, set 1 stays
    for t in (1, 2):
        obs, rtg, rew, mask = (x[:n_live].contiguous() for x in _inputs(spec, B, t, g))
        a, tok = eng.step(obs, rtg, rew, mask)
        u = sample_uniforms(3, 11, B, A, t, device=DEV)[:n_live].contiguous()
        live_cols = {k: v[:n_live] for k, v in cols.items()}
        _check(eng, spec, a, tok, _kinds(n_live, A, False), allow[:n_live], live_cols, u, f"live prefix step {t}")
    assert np.array_equal(eng.action_mask.numpy(), allow)
    eng.close()


# ---- 7. Mamba repeated forwards -------------------------------------------------------------------------------------------------
def test_mamba_repeated_forwards_obey_the_sets_in_every_column(hip_lib):
    from lram_amd.engine import Engine, sample_uniforms
    spec = preset("mamba_tiny")
    B, A, V, ND = 12, spec.act_dim, spec.n_vocab, spec.n_discrete
    eng = Engine(spec, init_state_dict(spec, seed=1), B, device=DEV)
    eng.set_compat_mode(mamba_repeat=A)
    allow = _slot_sets(B, V, ND)
    eng.set_action_mask(allow)
    g = torch.Generator(device=DEV).manual_seed(7)
    for t in range(2):                                          # greedy: every pass's column is the argmax of its sub-row
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        a, tok = eng.step(obs, rtg, rew, mask)
        torch.cuda.synchronize()
        tk = tok.cpu().numpy()
        assert allow[np.arange(B)[:, None], tk].all(), f"greedy step {t}: a column left its slot's set"
        lg = eng.taps()[2].view(B, A, V).cpu().numpy()         # (the last pass's logits: its own column and the ones behind it)
        assert all(int(tk[b, A - 1]) == amr.masked_argmax(lg[b, A - 1], allow[b]) for b in range(B))
        assert torch.equal(a, minmax_inv_tokenize(tok.long(), spec.action_channels, ND))
    eng.set_sampling(temperature=1.5, seed=13)
    for t in range(2, 4):
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        a, tok = eng.step(obs, rtg, rew, mask)
        torch.cuda.synchronize()
        tk = tok.cpu().numpy()
        assert allow[np.arange(B)[:, None], tk].all(), f"sampled step {t}: a column left its slot's set"
        u = sample_uniforms(13, 0, B, A, t - 2, device=DEV)
        want = _expected(eng.taps()[2].view(B, A, V), u, _kinds(B, A, False), allow,
                         {"temperature": np.full(B, 1.5), "top_k": np.zeros(B, dtype=np.int32), "top_p": np.zeros(B),
                          "greedy": np.zeros(B, dtype=bool)}, ND)
        assert torch.equal(tok[:, A - 1], want[:, A - 1]), f"sampled step {t}: the last pass's column"
    assert eng.sampling["draws"] == 2
    eng.close()


# ---- 8. graph mode --------------------------------------------------------------------------------------------------------------
def test_setting_a_mask_drops_the_graph_and_replays_obey_it(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_tiny")
    B, A, V, ND = 12, spec.act_dim, spec.n_vocab, spec.n_discrete
    eng = Engine(spec, init_state_dict(spec, seed=3), B, device=DEV)
    eng.set_graph_mode(True)
    g = torch.Generator(device=DEV).manual_seed(5)
    obs, rtg, rew, _ = _inputs(spec, B, 0, g)
    mask = torch.zeros(B, dtype=torch.uint8, device=DEV)
    zeros = torch.zeros(B, A, dtype=torch.float64, device=DEV)
    allow = _slot_sets(B, V, ND)
    plain = []
    for t in range(3):                                          # step 0 captures the unmasked step, the others replay it
        _, tok = eng.step(obs, rtg, rew, mask)
        plain.append(tok.clone())
    eng.set_action_mask(allow)
    differ = 0
    for t in range(3):                                          # a new capture with the masked head, then its replays
        a, tok = eng.step(obs, rtg, rew, mask)
        _check(eng, spec, a, tok, _kinds(B, A, False), allow, None, zeros, f"graph step {t} under the mask")
        differ += int((tok != eng.taps()[2].view(B, A, V).argmax(-1)).sum())
    assert differ > 0
    eng.set_action_mask(None)
    a, tok = eng.step(obs, rtg, rew, mask)
    torch.cuda.synchronize()
    assert torch.equal(tok, eng.taps()[2].view(B, A, V).argmax(-1).to(torch.int32)), "cleared, the graph still holds the masked head"
    eng.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_as_it_was(hip_lib):
    import ctypes
    from lram_amd.engine import Engine, LramError, pack_action_mask
    spec = preset("xlstm_tiny")
    B, A, V, ND = 12, spec.act_dim, spec.n_vocab, spec.n_discrete
    eng = Engine(spec, init_state_dict(spec, seed=3), B, device=DEV)
    allow = _slot_sets(B, V, ND)
    eng.set_action_mask(allow)
    g = torch.Generator(device=DEV).manual_seed(5)
    obs, rtg, rew, mask = _inputs(spec, B, 0, g)
    eng.step(obs, rtg, rew, mask)
    torch.cuda.synchronize()
    hid = eng.taps()[1].clone()
    # an empty sub-row: the host check (ValueError) and, past it, the library
    bad = allow.copy()
    bad[4] = False
    with pytest.raises(ValueError, match="slot 4 allows nothing"):
        eng.set_action_mask(bad)
    words = pack_action_mask(bad)
    assert eng.lib.lram_set_action_mask(eng._h, ctypes.c_void_p(words.data_ptr()), words.shape[1]) != 0
    assert b"slot 4 allows nothing" in eng.lib.lram_last_error()
    # wrong `words`
    good = pack_action_mask(allow)
    for w in (good.shape[1] - 1, good.shape[1] + 1, 0):
        assert eng.lib.lram_set_action_mask(eng._h, ctypes.c_void_p(good.data_ptr()), w) != 0
        assert b"words must be" in eng.lib.lram_last_error()
    assert np.array_equal(eng.action_mask.numpy(), allow)
    # a slot that allows nothing below n_discrete: accepted (no table: the range is the vocabulary), discrete calls refused
    cont = allow.copy()
    cont[7, :ND] = False
    eng.set_action_mask(cont)
    obs2, rtg2, rew2 = (x[:, None].expand(-1, 2, *x.shape[1:]).contiguous() for x in (obs, rtg, rew))
    tgt = torch.zeros(B, 2, A, dtype=torch.int32, device=DEV)
    for call in (lambda: eng.step(obs, rtg, rew, mask, discrete=True),
                 lambda: eng.prefill(obs[:, None].contiguous(), rtg[:, None].contiguous(), rew[:, None].contiguous(), discrete=True),
                 lambda: eng.score(obs2, rtg2, rew2, tokens=tgt, discrete=True),                       # the score entries: dense,
                 lambda: eng.score(obs2, rtg2, rew2, tokens=tgt, discrete=True, over="selectable", lengths=[2] * (B - 1) + [1]),
                 lambda: eng.score(obs2, rtg2, rew2, tokens=tgt, discrete=True, lengths=[1] * B, append=True)):   # ragged, append
        with pytest.raises(LramError, match="slot 7 nothing below n_discrete"):
            call()
    torch.cuda.synchronize()
    assert torch.equal(eng.taps()[1], hid), "a refused call launched something"
    # ... and so is a slot table that makes slot 7 discrete; one that keeps it continuous is taken
    disc = [b in (1, 7) for b in range(B)]
    with pytest.raises(LramError, match="allows slot 7 nothing"):
        eng.set_slot_table(disc, [1 if d else A for d in disc], [False] * B)
    assert eng.slot_table() is None and np.array_equal(eng.action_mask.numpy(), cont)
    disc = [b == 1 for b in range(B)]
    eng.set_slot_table(disc, [1 if d else A for d in disc], [False] * B)
    with pytest.raises(ValueError, match="slot 1 allows nothing"):      # with the table, slot 1's range is [0, n_discrete)
        cont2 = cont.copy()
        cont2[1, :ND] = False
        eng.set_action_mask(cont2)
    assert np.array_equal(eng.action_mask.numpy(), cont)
    a, tok = eng.step(obs, rtg, rew, mask, discrete="per_slot")
    torch.cuda.synchronize()
    assert cont[1, int(tok[1, 0])] and int(tok[1, 0]) < ND
    eng.close()


# ---- 10. head geometries --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["over512", "two", "disc300"])
def test_head_geometries(hip_lib, cid):
    from lram_amd.engine import Engine
    spec = hc.case_spec(cid, "xlstm")
    B, A, V, ND = 7, spec.act_dim, spec.n_vocab, spec.n_discrete
    eng = Engine(spec, init_state_dict(spec, seed=1), B, device=DEV)
    discrete = cid == "disc300"
    if cid == "two":
        allow = np.zeros((B, V), dtype=bool)
        allow[np.arange(B), np.arange(B) % 2] = True            # one token allowed
    elif cid == "disc300":
        allow = np.zeros((B, V), dtype=bool)
        for b in range(B):
            allow[b, (np.arange(7) * 43 + b * 5) % ND] = True   # a set of 7 among 300 actions
    else:
        allow = _slot_sets(B, V, ND)                            # V = 518: the unstaged argmax walk, 17 words per slot
    eng.set_action_mask(allow)
    g = torch.Generator(device=DEV).manual_seed(3)
    for t in range(2):
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        a, tok = eng.step(obs, rtg, rew, mask, discrete=discrete)
        torch.cuda.synchronize()
        lg = eng.taps()[2].view(B, A, V).cpu().numpy()
        tk = tok.cpu()
        for b in range(B):
            for j in range(1 if discrete else A):
                assert int(tk[b, j]) == amr.masked_argmax(lg[b, j], allow[b], ND if discrete else V), (cid, t, b, j)
        if discrete:
            assert torch.equal(a[:, 0], tok[:, 0].float())
        else:
            assert torch.equal(a, minmax_inv_tokenize(tok.long(), spec.action_channels, ND))
        for over in ("vocab", "selectable"):
            got = eng.last_logp(tok, over=over)
            ref = np.zeros((B, A))
            for b in range(B):
                for j in range(1 if discrete else A):
                    ref[b, j] = amr.masked_score_logp(lg[b, j], int(tk[b, j]), allow[b], ND if discrete else V, over)
            _assert_logp(got, ref, f"{cid} step {t} over={over}")
    eng.close()
