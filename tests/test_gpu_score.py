"""GPU: scoring stored trajectories -- the head at every timestep (lram_score), the log-probability of the tokens just taken
(lram_score_last) and the row code on caller logits (lram_score_tokens), through the C ABI.

Bars (none tuned to the code's output):
  * logp against float64 log_softmax of THE SAME logits, rounded to fp32: within 2 fp32 ulps of the result -- the kernel's
    maximum, sum and log are fp64 and the only fp32 rounding is the store;
  * greedy tokens equal torch.argmax (first index on ties); masked entries and unused columns hold exactly logp +0.0,
    token -1, action +0.0;
  * two fp32 evaluations of the logits (engine vs engine, engine vs CPU oracle): 2e-4 by helpers.rel_err, the project's bar;
    actions by its tie rule (exact / 1e-4 unless the reference's own top-2 gap is below 2e-4), and the committed seeds have no
    such tie, which is asserted;
  * logp against log_softmax of the ORACLE's logits: log-softmax is 2-Lipschitz in the maximum norm, so twice the allowed
    logit difference of that timestep;
  * everything that compares two engine runs (state after score vs prefill, blocked vs unblocked scratch, masked vs
    unmasked) is bit for bit.
Widths of the row test: lram_create sets no upper bound on n_vocab, so "the largest it accepts" does not exist; the kernel has
two forms -- rows of up to 512 logits are staged, wider ones are walked in global memory -- and 512, 513 and 4099 stand for
the largest staged row, the first streamed one and a streamed row that is no multiple of the wave."""
import dataclasses

import pytest
import torch

from lram_amd import init_state_dict, preset
from oracle import dt_ref
from tests.helpers import Fp64Oracle, assert_actions_match, assert_close_or_as_close_as_fp32_oracle, make_inputs, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEG_INF = float("-inf")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_2ulp(got, ref64, what):
    """got (fp32) against ref64 rounded to fp32: equal (infinities, zeros), both NaN, or within 2 ulps of the result."""
    got, ref = got.detach().cpu(), ref64.detach().cpu().to(torch.float32)
    ulp = torch.nextafter(ref.abs(), torch.full_like(ref, float("inf"))) - ref.abs()
    ok = (got == ref) | (got.isnan() & ref.isnan()) | ((got - ref).abs() <= 2 * ulp)
    worst = ((got - ref).abs() / ulp)[~(got == ref) & ref.isfinite() & got.isfinite()]
    print(f"{what}: {got.numel()} entries, worst {float(worst.max()) if worst.numel() else 0.0:.2f} ulp")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} entries off; first: got {got[~ok][0]!r} want {ref[~ok][0]!r}"


def _ref_logp(logits, tokens, n, temperature):
    """float64 log_softmax(temperature * logits[..., :n]) gathered at `tokens`; -inf where the token is outside 0 .. n - 1."""
    z = torch.log_softmax(temperature * logits[..., :n].double().cpu(), dim=-1)
    tok = tokens.cpu().long()
    inside = (tok >= 0) & (tok < n)
    out = z.gather(-1, tok.clamp(0, n - 1).unsqueeze(-1)).squeeze(-1)
    return torch.where(inside, out, torch.full_like(out, NEG_INF))


def _stack(seq):
    return tuple(torch.stack([x[i] for x in seq], 1).contiguous().to(DEV) for i in range(3))


def _state(eng, spec):
    out = []
    for blk in range(spec.n_blocks):
        kinds = (0, 3) if (spec.backbone == "mamba" or blk in spec.slstm_at) else (0, 1, 2, 3)
        out += [eng.export_state_tensor(blk, w) for w in kinds]
    torch.cuda.synchronize()
    return out


def _same_state(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: state tensor {i} differs"


def _engine(spec, sd, B):
    from lram_amd.engine import Engine
    return Engine(spec, sd, B, device=DEV)


# ---- 1. the row code alone ---------------------------------------------------------------------------------------------------
def _rows(V, A, R, seed):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(R, A, V, generator=g) * 3.0
    lg[0] = 0.25                                   # a constant row: every token ties
    lg[1] = torch.randn(A, V, generator=g)
    lg[1, :, V // 2] += 1e4                        # one logit 1e4 above the rest
    tok = torch.randint(0, V, (R, A), generator=g, dtype=torch.int32)
    tok[1, 0] = V // 2
    if V >= 3:
        lg[2, :, ::2] = NEG_INF                    # -inf entries ...
        tok[2, 0] = 0                              # ... one of them at the target
        if A > 1:
            tok[2, 1] = 1
        lg[3, :, V - 1] = float("nan")             # a NaN row
        tok[3] = tok[3].clamp(max=V - 2)
    return lg, tok


@pytest.mark.parametrize("V", [1, 18, 63, 64, 65, 82, 274, 512, 513, 4099])
def test_row_code_against_float64_log_softmax(hip_lib, V):
    from lram_amd.engine import score_tokens
    R = 13                                         # not a multiple of the four waves of a workgroup
    n_discrete = min(18, V)
    channels = max(1, V - n_discrete)
    for A in (1, 8):
        lg, tok = _rows(V, A, R, seed=1000 + V + A)
        tok_out = tok.clone()                      # targets out of range: below, at the end of the vocabulary, past it
        tok_out[5, 0], tok_out[6, 0], tok_out[7, 0] = -1, V, V + 7
        tok_out[8, 0] = n_discrete                 # outside the selectable range of a discrete row (inside the vocabulary if V > 18)
        lg_d, tok_d = lg.to(DEV), tok_out.to(DEV)
        for discrete in (False, True):
            nsel = n_discrete if discrete else V
            cols = 1 if discrete else A
            greedy = torch.argmax(lg[:, :cols, :nsel], dim=-1)
            for over in ("vocab", "selectable"):
                n = nsel if over == "selectable" else V
                for t in (1.0, 0.37):
                    res = score_tokens(lg_d, (n_discrete, channels), tokens=tok_d, discrete=discrete, over=over, temperature=t)
                    torch.cuda.synchronize()
                    what = f"V={V} A={A} discrete={discrete} over={over} t={t}"
                    want = _ref_logp(lg[:, :cols], tok_out[:, :cols], n, t)
                    _assert_2ulp(res.logp[:, :cols], want, what)
                    assert bool((res.logp[5:8, 0] == NEG_INF).all()), what
                    if V >= 3:
                        if n == V:                                                # the NaN (last logit) is inside the range
                            assert bool(res.logp[3, 0].isnan()), what
                        assert float(res.logp[2, 0]) == NEG_INF, what             # -inf at the target
                    assert torch.equal(res.tokens[:, :cols].cpu().long(), greedy), what
                    if discrete:
                        assert torch.equal(res.actions[:, 0].cpu(), greedy[:, 0].float()), what
                        # columns a discrete call does not use: the fill values, exactly
                        assert bool((_bits(res.logp[:, 1:]) == 0).all()) and bool((res.tokens[:, 1:] == -1).all()), what
                        assert bool((_bits(res.actions[:, 1:]) == 0).all()), what
                    else:
                        ref_a = dt_ref.minmax_inv_tokenize(greedy, channels, n_discrete)
                        # two fp32 roundings (product, then sum) as MinMaxTokenizer.inv_tokenize, whatever the channel count
                        assert torch.equal(res.actions.cpu(), ref_a), what
        # a `valid` mask: masked rows hold the fill values exactly, the others are untouched by it
        valid = (torch.arange(R) % 3 != 0)
        full = score_tokens(lg_d, (n_discrete, channels), tokens=tok_d)
        part = score_tokens(lg_d, (n_discrete, channels), tokens=tok_d, valid=valid.to(DEV))
        torch.cuda.synchronize()
        for name in ("actions", "tokens", "logp"):
            x, y = getattr(full, name).cpu(), getattr(part, name).cpu()
            assert torch.equal(_bits(x[valid]), _bits(y[valid])), (V, A, name)
            fill = torch.full_like(y[~valid], -1) if name == "tokens" else torch.zeros_like(y[~valid])
            assert torch.equal(_bits(y[~valid]), _bits(fill)), (V, A, name)


@pytest.mark.parametrize("channels", [64, 256])
def test_float_targets_tokenise_as_the_reference_tokenizer(hip_lib, channels):
    """Every bin edge k * bin_width - 1 and one fp32 ulp to either side, -1, 1, beyond both, +-0: the token is
    oracle.dt_ref.minmax_tokenize's (checked through logp: the rows hold pairwise distinct logits, so equal logp means the
    same token, and the same kernel on the same logits with that token as an int32 target gives the same bits); NaN and
    +-inf give -inf."""
    from lram_amd.engine import score_tokens
    n_discrete, A = 18, 8
    V = n_discrete + channels
    bw = 2.0 / channels
    edges = torch.arange(channels + 1, dtype=torch.float32) * bw - 1.0
    up = torch.nextafter(edges, torch.full_like(edges, 2.0))
    down = torch.nextafter(edges, torch.full_like(edges, -2.0))
    extra = torch.tensor([-1.0, 1.0, 1.5, 3e9, -1.5, -3e9, 0.0, -0.0, 0.999999, -0.999999])
    x = torch.cat([edges, up, down, extra])
    n_fin = x.numel()
    x = torch.cat([x, torch.tensor([float("nan"), float("inf"), NEG_INF])])
    pad = (-x.numel()) % A
    x = torch.cat([x, torch.zeros(pad)]).reshape(-1, A)
    R = x.shape[0]
    g = torch.Generator().manual_seed(channels)
    lg = torch.randn(R, A, V, generator=g) * 2.0
    assert all(lg[r, j].unique().numel() == V for r in range(R) for j in range(A))
    want_tok = dt_ref.minmax_tokenize(torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), channels, n_discrete).to(torch.int32)
    assert int(want_tok.min()) >= n_discrete and int(want_tok.max()) <= V - 1
    by_float = score_tokens(lg.to(DEV), (n_discrete, channels), actions=x.to(DEV), want=("logp",))
    by_token = score_tokens(lg.to(DEV), (n_discrete, channels), tokens=want_tok.to(DEV), want=("logp",))
    torch.cuda.synchronize()
    got, ref = by_float.logp.cpu().reshape(-1), by_token.logp.cpu().reshape(-1)
    finite = torch.ones(R * A, dtype=torch.bool)
    finite[n_fin:n_fin + 3] = False
    bad = (_bits(got) != _bits(ref)) & finite
    assert not bool(bad.any()), f"channels {channels}: {int(bad.sum())} targets tokenised differently, first x = {x.reshape(-1)[bad][0]!r}"
    assert bool((got[~finite] == NEG_INF).all())
    _assert_2ulp(ref.reshape(R, A), _ref_logp(lg, want_tok, V, 1.0), f"channels {channels}")
    # discrete rows take (int)action
    xd = torch.tensor([[0.0], [3.0], [17.0], [17.9], [18.0], [-1.0], [float("nan")]]).repeat(1, A)
    lgd = lg[: xd.shape[0]]
    res = score_tokens(lgd.to(DEV), (n_discrete, channels), actions=xd.to(DEV), discrete=True, over="selectable", want=("logp",))
    torch.cuda.synchronize()
    tok = torch.tensor([0, 3, 17, 17, 18, -1, -1])
    _assert_2ulp(res.logp[:, 0], _ref_logp(lgd[:, 0], tok, n_discrete, 1.0), "discrete float targets")


# ---- 2. score against sequential steps: the token-sequential path ------------------------------------------------------------
def _no_ties(logits, spec, discrete):
    """The reference run's own top-2 gap over the rows compared is at least the tie rule's 2e-4."""
    lg = logits[..., 0, : spec.n_discrete] if discrete else logits
    top2 = lg.topk(2, dim=-1).values
    return float((top2[..., 0] - top2[..., 1]).min())


def _steps(eng, seq, spec, discrete):
    acts, toks, lgs = [], [], []
    for obs, rtg, rew, _ in seq:
        a, t = eng.step(obs.to(DEV), rtg.to(DEV), rew.to(DEV), None, discrete=discrete)
        torch.cuda.synchronize()
        acts.append(a.clone().cpu()), toks.append(t.clone().cpu())
        lgs.append(eng.taps()[2].cpu().view(-1, spec.act_dim, spec.n_vocab))
    return torch.stack(acts, 1), torch.stack(toks, 1), torch.stack(lgs, 1)


def _check_against_steps(spec, res, acts, toks, lgs, discrete, what):
    L = acts.shape[1]
    cols = 1 if discrete else spec.act_dim
    gap = _no_ties(lgs, spec, discrete)
    assert gap >= 2e-4, f"{what}: the sequential run itself has a top-2 gap of {gap:.2e}: choose another seed"
    for t in range(L):
        ties = assert_actions_match(res.actions[:, t, :cols], acts[:, t, :cols], lgs[:, t], spec, discrete=discrete, what=f"{what} t={t}")
        assert ties == 0, (what, t)
        assert torch.equal(res.tokens[:, t, :cols].cpu(), toks[:, t, :cols]), (what, t)
        err = rel_err(res.logits[:, t, :cols], lgs[:, t, :cols])      # (columns a discrete call does not use are not written)
        assert err < 2e-4, (what, t, err)


@pytest.mark.parametrize("name,discrete", [("xlstm_tiny", False), ("xlstm_tiny", True), ("mamba_tiny", False)])
def test_score_equals_sequential_steps_and_prefill(hip_lib, name, discrete):
    spec = preset(name)
    sd = init_state_dict(spec, seed=17)
    B, L = 5, 9                                     # chunks of 4, 4 and 1 timesteps
    # (input seed 10: the CPU oracle's smallest top-2 gap over the three cases is 1.4e-3; seed 3 has one of 1.3e-4, a tie)
    seq = make_inputs(spec, B, L, seed=10, reset_prob=0.0)
    obs_seq, rtg_seq, rew_seq = _stack(seq)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    e_a, e_b, e_c = (_engine(spec, sd, B) for _ in range(3))
    acts, toks, lgs = _steps(e_a, seq, spec, discrete)
    target = toks.to(DEV).contiguous()              # the tokens the sequential run took
    res = e_b.score(obs_seq, rtg_seq, rew_seq, tokens=target, reset_mask=ones, discrete=discrete, logits=True)
    a_pre, _ = e_c.prefill(obs_seq, rtg_seq, rew_seq, reset_mask=ones, discrete=discrete)
    torch.cuda.synchronize()
    what = f"{name} discrete={discrete}"
    _check_against_steps(spec, res, acts, toks, lgs, discrete, what)
    cols = 1 if discrete else spec.act_dim
    _assert_2ulp(res.logp[:, :, :cols], _ref_logp(res.logits[:, :, :cols], target[:, :, :cols], spec.n_vocab, 1.0), what)
    _same_state(_state(e_b, spec), _state(e_c, spec), what)
    assert torch.equal(_bits(res.actions[:, L - 1]), _bits(a_pre)), what
    # the last timestep's logits are where a step leaves them
    assert torch.equal(_bits(e_b.taps()[2]), _bits(e_c.taps()[2])), what
    last = e_c.taps()[2].view(B, spec.act_dim, spec.n_vocab)
    assert torch.equal(_bits(res.logits[:, L - 1, :cols]), _bits(last[:, :cols])), what
    # one timestep is a one-step prefill
    r1 = e_b.score(obs_seq[:, :1].contiguous(), rtg_seq[:, :1].contiguous(), rew_seq[:, :1].contiguous(), discrete=discrete,
                   want=("actions",))
    a1, _ = e_c.prefill(obs_seq[:, :1].contiguous(), rtg_seq[:, :1].contiguous(), rew_seq[:, :1].contiguous(), discrete=discrete)
    torch.cuda.synchronize()
    assert torch.equal(_bits(r1.actions[:, 0]), _bits(a1)), what
    _same_state(_state(e_b, spec), _state(e_c, spec), what + " (one timestep)")
    for e in (e_a, e_b, e_c):
        e.close()


# ---- 3. / 4. the chunkwise kernels, the lanes, the bounded scratch --------------------------------------------------------------
def _float_targets(B, L, A, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, L, A, generator=g) * 2 - 1).contiguous()


@pytest.fixture(scope="module")
def m16():
    spec = preset("xlstm_16m")
    return spec, init_state_dict(spec, seed=41)


def test_score_through_the_chunkwise_kernels_against_the_oracle(hip_lib, m16, monkeypatch):
    """16M, 2 envs x 23 timesteps: chunks of 21 + 2, two lanes in flight.  Also the same call with the scratch bound at 16 rows
    (a chunk's 42 rows then take three blocks, the last one overlapping): bit-identical."""
    spec, sd = m16
    B, L = 2, 23
    seq = make_inputs(spec, B, L, seed=5, reset_prob=0.0)
    obs_seq, rtg_seq, rew_seq = _stack(seq)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    rec = _float_targets(B, L, spec.act_dim, 7)
    rec_tok = dt_ref.minmax_tokenize(rec, spec.action_channels, spec.n_discrete)
    e_s, e_p = _engine(spec, sd, B), _engine(spec, sd, B)
    monkeypatch.setenv("LRAM_SCORE_ROWS", "16")
    e_blk = _engine(spec, sd, B)
    monkeypatch.delenv("LRAM_SCORE_ROWS")
    res = e_s.score(obs_seq, rtg_seq, rew_seq, actions=rec.to(DEV), reset_mask=ones, logits=True)
    blk = e_blk.score(obs_seq, rtg_seq, rew_seq, actions=rec.to(DEV), reset_mask=ones, logits=True)
    a_pre, _ = e_p.prefill(obs_seq, rtg_seq, rew_seq, reset_mask=ones)
    torch.cuda.synchronize()
    ora = dt_ref.OraclePolicy(spec, sd)
    o_act, o_lg = [], []
    for obs, rtg, rew, _ in seq:
        a, dbg = ora.step(obs, rtg, rew, return_debug=True)
        o_act.append(a), o_lg.append(dbg["logits"])
    o_act, o_lg = torch.stack(o_act, 1), torch.stack(o_lg, 1)
    assert _no_ties(o_lg, spec, False) >= 2e-4
    o64 = None
    for t in range(L):
        ties = assert_actions_match(res.actions[:, t], o_act[:, t], o_lg[:, t], spec, what=f"t={t}")
        assert ties == 0, t
        scale = float(o_lg[:, t].abs().max())
        if rel_err(res.logits[:, t], o_lg[:, t]) >= 2e-4:      # an ill-conditioned timestep: as close to fp64 as the fp32 oracle is
            if o64 is None:
                f64 = Fp64Oracle(spec, sd)
                o64 = torch.stack([f64.step(obs, rtg, rew, return_debug=True)[1]["logits"] for obs, rtg, rew, _ in seq], 1)
            assert_close_or_as_close_as_fp32_oracle(res.logits[:, t], o_lg[:, t], o64[:, t], what=f"logits t={t}")
            want = _ref_logp(o64[:, t], rec_tok[:, t], spec.n_vocab, 1.0)      # the helper's cap on the logits, times two
            assert float((res.logp[:, t].cpu().double() - want).abs().max()) <= 2 * 5e-3 * scale, t
            continue
        want = _ref_logp(o_lg[:, t], rec_tok[:, t], spec.n_vocab, 1.0)
        err = float((res.logp[:, t].cpu().double() - want).abs().max())
        assert err <= 2 * 2e-4 * scale, (t, err, scale)
    _assert_2ulp(res.logp, _ref_logp(res.logits, rec_tok, spec.n_vocab, 1.0), "16M L=23, own logits")
    _same_state(_state(e_s, spec), _state(e_p, spec), "16M L=23")
    assert torch.equal(_bits(res.actions[:, L - 1]), _bits(a_pre))
    for name in ("actions", "tokens", "logp", "logits"):
        assert torch.equal(_bits(getattr(res, name)), _bits(getattr(blk, name))), f"bounded scratch: {name} differs"
    _same_state(_state(e_blk, spec), _state(e_p, spec), "16M L=23, bounded scratch")
    for e in (e_s, e_p, e_blk):
        e.close()


def test_score_over_four_chunks_against_sequential_steps(hip_lib, m16):
    """16M, 2 envs x 64 timesteps: four chunks of 16, lane 0 used twice.  Against 64 lram_step calls (the CPU oracle takes
    several seconds at this length)."""
    spec, sd = m16
    B, L = 2, 64
    seq = make_inputs(spec, B, L, seed=6, reset_prob=0.0)
    obs_seq, rtg_seq, rew_seq = _stack(seq)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    e_a, e_b, e_c = (_engine(spec, sd, B) for _ in range(3))
    acts, toks, lgs = _steps(e_a, seq, spec, False)
    target = toks.to(DEV).contiguous()
    res = e_b.score(obs_seq, rtg_seq, rew_seq, tokens=target, reset_mask=ones, logits=True)
    a_pre, _ = e_c.prefill(obs_seq, rtg_seq, rew_seq, reset_mask=ones)
    torch.cuda.synchronize()
    _check_against_steps(spec, res, acts, toks, lgs, False, "16M L=64")
    _assert_2ulp(res.logp, _ref_logp(res.logits, target, spec.n_vocab, 1.0), "16M L=64, own logits")
    for t in range(L):      # 2-Lipschitz: within twice the allowed logit difference of the sequential run's logits
        want = _ref_logp(lgs[:, t], toks[:, t], spec.n_vocab, 1.0)
        assert float((res.logp[:, t].cpu().double() - want).abs().max()) <= 2 * 2e-4 * float(lgs[:, t].abs().max()), t
    _same_state(_state(e_b, spec), _state(e_c, spec), "16M L=64")
    assert torch.equal(_bits(res.actions[:, L - 1]), _bits(a_pre))
    for e in (e_a, e_b, e_c):
        e.close()


# ---- 5. masks and slots end to end -----------------------------------------------------------------------------------------------
def test_valid_mask_and_slot_table_end_to_end(hip_lib):
    from lram_amd.domains import Domain, SlotTable
    spec = dataclasses.replace(preset("xlstm_tiny"), act_dim=8)
    sd = init_state_dict(spec, seed=19, with_image_encoder=True)
    tab = SlotTable.from_domains([(Domain("atari", True, 1), 2), (Domain("metaworld", False, 3), 1), (Domain("dmc", False, 6), 1)],
                                 max_act_dim=spec.act_dim)
    B, L, A = 4, 9, spec.act_dim
    used = tab.act_dim.tolist()
    assert used == [1, 1, 3, 6] and tab.discrete.tolist() == [True, True, False, False]
    seq = make_inputs(spec, B, L, seed=23, reset_prob=0.0)
    obs_seq, rtg_seq, rew_seq = _stack(seq)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    rec = _float_targets(B, L, A, 29)
    rec[:2, :, 0] = torch.randint(0, spec.n_discrete, (2, L), generator=torch.Generator().manual_seed(2)).float()   # the discrete slots' action index
    lengths = torch.tensor([0, 9, 4, 7])
    valid = (torch.arange(L).reshape(1, L) < lengths.reshape(B, 1))
    e_full, e_mask = _engine(spec, sd, B), _engine(spec, sd, B)
    for e in (e_full, e_mask):
        e.set_slot_table(*tab.engine_arrays())
    kw = dict(actions=rec.to(DEV), reset_mask=ones, discrete="per_slot", over="selectable", logits=True)
    full = e_full.score(obs_seq, rtg_seq, rew_seq, **kw)
    part = e_mask.score(obs_seq, rtg_seq, rew_seq, valid=valid.to(DEV), **kw)
    torch.cuda.synchronize()
    col = torch.arange(A).reshape(1, 1, A) < torch.tensor(used).reshape(B, 1, 1)
    live_full = col.expand(B, L, A)
    live_part = live_full & valid.reshape(B, L, 1)
    for res, live, what in ((full, live_full, "unmasked"), (part, live_part, "masked")):
        a, tok, lp = res.actions.cpu(), res.tokens.cpu(), res.logp.cpu()
        assert bool((_bits(a[~live]) == 0).all()) and bool((_bits(lp[~live]) == 0).all()) and bool((tok[~live] == -1).all()), what
        assert bool((tok[live] >= 0).all()), what
        assert bool((res.logits.cpu()[~live] == 0).all()), what
    for name in ("actions", "tokens", "logp", "logits"):
        x, y = getattr(full, name).cpu(), getattr(part, name).cpu()
        assert torch.equal(_bits(x[live_part]), _bits(y[live_part])), name
    _same_state(_state(e_full, spec), _state(e_mask, spec), "valid mask")
    # every slot was scored with its own head: range, greedy token and target as the table says
    lg = full.logits.cpu()
    for b in range(B):
        n = spec.n_discrete if tab.discrete[b] else spec.n_vocab
        k = used[b]
        assert torch.equal(full.tokens[b, :, :k].cpu().long(), torch.argmax(lg[b, :, :k, :n], dim=-1)), b
        tgt = rec[b, :, :k].long() if tab.discrete[b] else dt_ref.minmax_tokenize(rec[b, :, :k], spec.action_channels, spec.n_discrete)
        _assert_2ulp(full.logp[b, :, :k], _ref_logp(lg[b, :, :k], tgt, n, 1.0), f"slot {b}")
    e_full.close(), e_mask.close()


# ---- 6. the log-probability of the tokens just taken ---------------------------------------------------------------------------------
def test_last_logp_scores_the_drawn_tokens_and_consumes_no_draw(hip_lib):
    spec = preset("xlstm_tiny")
    sd = init_state_dict(spec, seed=31)
    B, L = 5, 6
    seq = make_inputs(spec, B, L, seed=37, reset_prob=0.0)
    obs_seq, rtg_seq, rew_seq = _stack(seq)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    T = 0.75
    e1, e2, e_plain = (_engine(spec, sd, B) for _ in range(3))
    for e in (e1, e2):
        e.set_sampling(temperature=T, top_k=0, top_p=0.0, seed=20261018)
    step = lambda e, i: e.step(seq[i][0].to(DEV), seq[i][1].to(DEV), seq[i][2].to(DEV), None)
    _, tok1 = step(e1, 0)
    _, tok2 = step(e2, 0)
    torch.cuda.synchronize()
    assert torch.equal(tok1, tok2)
    lp = e1.last_logp(tok1, over="selectable", temperature=T)
    torch.cuda.synchronize()
    lg = e1.taps()[2].view(B, spec.act_dim, spec.n_vocab)
    _assert_2ulp(lp, _ref_logp(lg, tok1, spec.n_vocab, T), "last_logp")
    assert bool((lp.cpu() < 0).all()) and bool(lp.cpu().isfinite().all())
    # a score in between (the state put back afterwards): deterministic, greedy, no draw
    keep = e1.save_slots(list(range(B)))
    armed = e1.score(obs_seq, rtg_seq, rew_seq, reset_mask=ones, want=("tokens",))
    e1.load_slots(list(range(B)), keep)
    plain = e_plain.score(obs_seq, rtg_seq, rew_seq, reset_mask=ones, want=("tokens",))
    torch.cuda.synchronize()
    assert torch.equal(armed.tokens, plain.tokens)
    assert e1.sampling["draws"] == 1 and e2.sampling["draws"] == 1
    _, tok1 = step(e1, 1)
    _, tok2 = step(e2, 1)
    torch.cuda.synchronize()
    assert torch.equal(tok1, tok2)
    for e in (e1, e2, e_plain):
        e.close()


def test_agent_scores_trajectories_and_its_own_actions(hip_lib):
    from lram_amd.agent import RecurrentAgent
    from lram_amd.rollout import score_loss
    spec = preset("xlstm_tiny")
    sd = init_state_dict(spec, seed=33)
    B, L, n_obs, n_act = 3, 7, 11, 3
    g = torch.Generator().manual_seed(5)
    mean, std = torch.randn(spec.state_dim, generator=g) * 0.1, torch.rand(spec.state_dim, generator=g) + 0.5
    agent = RecurrentAgent(spec, sd, n_envs=B, device=DEV, state_mean=mean, state_std=std)
    obs = torch.rand(B, L, n_obs, generator=g) * 2 - 1
    rtg = torch.full((B, L), 3.0) - 0.01 * torch.arange(L)
    rec = torch.rand(B, L, n_act, generator=g) * 2 - 1
    lengths = torch.tensor([7, 2, 5])
    res = agent.score_trajectories(obs, rtg, actions=rec, lengths=lengths, logits=True)
    torch.cuda.synchronize()
    valid = torch.arange(L).reshape(1, L) < lengths.reshape(B, 1)
    act_mask = torch.arange(spec.act_dim) < n_act
    tok = dt_ref.minmax_tokenize(rec, spec.action_channels, spec.n_discrete)
    want = _ref_logp(res.logits[:, :, :n_act], tok, spec.n_vocab, 1.0)
    _assert_2ulp(res.logp[:, :, :n_act][valid], want[valid], "score_trajectories")
    assert bool((res.tokens.cpu()[~valid] == -1).all())
    loss = score_loss(res, valid, act_mask.expand(B, spec.act_dim))
    ref = (-want[valid]).mean(dim=-1).mean()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    # the same trajectories stepped through predict_batch give the greedy actions score_trajectories reported
    agent.engine.reset()
    for t in range(L):
        a = agent.predict_batch(obs[:, t], rtg[:, t])
        lp = agent.action_log_prob(over="vocab")
        torch.cuda.synchronize()
        lg = agent.engine.taps()[2].view(B, spec.act_dim, spec.n_vocab)
        v = valid[:, t]
        assert assert_actions_match(res.actions[:, t].cpu()[v], a.cpu()[v], lg.cpu()[v], spec, what=f"t={t}") == 0, t
        _assert_2ulp(lp, _ref_logp(lg, agent.engine._tokens, spec.n_vocab, 1.0), f"action_log_prob t={t}")
    agent.engine.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_leave_the_state_alone(hip_lib):
    from lram_amd.engine import LramError
    spec = preset("mamba_tiny")
    sd = init_state_dict(spec, seed=3)
    B, L = 3, 5
    seq = make_inputs(spec, B, L, seed=9, reset_prob=0.0)
    obs_seq, rtg_seq, rew_seq = _stack(seq)
    eng = _engine(spec, sd, B)
    tok = torch.zeros(B, spec.act_dim, dtype=torch.int32, device=DEV)
    tok_seq = torch.zeros(B, L, spec.act_dim, dtype=torch.int32, device=DEV)
    act_seq = torch.zeros(B, L, spec.act_dim, device=DEV)

    def refused(call, *needles):
        before = _state(eng, spec)
        with pytest.raises(LramError) as err:
            call()
        msg = str(err.value)
        assert all(n in msg for n in needles), msg
        _same_state(before, _state(eng, spec), msg)

    refused(lambda: eng.last_logp(tok), "lram_score_last", "no action-producing call")
    eng.step(seq[0][0].to(DEV), seq[0][1].to(DEV), seq[0][2].to(DEV), None)
    eng.step(seq[1][0].to(DEV), seq[1][1].to(DEV), seq[1][2].to(DEV), None)
    torch.cuda.synchronize()
    assert float(_state(eng, spec)[0].abs().max()) > 0
    refused(lambda: eng.score(obs_seq, rtg_seq, rew_seq, actions=act_seq, tokens=tok_seq), "lram_score", "both")
    refused(lambda: eng.score(obs_seq, rtg_seq, rew_seq, want=()), "lram_score", "no output")
    refused(lambda: eng.score(obs_seq, rtg_seq, rew_seq, want=("logp",)), "lram_score", "needs a target")
    eng.set_compat_mode(3, False)
    refused(lambda: eng.score(obs_seq, rtg_seq, rew_seq, tokens=tok_seq), "lram_score", "mamba_repeat")
    eng.set_compat_mode(1, False)
    # ... and the engine is usable afterwards
    res = eng.score(obs_seq, rtg_seq, rew_seq, tokens=tok_seq)
    torch.cuda.synchronize()
    assert bool(res.logp.cpu().isfinite().all())
    assert bool(eng.last_logp(tok).cpu().isfinite().all())
    eng.close()
