"""GPU: every token front-end and action-head geometry `lram_create` accepts, not only the two every other test uses (20 / 4 / 256 /
18 and the published 204 / 8 / 256 / 18), against the CPU oracle (tests/head_cases.py: V = 2 .. 518, N = act_dim * V from 2 to
8704 with an odd row pitch among them, K = state_dim from 4 to 1028, 1 / 64 / 100 / 495 / 500 action channels, discrete heads of
0, 1, 7, 18 and 300 logits, pred_token 0 / 1 / 2).  These numbers choose the kernel of the state Linear and of the head GEMM, the
instance of the sampling kernel, the strides of all three head kernels and the bin width of the de-tokenisation.

Bars (the project's fixed ones, none tuned to the output): embedded tokens 1e-5 and logits 2e-4 by helpers.rel_err, as
test_gpu_parity._run_parity holds the taps; tokens EQUAL the oracle's argmax on every row whose oracle top-2 gap is at least 1e-3
(rows below it are left out of the token comparison only, at most 2 % of a run; the seeds of head_cases.SEEDS leave out at
most 1 % on the CPU); actions equal oracle.dt_ref.minmax_inv_tokenize of the tokens BIT FOR BIT whatever the channel count
(the kernels round the product and the sum separately, as the reference does); logp within 2 fp32 ulps of a float64
log-softmax of the same logits (test_gpu_score._assert_2ulp)."""
import functools

import pytest
import torch

from lram_amd import init_state_dict
from oracle import dt_ref
from tests import head_cases as hc
from tests.helpers import make_inputs, rel_err
from tests.test_gpu_sampling import _check_step
from tests.test_gpu_score import _assert_2ulp, _bits, _ref_logp, _same_state, _state

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BBS = list(hc.BACKBONES)


def _engine(spec, sd, B):
    from lram_amd.engine import Engine
    return Engine(spec, sd, B, device=DEV)


@functools.lru_cache(maxsize=None)
def _reference(cid, bb, B, seed, steps=hc.STEPS, reset_prob=hc.RESET_PROB, discrete=False, pred=1, repeat=1):
    """(spec, weights, inputs, oracle steps) of one run: computed once, shared by the tests that need it, never modified."""
    spec = hc.case_spec(cid, bb, pred)
    sd = init_state_dict(spec, seed=seed)
    seq = make_inputs(spec, B, steps, seed=1234 + seed, reset_prob=reset_prob)
    kw = {"mamba_repeat": repeat} if repeat != 1 else {}
    return spec, sd, seq, hc.oracle_steps(spec, sd, seq, discrete=discrete, **kw)


def _dev(inp):
    return tuple(x.to(DEV) for x in inp)


def _seq_tensors(seq):
    return tuple(torch.stack([x[i] for x in seq], 1).contiguous().to(DEV) for i in range(3))


class _Tally:
    """Rows compared / left out / wrong over one run."""

    def __init__(self, what):
        self.what, self.rows, self.left_out = what, 0, 0

    def tokens(self, got, want, clear, where):
        got, want = got.cpu().long().reshape(want.shape), want.long()
        wrong = (got != want) & clear
        self.rows += clear.numel()
        self.left_out += int((~clear).sum())
        assert not bool(wrong.any()), f"{self.what} {where}: {int(wrong.sum())} tokens differ from the oracle's argmax on rows with a " \
                                      f"top-2 gap >= {hc.GAP:g} (first: row {wrong.nonzero()[0].tolist()}, got {int(got[wrong][0])} " \
                                      f"want {int(want[wrong][0])})"

    def done(self):
        share = self.left_out / max(1, self.rows)
        print(f"[head sweep] {self.what}: {self.rows} rows, 0 token mismatches, {self.left_out} left out ({share:.2%})")
        assert share <= hc.MAX_LEFT_OUT, f"{self.what}: {share:.2%} of the rows were left out of the token comparison"


def _check_actions(spec, a, tok, discrete, what):
    """Actions are the de-tokenised tokens bit for bit (all rows: this needs no oracle margin)."""
    a, tok = a.cpu(), tok.cpu()
    if discrete:
        assert torch.equal(_bits(a[:, 0]), _bits(tok[:, 0].float())), f"{what}: discrete action != float(token)"
        assert bool(((tok[:, 0] >= 0) & (tok[:, 0] < spec.n_discrete)).all()), f"{what}: discrete token out of range"
    else:
        want = dt_ref.minmax_inv_tokenize(tok.long(), spec.action_channels, spec.n_discrete)
        assert torch.equal(_bits(a), _bits(want)), f"{what}: {int((_bits(a) != _bits(want)).sum())} actions are not " \
                                                   f"minmax_inv_tokenize(token) bit for bit ({spec.action_channels} channels)"
        assert bool(((tok >= 0) & (tok < spec.n_vocab)).all()), f"{what}: token out of range"


def _run_steps(eng, spec, seq, ref, what, discrete=False):
    """lram_step over seq against the oracle steps `ref`: both taps, tokens under the gap rule, actions bit for bit."""
    tally = _Tally(what)
    B, cols = eng.batch, 1 if discrete else spec.act_dim
    for t, inp in enumerate(seq):
        obs, rtg, rew, mask = _dev(inp)
        a, tok = eng.step(obs, rtg, rew, mask, discrete=discrete)
        torch.cuda.synchronize()
        tokens_tap, _, logits = eng.taps()
        a_ref, tok_ref, lg_ref, emb_ref, clear = ref[t]
        if tokens_tap is not None:
            err = rel_err(tokens_tap, emb_ref)
            assert err < 1e-5, f"{what} step {t}: embedded tokens {err:.2e}"
        err = rel_err(logits.view(B, spec.act_dim, spec.n_vocab)[:, :cols], lg_ref)
        assert err < 2e-4, f"{what} step {t}: logits {err:.2e}"
        tally.tokens(tok[:, :cols], tok_ref, clear, f"step {t}")
        _check_actions(spec, a, tok, discrete, f"{what} step {t}")
    tally.done()


# ---------------------------------------------------------------------------------------------------------------------
# 1. step parity: every case, both backbones, batches on both sides of every kernel switch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,bb,B,micro", hc.STEP_RUNS, ids=[f"{c}-{bb}-{B}" + (f"-slices{m}" if m else "") for c, bb, B, m in hc.STEP_RUNS])
def test_step_parity_against_the_oracle(hip_lib, cid, bb, B, micro):
    """4 env-steps with random restarts.  3 rows take the GEMV, 7 / 40 the few-row kernel (the fp32 tile kernel where K < 32 or
    K > 1024), 264 / 400 the f16x2 head; 264 slots in two slices of 132 put the head back on the few-row kernel."""
    seed, share = hc.SEEDS[(cid, bb, B)]
    assert share <= 0.01
    spec, sd, seq, ref = _reference(cid, bb, B, seed)
    eng = _engine(spec, sd, B)
    if micro:
        eng.set_micro_batches(micro)
    _run_steps(eng, spec, seq, ref, f"{cid}/{bb} B={B}" + (f" slices={micro}" if micro else ""))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the discrete head: 1, 7, 18 and 300 logits; refused where there is none
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bb", BBS)
@pytest.mark.parametrize("cid", ["mt_disc", "two", "odd", "disc300"])
def test_discrete_head(hip_lib, cid, bb):
    seed, _ = hc.SEEDS[(cid, bb, 7)]
    spec, sd, seq, ref = _reference(cid, bb, 7, seed, discrete=True)
    eng = _engine(spec, sd, 7)
    _run_steps(eng, spec, seq, ref, f"{cid}/{bb} discrete", discrete=True)
    eng.close()


@pytest.mark.parametrize("bb", BBS)
def test_discrete_calls_are_refused_without_discrete_actions(hip_lib, bb):
    """n_discrete = 0 (the reference's dmcontrol head): every entry that would take an argmax over no logits refuses before it
    launches anything -- the recurrent state is bit for bit what it was -- and the engine goes on stepping."""
    from lram_amd.engine import LramError
    B, L = 7, 3
    seed, _ = hc.SEEDS[("dmc", bb, B)]
    spec, sd, seq, ref = _reference("dmc", bb, B, seed)
    assert spec.n_discrete == 0
    eng = _engine(spec, sd, B)
    obs, rtg, rew, mask = _dev(seq[0])
    a0, t0 = (x.clone() for x in eng.step(obs, rtg, rew, mask))
    before = _state(eng, spec)
    obs_seq, rtg_seq, rew_seq = _seq_tensors(seq[:L])
    tok_seq = torch.zeros(B, L, spec.act_dim, dtype=torch.int32, device=DEV)
    with pytest.raises(LramError, match="lram_step: a discrete head needs n_discrete >= 1"):
        eng.step(obs, rtg, rew, mask, discrete=True)
    with pytest.raises(LramError, match="lram_prefill: a discrete head needs n_discrete >= 1"):
        eng.prefill(obs_seq, rtg_seq, rew_seq, discrete=True)
    with pytest.raises(LramError, match="lram_score: a discrete head needs n_discrete >= 1"):
        eng.score(obs_seq, rtg_seq, rew_seq, tokens=tok_seq, discrete=True)
    with pytest.raises(LramError, match="a discrete slot needs n_discrete > 0"):
        eng.set_slot_table([True] + [False] * (B - 1), [1] * B)
    assert eng.slot_table() is None
    _same_state(before, _state(eng, spec), "after the refused discrete calls")
    # armed for sampling: the refused discrete step left the last head as it was (continuous), so the drawn distribution that
    # lram_score_last_sampled scores is the continuous one; a discrete step is still refused
    eng.set_sampling(temperature=0.75, top_k=10, top_p=0.5, seed=3)
    with pytest.raises(LramError, match="lram_step: a discrete head needs n_discrete >= 1"):
        eng.step(obs, rtg, rew, mask, discrete=True)
    lp = eng.last_logp(t0, over="sampled")
    torch.cuda.synchronize()
    assert lp.shape == (B, spec.act_dim) and not bool(lp.isnan().any())
    _same_state(before, _state(eng, spec), "after the refused sampled discrete step")
    eng.set_sampling(None)
    # ... and the run continues as if nothing had been asked
    tally = _Tally(f"dmc/{bb} after refusals")
    tally.tokens(t0, ref[0][1], ref[0][4], "step 0")
    for t in range(1, len(seq)):
        a, tok = eng.step(*_dev(seq[t]))
        torch.cuda.synchronize()
        tally.tokens(tok, ref[t][1], ref[t][4], f"step {t}")
        _check_actions(spec, a, tok, False, f"dmc/{bb} step {t}")
    tally.done()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. stored contexts: lram_prefill and lram_score over 9 timesteps
# ---------------------------------------------------------------------------------------------------------------------
def _check_context(cid, bb, pred=1):
    B, L = 7, hc.CONTEXT_L
    seed, _ = hc.SEEDS[(cid, bb, B)]
    spec, sd, seq, ref = _reference(cid, bb, B, seed, steps=L, reset_prob=0.0, pred=pred)
    what = f"{cid}/{bb} pred_token={pred} L={L}"
    obs_seq, rtg_seq, rew_seq = _seq_tensors(seq)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    e_p, e_s = _engine(spec, sd, B), _engine(spec, sd, B)
    act, tok = (x.clone() for x in e_p.prefill(obs_seq, rtg_seq, rew_seq, reset_mask=ones))
    torch.cuda.synchronize()
    tally = _Tally(what + " prefill")
    tally.tokens(tok, ref[L - 1][1], ref[L - 1][4], "last timestep")
    tally.done()
    _check_actions(spec, act, tok, False, what + " prefill")
    # recorded float actions: the oracle's own actions (bin edges, where tokenising is least forgiving) on half the entries,
    # uniform values on the other half
    g = torch.Generator().manual_seed(seed)
    edges = torch.stack([r[0] for r in ref], 1)
    rec = torch.where(torch.rand(edges.shape, generator=g) < 0.5, edges, torch.rand(edges.shape, generator=g) * 2 - 1).contiguous()
    res = e_s.score(obs_seq, rtg_seq, rew_seq, actions=rec.to(DEV), reset_mask=ones, logits=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(res.actions[:, L - 1]), _bits(act)), f"{what}: score's last row is not prefill's action"
    assert torch.equal(res.tokens[:, L - 1], tok), f"{what}: score's last row is not prefill's token"
    _same_state(_state(e_p, spec), _state(e_s, spec), what + ": state after score vs after prefill")
    for t in range(L):
        err = rel_err(res.logits[:, t], ref[t][2])
        assert err < 2e-4, f"{what} t={t}: logits {err:.2e}"
        _check_actions(spec, res.actions[:, t], res.tokens[:, t], False, f"{what} score t={t}")
    assert torch.equal(res.tokens.cpu().long(), res.logits.cpu().argmax(-1)), f"{what}: score tokens are not the argmax of its logits"
    target = dt_ref.minmax_tokenize(rec, spec.action_channels, spec.n_discrete)
    _assert_2ulp(res.logp, _ref_logp(res.logits, target, spec.n_vocab, 1.0), what + " logp")
    e_p.close(), e_s.close()


@pytest.mark.parametrize("bb", BBS)
@pytest.mark.parametrize("cid", list(hc.CASES))
def test_prefill_and_score_over_nine_timesteps(hip_lib, cid, bb):
    """27 tokens: on Mamba more than one token-sequential chunk.  The state Linear runs over all 63 timestep rows at once
    (lda = L * state_dim per env in the step form, one GEMM over B * L rows in the stored-context form); the head runs at every
    timestep in row blocks on the fp32 tile kernel."""
    _check_context(cid, bb)


# ---------------------------------------------------------------------------------------------------------------------
# 4. sampling: PER 1 / 5 / 8 at their limits, V = 2, odd strides, a discrete head of 300 logits; refused past 512 logits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bb", BBS)
@pytest.mark.parametrize("cid", ["dmc", "two", "odd", "v320", "wide", "disc300"])
def test_sampled_tokens_are_drawn_from_the_steps_own_logits(hip_lib, cid, bb):
    B = 7
    seed, _ = hc.SEEDS[(cid, bb, B)]
    spec, sd, seq, _ = _reference(cid, bb, B, seed)
    discrete = cid == "disc300"
    kw = dict(temperature=0.75, top_k=200, top_p=0.5) if discrete else dict(temperature=0.75, top_k=min(10, spec.n_vocab), top_p=0.5)
    eng = _engine(spec, sd, B)
    eng.set_sampling(seed=20261019, slot_base=2 ** 32 - 4, **kw)
    off_argmax = 0
    for t, inp in enumerate(seq):
        a, tok = eng.step(*_dev(inp), discrete=discrete)
        _check_step(eng, spec, a, tok, discrete, kw, 20261019, 2 ** 32 - 4, t, f"{cid}/{bb} sampled step {t}")
        lg = eng.taps()[2].view(B, spec.act_dim, spec.n_vocab)
        am = lg[:, 0, : spec.n_discrete].argmax(-1) if discrete else lg.argmax(-1)
        off_argmax += int(((tok[:, 0] if discrete else tok) != am).sum())
    assert eng.sampling["draws"] == len(seq)
    if spec.n_vocab > 2:
        assert off_argmax > 0, "every sampled token was the argmax: nothing was drawn"
    eng.close()


@pytest.mark.parametrize("bb", BBS)
def test_sampling_is_refused_past_512_logits_and_the_argmax_path_goes_on(hip_lib, bb):
    from lram_amd.engine import LramError
    B = 7
    seed, _ = hc.SEEDS[("over512", bb, B)]
    spec, sd, seq, ref = _reference("over512", bb, B, seed)
    assert spec.n_vocab == 518
    eng = _engine(spec, sd, B)
    with pytest.raises(LramError, match="lram_set_sampling: the sampling kernel holds rows of up to 512 logits"):
        eng.set_sampling(temperature=0.75, top_k=10, top_p=0.5, seed=1)
    assert eng.sampling is None
    _run_steps(eng, spec, seq, ref, f"over512/{bb} after the refused set_sampling")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the slot table on rows of 107 logits at an odd pitch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bb", BBS)
def test_slot_table_on_the_odd_geometry(hip_lib, bb):
    """Slots with 1, 2 and 3 action dims and discrete slots under discrete = LRAM_HEAD_PER_SLOT: the argmax head against the oracle
    (whose state does not depend on the head), the sampled head against lram_sample_tokens on the step's own logits.  Columns a
    slot does not use hold 0.0f / -1."""
    from lram_amd.engine import sample_tokens, sample_uniforms
    B = 7
    seed, _ = hc.SEEDS[("odd", bb, B)]
    spec, sd, seq, ref = _reference("odd", bb, B, seed)
    A, V, ND = spec.act_dim, spec.n_vocab, spec.n_discrete
    disc = [False, False, False, True, False, False, True]
    used = [1, 2, 3, 1, 3, 2, 1]
    kw = dict(temperature=0.75, top_k=5, top_p=0.5)
    e_a, e_s = _engine(spec, sd, B), _engine(spec, sd, B)
    for e in (e_a, e_s):
        e.set_slot_table(disc, used)
    e_s.set_sampling(seed=77, slot_base=5, **kw)
    tally = _Tally(f"odd/{bb} slot table")
    for t, inp in enumerate(seq):
        _, _, lg_ref, _, _ = ref[t]
        a, tok = (x.clone() for x in e_a.step(*_dev(inp), discrete="per_slot"))
        a_s, tok_s = (x.clone() for x in e_s.step(*_dev(inp), discrete="per_slot"))
        torch.cuda.synchronize()
        lg = e_s.taps()[2].view(B, A, V)
        u = sample_uniforms(77, 5, B, A, t, device=DEV)
        for b in range(B):
            n = used[b]
            if disc[b]:
                row = lg_ref[b, :1, :ND]
                tally.tokens(tok[b, :1], row.argmax(-1), hc.gaps(row) >= hc.GAP, f"step {t} slot {b}")
                assert torch.equal(_bits(a[b, :1]), _bits(tok[b, :1].float()))
                want = sample_tokens(lg[b, :1, :ND], u[b, :1].contiguous(), **kw)
                assert torch.equal(tok_s[b, :1], want) and torch.equal(_bits(a_s[b, :1]), _bits(want.float())), (t, b)
            else:
                tally.tokens(tok[b, :n], lg_ref[b, :n].argmax(-1), hc.gaps(lg_ref[b, :n]) >= hc.GAP, f"step {t} slot {b}")
                want = sample_tokens(lg[b, :n].contiguous(), u[b, :n].contiguous(), **kw)
                assert torch.equal(tok_s[b, :n], want), (t, b)
                for act, tk in ((a, tok), (a_s, tok_s)):
                    inv = dt_ref.minmax_inv_tokenize(tk[b, :n].cpu().long(), spec.action_channels, ND)
                    assert torch.equal(_bits(act[b, :n].cpu()), _bits(inv)), (t, b)
            for act, tk in ((a, tok), (a_s, tok_s)):   # unused columns: the fill values, exactly
                assert bool((_bits(act[b, n:]) == 0).all()) and bool((tk[b, n:] == -1).all()), (t, b)
    tally.done()
    assert e_s.sampling["draws"] == len(seq)
    e_a.close(), e_s.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. Mamba's repeated forwards: column blocks of the head at odd float offsets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 7, 264])
def test_mamba_repeated_forwards_on_the_odd_geometry(hip_lib, B):
    """mamba_repeat = 3 with act_dim 3 and V = 107: forward p evaluates the head on the column block from p * 107 floats on -- an
    output pointer that is 4-byte aligned only -- through the GEMV (3 rows), the few-row kernel (7) and the f16x2 kernel (264)."""
    seed, share = hc.REPEAT_SEEDS[B]
    assert share <= 0.01
    spec, sd, seq, ref = _reference("odd", "mamba", B, seed, repeat=3)
    eng = _engine(spec, sd, B)
    eng.set_compat_mode(mamba_repeat=3)
    _run_steps(eng, spec, seq, ref, f"odd/mamba repeat=3 B={B}")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the action read from another token row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bb", BBS)
@pytest.mark.parametrize("pred", [0, 2])
def test_pred_token_other_than_the_rtg_token(hip_lib, pred, bb):
    """pred_token 0 / 2 (accepted by lram_create; every configuration of the reference has 1): the head reads the state token's /
    the reward token's row of the hidden states in lram_step, lram_prefill and at every timestep of lram_score."""
    seed, share = hc.PRED_SEEDS[(pred, bb)]
    assert share <= 0.01
    spec, sd, seq, ref = _reference("mt_disc", bb, 7, seed, pred=pred)
    assert spec.pred_token == pred
    base = _reference("mt_disc", bb, 7, seed)[3]
    assert any(not torch.equal(r[2], r1[2]) for r, r1 in zip(ref, base)), "the oracle reads the same row whatever pred_token"
    eng = _engine(spec, sd, 7)
    _run_steps(eng, spec, seq, ref, f"mt_disc/{bb} pred_token={pred}")
    eng.close()
    _check_context("mt_disc", bb, pred=pred)
