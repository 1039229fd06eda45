"""GPU: one row gives one token and one action from every kernel of the action head.  The argmax, sampling and score kernels
apply the same row rules (csrc/action_head.h: which columns a slot uses, the argmax by torch's NaN / first-index rule, the
de-tokenisation); this runs the logits of ONE env-step through all of them and compares every row, with no tolerance and no row
left out:

  step      lram_step, argmax head, under a slot table that mixes discrete and continuous slots with differing act_dim
  score     lram_score_tokens on the step's logits tap (per head mode: that entry takes no table)
  rows      lram_sample_rows on the same logits, mode 0 (greedy) on every row
  sampled   lram_step on a second engine armed with top_k = 1

Geometries (tests/head_cases.py): one row width per PER class of the staged kernels and both of its edges -- V = 2, 64 | 65, 107,
320 | 321, 512 -- and a discrete head of 300 logits.  7 env slots (the last workgroup is partly empty); slot 1 is fed a NaN
observation (its rows are all NaN: every index ties, the first wins) and slot 4 an all-zero one."""
import pytest
import torch

from lram_amd import init_state_dict
from tests import head_cases as hc
from tests.helpers import make_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 7
GEOMETRIES = ["two", "dmc", "v65", "odd", "v320", "v321", "wide", "disc300"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _table(spec):
    """Slots 2 and 4 discrete where the head has discrete actions; the others use 1 .. act_dim action dims."""
    disc = [spec.n_discrete > 0 and b in (2, 4) for b in range(B)]
    used = [1 if disc[b] else 1 + (b + 1) % spec.act_dim for b in range(B)]
    return disc, used


def test_the_geometries_cover_every_per_class_and_its_edges():
    widths = {hc.case_spec(c, "xlstm").n_vocab for c in GEOMETRIES}
    assert {2, 64, 65, 320, 321, 512} <= widths
    assert hc.case_spec("disc300", "xlstm").n_discrete == 300


@pytest.mark.parametrize("cid", GEOMETRIES)
def test_one_row_gives_one_token_and_one_action_from_every_head_kernel(hip_lib, cid):
    from lram_amd.engine import Engine, sample_rows, score_tokens
    spec = hc.case_spec(cid, "xlstm")
    A, V, ND = spec.act_dim, spec.n_vocab, spec.n_discrete
    sd = init_state_dict(spec, seed=1)
    obs, rtg, rew, mask = (x.to(DEV) for x in make_inputs(spec, B, 1, seed=77)[0])
    obs[1] = float("nan")
    obs[4] = 0.0
    disc, used = _table(spec)
    assert len(set(used)) > 1 or A == 1

    def step(eng):
        # (the outputs start from values no head writes, so that a column left alone shows)
        a = torch.full((B, A), 7.5, dtype=torch.float32, device=DEV)
        t = torch.full((B, A), 99999, dtype=torch.int32, device=DEV)
        eng.step(obs, rtg, rew, mask, discrete="per_slot", out_actions=a, out_tokens=t)
        torch.cuda.synchronize()
        return a.cpu(), t.cpu()

    e_a, e_s = Engine(spec, sd, B, device=DEV), Engine(spec, sd, B, device=DEV)
    for e in (e_a, e_s):
        e.set_slot_table(disc, used)
    e_s.set_sampling(temperature=1.0, top_k=1, seed=5)
    act, tok = step(e_a)
    lg = e_a.taps()[2].view(B, A, V).contiguous()
    act_s, tok_s = step(e_s)
    assert torch.equal(_bits(e_s.taps()[2]), _bits(lg.view(B, -1))), "the two engines disagree on the logits themselves"
    assert bool(lg[1].isnan().all()), "slot 1's rows are not all NaN: the NaN observation did not reach the head"
    assert not bool(lg[[0, 2, 3, 4, 5, 6]].isnan().any()), "the NaN observation left its slot"

    # score kernel and row kernel on the same logits, per head mode
    zeros = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)  # noqa: E731
    sc = {False: score_tokens(lg, spec, discrete=False, want=("actions", "tokens"))}
    rows = {False: sample_rows(lg.view(B * A, V), greedy=True, uniform=zeros(B * A))[0].view(B, A).cpu()}
    if ND > 0:
        sc[True] = score_tokens(lg, spec, discrete=True, want=("actions", "tokens"))
        rows[True] = sample_rows(lg[:, 0, :ND], greedy=True, uniform=zeros(B))[0].view(B, 1).cpu()
    torch.cuda.synchronize()
    if ND > 0:   # the score kernel's own fill values on the columns a discrete call does not use
        assert bool((sc[True].tokens[:, 1:] == -1).all()) and bool((_bits(sc[True].actions[:, 1:]) == 0).all())

    compared = 0
    for b in range(B):
        n, s = used[b], sc[disc[b]]
        s_tok, s_act = s.tokens[b, :n].cpu(), s.actions[b, :n].cpu()
        where = f"{cid} slot {b} ({'discrete' if disc[b] else 'continuous'}, {n} dims)"
        assert torch.equal(tok[b, :n], s_tok), f"{where}: step tokens {tok[b, :n].tolist()} != score tokens {s_tok.tolist()}"
        assert torch.equal(tok[b, :n], rows[disc[b]][b, :n]), f"{where}: step tokens != lram_sample_rows' greedy tokens"
        assert torch.equal(_bits(act[b, :n]), _bits(s_act)), f"{where}: step actions are not the score kernel's bit for bit"
        assert torch.equal(tok_s[b, :n], tok[b, :n]), f"{where}: the step sampled with top_k = 1 != the argmax step's tokens"
        assert torch.equal(_bits(act_s[b, :n]), _bits(act[b, :n])), f"{where}: ... nor its actions"
        for a_, t_ in ((act, tok), (act_s, tok_s)):   # columns the table marks unused: the fill values, exactly
            assert bool((t_[b, n:] == -1).all()) and bool((_bits(a_[b, n:]) == 0).all()), f"{where}: unused columns are not -1 / 0"
        compared += n
    assert compared == sum(used)
    assert bool((tok[1, : used[1]] == 0).all()), "a row of NaNs: every index ties, the first wins"
    e_a.close(), e_s.close()
