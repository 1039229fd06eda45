"""CPU: the scoring entries (lram_score, lram_score_last, lram_score_tokens) are declared and bound with matching argument
counts, rollout.score_loss restates the reference's reductions (src/algos/universal_decision_transformer_sb3.py:398-434), and
the score kernel needs neither scratch memory nor a spilled register."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from lram_amd import build, engine
from lram_amd.rollout import score_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lram_hip.h")
ENTRIES = ("lram_score", "lram_score_last", "lram_score_tokens")


def _declarations():
    """name -> number of parameters, for every function the header declares (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(lram_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_header_declares_the_three_entries():
    decl = _declarations()
    for name in ENTRIES:
        assert name in decl, name
    assert decl["lram_score"] == 18 and decl["lram_score_last"] == 6 and decl["lram_score_tokens"] == 18


def test_engine_binds_them_with_matching_argument_counts():
    decl = _declarations()
    for name in ENTRIES:
        assert name in engine._SYMBOLS, name
        restype, argtypes = engine._SYMBOLS[name]
        assert len(argtypes) == decl[name], (name, len(argtypes), decl[name])
    src = open(os.path.join(ROOT, "lram_amd", "engine.py")).read()
    for name in ENTRIES:   # ... and calls each of them
        assert re.search(r"lib\.%s\(" % name, src), name
    for method in ("def score(", "def last_logp(", "def score_tokens("):
        assert method in src, method
    assert "score_kernels.hip" in build.SOURCES


def _case(seed, B=5, L=7, A=6, V=19):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, L, A, V, generator=g, dtype=torch.float64)
    tokens = torch.randint(0, V, (B, L, A), generator=g)
    valid = torch.rand(B, L, generator=g) < 0.7
    valid[0, 0] = True
    act_mask = torch.rand(B, L, A, generator=g) < 0.6
    act_mask[0, 0] = False      # a valid timestep whose action mask is all zero
    logp = torch.log_softmax(logits, -1).gather(-1, tokens.unsqueeze(-1)).squeeze(-1)
    return logits, tokens, valid, act_mask, logp


@pytest.mark.parametrize("seed", [0, 1])
def test_score_loss_reference_reduction_equals_cross_entropy_code(seed):
    logits, tokens, valid, act_mask, logp = _case(seed)
    B, L, A, V = logits.shape
    # universal_decision_transformer_sb3.py:409-434 with reduction "none", written out
    att = valid.reshape(-1)
    lg = logits.reshape(-1, A, V)[att].reshape(-1, V)
    tg = tokens.reshape(-1, A)[att].reshape(-1)
    loss = F.cross_entropy(lg, tg, reduction="none")
    m = act_mask[valid].reshape(-1, A).double()
    want = (torch.sum(loss.reshape(-1, A) * m, dim=1) / (torch.sum(m, -1) + 1e-8)).mean()
    got = score_loss(logp, valid, act_mask, reduction="reference")
    assert torch.allclose(got, want, rtol=1e-12, atol=0), (float(got), float(want))
    assert bool((m.sum(-1) == 0).any())
    # a result object, a uint8 mask and a per-env action mask go the same way
    res = engine.ScoreResult(logp=logp)
    per_env = act_mask[:, 0]
    want2 = score_loss(logp, valid, per_env.reshape(B, 1, A).expand(B, L, A), reduction="reference")
    assert torch.equal(score_loss(res, valid.to(torch.uint8), per_env, reduction="reference"), want2)


def test_score_loss_mean_reduction_is_the_plain_masked_mean():
    logits, tokens, valid, act_mask, logp = _case(2)
    keep = valid.unsqueeze(-1) & act_mask
    want = (-logp[keep]).mean()
    assert torch.allclose(score_loss(logp, valid, act_mask, reduction="mean"), want, rtol=1e-12, atol=0)
    # = the reference's reduced loss function over the unmasked entries (:422-428)
    A, V = logits.shape[2:]
    lg = logits.reshape(-1, V)[keep.reshape(-1)]
    assert torch.allclose(want, F.cross_entropy(lg, tokens.reshape(-1)[keep.reshape(-1)]), rtol=1e-12, atol=0)
    # no action mask: every dim of every valid timestep
    assert torch.allclose(score_loss(logp, valid, reduction="mean"), (-logp[valid]).mean(), rtol=1e-12, atol=0)


def test_score_loss_ignores_what_the_masks_exclude_and_refuses_misuse():
    _, _, valid, act_mask, logp = _case(3)
    poisoned = logp.clone()
    poisoned[~(valid.unsqueeze(-1) & act_mask)] = float("-inf")   # e.g. padded action dims with out-of-range targets
    for red in ("reference", "mean"):
        assert torch.equal(score_loss(poisoned, valid, act_mask, reduction=red), score_loss(logp, valid, act_mask, reduction=red))
    with pytest.raises(ValueError):
        score_loss(logp, valid, act_mask, reduction="sum")
    with pytest.raises(ValueError):
        score_loss(engine.ScoreResult(), valid)


_RESOURCES = {}


def _score_resources():
    if not _RESOURCES:   # one compile for the four instances
        from tests.test_slot_state_resources import _resources
        _RESOURCES.update(_resources("score_kernels.hip"))
    return _RESOURCES


@pytest.mark.parametrize("per", [0, 1, 5, 8])
def test_score_kernel_has_no_scratch_and_no_spills(per):
    res = _score_resources()
    hits = [k for k in res if "action_score_kernelILi%dE" % per in k]
    assert len(hits) == 1, (per, sorted(res))
    r = res[hits[0]]
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] <= 64 and r["AGPRs"] == 0, r              # eight waves per SIMD
    assert r["LDS Size [bytes/block]"] <= 4 * 64 * 4 * max(per, 1), r
