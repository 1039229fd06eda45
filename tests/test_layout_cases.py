"""CPU: the case table of the layout sweep (tests/layout_cases.py) is what it says -- every layout passes `engine_limits`, reaches
the arm of the host code it is there for, the recorded figures of every seed (the oracle's smallest top-2 gap, its distance from
the float64 evaluation in the hidden states and in C / n per element) are the ones the oracle gives now, and the weight loader produces every name lram_finalize asks for."""
import os
import re

import pytest

from lram_amd import init_state_dict, spec_from_agent_params
from lram_amd.config import engine_limits
from lram_amd.weights import check_state_dict, engine_layout, reference_layout
from tests import layout_cases as lc


@pytest.mark.parametrize("cid", lc.ALL_CASES)
def test_every_case_is_a_layout_the_engine_accepts(cid):
    spec = lc.case_spec(cid)
    assert engine_limits(spec) == []
    assert 1 <= spec.n_blocks <= lc.MAX_BLOCKS and spec.state_dim == 20 and spec.act_dim == 4
    if cid in lc.XLSTM_CASES:
        assert (spec.d_model, spec.n_heads, spec.inner, spec.head_dim, spec.d_model // spec.n_heads) == (256, 4, 512, 128, 64)
        assert spec.slstm_at == sorted(set(spec.slstm_at))
    else:
        assert spec.d_model == 64 and spec.d_state == 16


def _stretches(spec):
    """Runs of blocks of one kind, in order: [("s", 2), ("m", 1), ...]."""
    out = []
    for i in range(spec.n_blocks):
        k = "s" if i in spec.slstm_at else "m"
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return [tuple(x) for x in out]


def test_the_table_reaches_what_it_is_there_for():
    v = {c: lc.case_spec(c) for c in lc.ALL_CASES}
    m = {c: lc.mlstm_blocks(v[c]) for c in lc.XLSTM_CASES}
    assert len(lc.ALL_CASES) == 13 and set(lc.ORACLE_CASES) == set(lc.ALL_CASES) - {"deep64"}
    assert set(lc.LAZY_CASES) == set(lc.XLSTM_CASES) - {"s_all", "one_s"}
    # s_first: an sLSTM block ahead of any mLSTM block; all of its folds (no more than fold_bubbles) go ahead of the first read pass
    assert v["s_first"].slstm_at[0] == 0 and m["s_first"][0] > 0 and len(m["s_first"]) <= lc.FOLD_BUBBLES
    # s_last: the last block is an sLSTM block (post-blocks norm behind an FFN), so the last mLSTM block is not the last block
    assert v["s_last"].slstm_at == [v["s_last"].n_blocks - 1] and m["s_last"][-1] == v["s_last"].n_blocks - 2
    # s_pair: two adjacent sLSTM blocks behind an mLSTM block: no read pass follows the first stretch directly (must = 0), one
    # mLSTM block is still to fold (the first took a fold ahead of the first read pass)
    assert _stretches(v["s_pair"]) == [("m", 1), ("s", 2), ("m", 1)]
    # s_head_pair: two sLSTM stretches before any read pass
    assert _stretches(v["s_head_pair"]) == [("s", 2), ("m", 2)]
    assert v["s_ends"].slstm_at == [0, v["s_ends"].n_blocks - 1]
    # alt: every mLSTM block sits between sLSTM blocks (or an sLSTM block and the end); more mLSTM blocks than fold_bubbles
    assert _stretches(v["alt"]) == [("s", 1), ("m", 1)] * 3 and len(m["alt"]) > lc.FOLD_BUBBLES
    # m3_s: more than fold_bubbles mLSTM blocks ahead of the first sLSTM block -- the third has no fold yet when its turn comes
    assert v["m3_s"].slstm_at[0] == 3 > lc.FOLD_BUBBLES and m["m3_s"][:3] == [0, 1, 2]
    assert m["s_all"] == [] and v["s_all"].n_blocks == 3
    assert v["one_m"].n_blocks == 1 and m["one_m"] == [0] and len(m["one_m"]) < lc.FOLD_TAIL_BLOCKS
    assert v["one_s"].n_blocks == 1 and m["one_s"] == []
    assert v["deep64"].n_blocks == v["m_64"].n_blocks == lc.MAX_BLOCKS and v["m_one"].n_blocks == 1
    assert len(m["deep64"]) == 62
    # every layout is one that no test of the other files has: none is the [1] / [1, 3] / [1, 3, 5] pattern
    for c in lc.XLSTM_CASES:
        assert v[c].slstm_at not in ([1], [1, 3], [1, 3, 5]) or v[c].n_blocks == 64
    assert set(lc.STEP_SEEDS) == {(c, s) for c in lc.ORACLE_CASES for s in ("exercise", "trained_like")}
    assert set(lc.CONTEXT_SEEDS) == set(lc.ORACLE_CASES) and set(lc.DISCRETE_SEEDS) == set(lc.DISCRETE_CASES)
    assert set(lc.LAZY_SEEDS) == set(lc.LAZY_CASES) - {"deep64"}
    for table in (lc.STEP_SEEDS, lc.CONTEXT_SEEDS, lc.DISCRETE_SEEDS, lc.LAZY_SEEDS):
        for key, (seed, gap, dist, elem) in table.items():
            assert seed >= 1 and gap >= lc.GAP_MIN and dist <= lc.DIST_MAX and elem <= lc.ELEM_MAX, key


def _check(got, recorded, key):
    """The recorded figures (two significant digits) are the oracle's; the conditions hold for the figures as they are now."""
    (gap, dist, elem), (_, r_gap, r_dist, r_elem) = got, recorded
    assert abs(gap - r_gap) <= 0.06 * r_gap and abs(dist - r_dist) <= 0.06 * r_dist + 1e-8, (key, gap, dist, recorded)
    assert abs(elem - r_elem) <= 0.06 * r_elem + 1e-8, (key, elem, recorded)
    assert gap >= lc.GAP_MIN and dist <= lc.DIST_MAX and elem <= lc.ELEM_MAX, (key, gap, dist, elem)


@pytest.mark.parametrize("scheme", ["exercise", "trained_like"])
@pytest.mark.parametrize("cid", lc.ORACLE_CASES)
def test_recorded_step_figures_are_the_oracles(cid, scheme):
    rec = lc.STEP_SEEDS[(cid, scheme)]
    _check(lc.step_figures(cid, scheme, rec[0]), rec, (cid, scheme))


def test_recorded_deep64_figures_are_the_oracles():
    _check(lc.step_figures("deep64", lc.DEEP64_SCHEME, lc.DEEP64_SEED), lc.DEEP64_STEP, "deep64")
    assert lc.case_scheme("deep64") == "reference" and lc.case_scheme("alt") == "exercise"


@pytest.mark.parametrize("cid", lc.ORACLE_CASES)
def test_recorded_context_figures_are_the_oracles(cid):
    rec = lc.CONTEXT_SEEDS[cid]
    _check(lc.context_figures(cid, rec[0]), rec, cid)
    if cid in lc.DISCRETE_SEEDS:
        rec = lc.DISCRETE_SEEDS[cid]
        _check(lc.step_figures(cid, "exercise", rec[0], discrete=True), rec, (cid, "discrete"))


@pytest.mark.parametrize("cid", sorted(lc.LAZY_SEEDS))
def test_recorded_lazy_run_figures_are_the_oracles(cid):
    rec = lc.LAZY_SEEDS[cid]
    _check(lc.lazy_figures(cid, rec[0]), rec, cid)


def test_slstm_at_all_resolves_to_the_slstm_only_layout():
    ap = {"kind": "MDDXLSTM",
          "huggingface": {"hidden_size": 256, "n_layer": 3, "n_head": 4, "max_length": 50,
                          "xlstm_config": {"num_blocks": 3, "embedding_dim": 256, "slstm_at": "all",
                                           "mlstm_block": {"mlstm": {"num_heads": 4}},
                                           "slstm_block": {"slstm": {"num_heads": 4}, "feedforward": {"proj_factor": 1.3, "act_fn": "gelu"}}}},
          "model_kwargs": {"reward_condition": True, "rtg_condition": True, "action_condition": False, "shared_a_head": True,
                           "tokenize_a": True, "use_time_embds": False},
          "replay_buffer_kwargs": {"max_state_dim": 20, "max_act_dim": 4}}
    spec = spec_from_agent_params(ap)
    want = lc.case_spec("s_all")
    assert spec.slstm_at == [0, 1, 2] == want.slstm_at
    assert (spec.backbone, spec.d_model, spec.n_blocks, spec.n_heads, spec.inner, spec.ffn_dim, spec.state_dim, spec.act_dim) == \
        (want.backbone, want.d_model, want.n_blocks, want.n_heads, want.inner, want.ffn_dim, want.state_dim, want.act_dim)
    assert engine_limits(spec) == []


def _finalize_names():
    """The weight names lram_finalize requires (`need(e, ...)` in csrc/engine.hip), by where they apply:
    (top level, every block, Mamba block, sLSTM block, mLSTM block)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lram_amd", "csrc", "engine.hip")
    src = open(path).read()
    body = src[src.index("void finalize(lram_engine* e) {"):src.index("// optional image front end")]
    head, loop = body.split("for (int i = 0; i < c.n_blocks; ++i) {", 1)
    common, rest = loop.split("if (c.backbone == LRAM_BACKBONE_MAMBA) {", 1)
    mamba, rest = rest.split("} else if (c.block_is_slstm[i]) {", 1)
    slstm, mlstm = rest.split("} else {", 1)
    top = re.findall(r'need\(e, "([^"]+)"', head)
    per = [re.findall(r'need\(e, p \+ "([^"]+)"', part) for part in (common, mamba, slstm, mlstm)]
    assert len(top) == 10 and [len(p) for p in per] == [1, 8, 12, 13], (top, per)
    return top, per


@pytest.mark.parametrize("cid", lc.ALL_CASES)
def test_the_loader_produces_every_weight_name_finalize_asks_for(cid):
    """init_state_dict gives the checkpoint keys of the layout (reference_layout), and the conversion to the engine's names
    (engine_layout) gives every name lram_finalize requires: per block by the block's kind, under the block's own index."""
    spec = lc.case_spec(cid)
    sd = init_state_dict(spec, seed=1)
    assert set(sd) == set(reference_layout(spec))
    check_state_dict(spec, sd)
    have = set(engine_layout(spec, sd))
    top, (common, mamba, slstm, mlstm) = _finalize_names()
    want = set(top)
    for i in range(spec.n_blocks):
        kind = mamba if spec.backbone == "mamba" else (slstm if i in spec.slstm_at else mlstm)
        want |= {f"b{i}.{n}" for n in common + kind}
    assert want <= have, sorted(want - have)
    assert not any(k.startswith(f"b{spec.n_blocks}.") for k in have)
    # nothing of the other kind under a block's index (a name of the wrong kind would be a weight laid out for the wrong kernels)
    if spec.backbone == "xlstm":
        only_s, only_m = set(slstm) - set(mlstm), set(mlstm) - set(slstm)
        for i in range(spec.n_blocks):
            wrong = only_m if i in spec.slstm_at else only_s
            assert not ({f"b{i}.{n}" for n in wrong} & have), (cid, i)
