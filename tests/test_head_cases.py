"""CPU: the case table of the head sweep (tests/head_cases.py) is what it says -- every geometry passes `engine_limits`, reaches
the kernel paths it is there for, and the recorded share of rows the oracle's own top-2 gap leaves out is the one the oracle
gives now."""
import pytest

from lram_amd import init_state_dict
from lram_amd.config import engine_limits
from tests import head_cases as hc
from tests.helpers import make_inputs


@pytest.mark.parametrize("bb", list(hc.BACKBONES))
@pytest.mark.parametrize("cid", list(hc.CASES))
def test_every_case_is_a_geometry_the_engine_accepts(cid, bb):
    for pred in (0, 1, 2):
        spec = hc.case_spec(cid, bb, pred)
        assert engine_limits(spec) == []
        assert spec.state_dim % 4 == 0 and spec.act_dim > 0 and 0 <= spec.n_discrete <= spec.n_vocab and spec.pred_token == pred


def test_the_table_reaches_what_it_is_there_for():
    v = {c: hc.case_spec(c, "mamba") for c in hc.CASES}
    assert [v[c].n_vocab for c in ("dmc", "mt_disc", "two", "odd", "v320", "wide", "over512")] == [64, 82, 2, 107, 320, 512, 518]
    assert v["dmc"].n_discrete == 0 and v["two"].n_discrete == 1 and v["disc300"].n_discrete == 300
    assert v["odd"].act_dim * v["odd"].n_vocab == 321 and v["two"].act_dim * v["two"].n_vocab == 2
    assert v["wide"].act_dim * v["wide"].n_vocab == 8704
    assert v["dmc"].state_dim < 32 and v["wide"].state_dim > 1024 and v["over512"].state_dim % 8 != 0 and v["two"].state_dim == 4
    for c in ("odd", "wide", "over512"):   # bin widths that are no power of two: the de-tokenisation rounds twice
        assert v[c].action_channels & (v[c].action_channels - 1)
    runs = set(hc.STEP_RUNS)
    assert len(runs) == len(hc.STEP_RUNS) == 3 * 2 * 5 + 5 * 2 * 2 + 2
    assert {(c, bb, B) for c, bb, B, _ in runs} == set(hc.SEEDS)
    for key, (seed, share) in list(hc.SEEDS.items()) + list(hc.REPEAT_SEEDS.items()) + list(hc.PRED_SEEDS.items()):
        assert seed >= 1 and 0.0 <= share <= 0.01, key


@pytest.mark.parametrize("bb", list(hc.BACKBONES))
@pytest.mark.parametrize("cid", list(hc.CASES))
def test_recorded_left_out_share_is_the_oracles(cid, bb):
    """Batch 7, recomputed on the spot: the recorded share (4 decimals) and at most 1 %."""
    seed, recorded = hc.SEEDS[(cid, bb, 7)]
    spec = hc.case_spec(cid, bb)
    seq = make_inputs(spec, 7, hc.STEPS, seed=1234 + seed, reset_prob=hc.RESET_PROB)
    share = hc.left_out_share(hc.oracle_steps(spec, init_state_dict(spec, seed=seed), seq))
    assert abs(share - recorded) < 5e-5, (cid, bb, share, recorded)
    assert share <= 0.01
