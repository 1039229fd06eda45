"""CPU: the case table of the appended-context sweep (tests/append_cases.py) is what it says -- the one call's two chunk plans are
the ones lram_amd.engine.context_plan gives at every env count of the table, every case id exists in the table it borrows its
model from and is a model the engine accepts, the shapes select the kernel instances they are there for (restated from the
launchers' own conditions), and the recorded oracle gap of the stored seeds is the one the oracle gives now."""
import pytest

from lram_amd.config import engine_limits
from lram_amd.engine import context_plan
from tests import append_cases as ac
from tests import geometry_cases as gc
from tests import layout_cases as lc


def _chunks(plan, L):
    return [b - a for a, b in zip(plan, plan[1:] + [L])]


def test_the_two_plans_of_the_call():
    assert ac.L == 21 and ac.LENGTHS == [0, 21, 14, 8, 3, 1, 0] and ac.RESTART == [1, 1, 0, 1, 0, 1, 0]
    for B in sorted({ac.case_batch(k) for k in ac.CASES}):
        n = ac.lengths(B)
        assert n[:7] == ac.LENGTHS and len(n) == B
        assert context_plan(ac.L, n, 4) == ac.PLAN_4 == [0, 4, 7, 10, 13, 16, 18, 20], B
        assert context_plan(ac.L, n, 21) == ac.PLAN_21 == [0, 7, 13, 18, 20], B
    # token-sequential: 12, 9, 6 and 3 tokens per launch; chunkwise: 21, 18 and 15 tokens, then 6 and 3 on the token-sequential kernels
    assert _chunks(ac.PLAN_4, ac.L) == [4, 3, 3, 3, 3, 2, 2, 1]
    assert _chunks(ac.PLAN_21, ac.L) == [7, 6, 5, 2, 1]
    # the held one-timestep chunk (the sLSTM step kernel and the Mamba lane kernel serve only that one) is in both
    assert ac.PLAN_4[-1] == ac.PLAN_21[-1] == ac.L - 1
    # slots 0 and 6 (and every slot b with b % 7 in (0, 6)) have no context: held in every chunk; slot 0's reset flag is set
    assert ac.LENGTHS[0] == ac.LENGTHS[6] == 0 and ac.RESTART[0] == 1 and ac.RESTART[6] == 0
    assert [b for b in range(7) if ac.LENGTHS[b] and ac.RESTART[b]] == [1, 3, 5]
    assert [b for b in range(7) if ac.LENGTHS[b] and not ac.RESTART[b]] == [2, 4]
    assert 7 % 4 == 3    # the last slot is B - 1 of a batch that is no multiple of the 4-env tile of the Mamba state update


def test_the_plans_the_other_append_tests_take_have_no_three_timestep_chunk():
    """tests/test_gpu_append.py: the 16M lengths on the token-sequential kernels (chunks of 4 and 1 timesteps), the tiny models'
    plan (4, 4, 2, 1).  Nine tokens per launch with a held env are this table's alone."""
    assert set(_chunks(context_plan(47, [47, 47, 30, 30, 9, 1], 4), 47)) == {4, 1}
    assert _chunks(context_plan(11, [11, 7, 0, 3, 1], 4), 11) == [4, 4, 2, 1]
    assert 3 in _chunks(ac.PLAN_4, ac.L)


@pytest.mark.parametrize("key", list(ac.CASES))
def test_every_case_exists_in_its_table_and_is_accepted(key):
    table, cid, B, bounds = ac.CASES[key]
    if table == "geometry":
        assert cid in gc.ALL_CASES
    elif table == "layout":
        assert cid in lc.ORACLE_CASES and cid not in ("deep64", "m_64")
    elif table == "own":
        assert cid in ac.OWN
    else:
        assert cid == "mamba_48m"
    spec = ac.case_spec(key)
    assert engine_limits(spec) == []
    assert key in ac.SEEDS and ac.SEEDS[key][0] >= 1 and ac.SEEDS[key][1] >= ac.MIN_GAP
    sample = ac.sampled_slots(key)
    assert sample == sorted(set(sample)) and 0 <= sample[0] and sample[-1] == B - 1 and set(range(7)) <= set(sample)
    for k in bounds:
        assert 0 < k < B and {k - 1, k} <= set(sample)
    # every role of the pattern is among the sampled slots
    assert {b % 7 for b in sample} == set(range(7))
    assert ac.case_plan(key) == (ac.PLAN_21 if (spec.backbone == "xlstm" and spec.head_dim % 128 == 0) else ac.PLAN_4)
    assert ac.case_plan(key, "0") == ac.PLAN_4


def test_the_table_reaches_what_it_is_there_for():
    assert len(gc.ALL_CASES) == 17 and set(gc.ALL_CASES) <= set(ac.CASES) and set(ac.SEEDS) == set(ac.CASES)
    assert ac.CHUNKWISE == ["nh1_dh128", "nh2_dh128", "nh2_dh512", "nh1_dh1024", "nh1_sdh384", "nh8_dh128", "nh8_dh256", "pf1_nh2"]
    v = {k: ac.case_spec(k) for k in ac.CASES}
    # mLSTM front ends: 1, 2 and 8 heads, and 4 heads with more than one channel group per thread (inner / 4 > 256 threads)
    assert {v[c].n_heads for c in gc.XLSTM_CASES} == {1, 2, 4, 8}
    assert v["s_first"].n_heads == 4 and v["s_first"].inner // 4 <= 256 and v["pf3_dh96"].n_heads == 4 and v["pf3_dh96"].inner // 4 <= 256
    assert v["nh4_dh512"].n_heads == 4 and v["nh4_dh512"].inner // 4 > 256 and v["nh4_dh512"].head_dim == 512
    # column workgroups per head of the chunkwise kernels (head dim / 128): 1, 2 (the 16M's), 4, 6, 8
    assert {v[c].head_dim // 128 for c in ac.CHUNKWISE} == {1, 2, 4, 6, 8}
    # mLSTM cell, launch_cell_t: 64 lanes per row from 256 (env, head, 256-column slice) items, 32 from 256 of 128 columns, else
    # 16, and 4 where the head dim is no multiple of 64
    def lanes(spec, B):
        dh, pairs = spec.head_dim, B * spec.n_heads
        if dh % 256 == 0 and pairs * (dh // 256) >= 256:
            return 64
        if dh % 128 == 0 and pairs * (dh // 128) >= 256:
            return 32
        return 16 if dh % 64 == 0 else 4
    assert lanes(v["nh8_dh256@35"], 35) == 64 and lanes(v["nh8_dh128@35"], 35) == 32
    assert lanes(v["nh8_dh256"], 7) == lanes(v["nh8_dh128"], 7) == 16 and lanes(v["pf3_dh96"], 7) == lanes(v["nh8_dh16"], 7) == 4
    # sLSTM head dims: token kernel 8 .. 256 of those it serves, step kernel 128 / 256 / 384, neither at 512 and 8
    sdh = {c: v[c].d_model // v[c].n_heads for c in gc.XLSTM_CASES}
    assert (sdh["nh2_dh512"], sdh["nh1_sdh384"], sdh["nh1_dh1024"], sdh[ac.SLSTM_128], sdh["nh8_dh256"]) == (256, 384, 512, 128, 128)
    assert ac.case_batch("pf1_nh2@37") % 16 == 5 and ac.case_batch("pf1_nh2@37") % 32 == 5       # two partial workgroups
    # Mamba: every d_state but the presets' 16 too, ragged channel groups, the lane kernel's conditions
    assert {v[c].d_state for c in gc.MAMBA_CASES} == {4, 8, 16, 32, 64}
    assert v["m_ds16_di144"].d_inner % 64 != 0 and v["m_ds32_e3_r7"].d_inner % 64 != 0
    m48 = v["mamba_48m_2b@70"]
    assert (m48.n_blocks, m48.d_state, m48.dt_rank) == (2, 16, 48) and ac.case_batch("mamba_48m_2b@70") >= 64
    assert ac.case_batch("mamba_48m_2b@70") % 8 == 6                                             # a partial 8-env wave
    # layouts: sLSTM first, last, adjacent, everywhere, the only block; one-block stacks of each kind
    assert v["s_first"].slstm_at == [0] and v["s_last"].slstm_at == [v["s_last"].n_blocks - 1] and v["s_pair"].slstm_at == [1, 2]
    assert v["s_all"].slstm_at == [0, 1, 2] and v["one_s"].slstm_at == [0] and v["one_s"].n_blocks == v["one_m"].n_blocks == 1
    assert v["m_one"].n_blocks == 1 and v["m_one"].backbone == "mamba" and v["alt"].slstm_at == [0, 2, 4]


RECOMPUTED = ["nh8_dh16", "nh1_dh1024", "nh8_dh256", "pf3_dh96", "m_ds32_e3_r7", "m_ds64_e1_r1", "s_all", "mamba_48m_2b@70"]


@pytest.mark.parametrize("key", RECOMPUTED)
def test_recorded_gap_is_the_oracles(key):
    seed, recorded = ac.SEEDS[key]
    gap = ac.case_gap(key, seed)
    assert abs(gap - recorded) <= 0.06 * recorded, (key, gap, recorded)
    assert gap >= ac.MIN_GAP


def test_a_rejected_seed_is_rejected_for_the_gap():
    """m_ds64_e1_r1, seed 1: 3.3e-4, below the rule -- the seed was passed over for the gap alone."""
    assert ac.case_gap("m_ds64_e1_r1", 1) < ac.MIN_GAP
