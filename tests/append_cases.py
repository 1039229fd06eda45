"""The cases of the appended-context sweep (tests/test_gpu_append_geometry.py on the GPU, tests/test_append_cases.py on the CPU):
ONE lram_prefill_append call -- 21 timesteps, 7 env slots of which two are held in every chunk -- on every model geometry of
tests/geometry_cases.py, on the block layouts of tests/layout_cases.py, under the switches that select another form of a
state-writing kernel, and at the env counts at which a launcher picks another instance.  The HOLD instance of a state-writing
kernel is chosen by the same launcher as the ordinary one (head count, head dim, env count, sLSTM head dim, d_state, tokens per
launch), so the geometry selects the code under test here as it does in the sweeps this file borrows its tables from.

The call: lengths 0, 21, 14, 8, 3, 1, 0 and the reset mask 1, 1, 0, 1, 0, 1, 0, after three env-steps, with one env-step behind it.
Slots 0 and 6 are held in every chunk -- slot 0 with a set reset flag, which a held env ignores; slot 6 is B - 1 with B % 4 = 3 --,
slots 1, 3, 5 restart, slots 2, 4 continue.  With more env slots, slot b takes the pattern at b % 7: the starts, and so the chunk
plan, are the same at every env count."""
import dataclasses

from lram_amd import init_state_dict, preset
from lram_amd.config import ModelSpec
from tests import geometry_cases as gc
from tests import layout_cases as lc
from tests.helpers import make_inputs

L, NPRE = 21, 3
LENGTHS = [0, 21, 14, 8, 3, 1, 0]
RESTART = [1, 1, 0, 1, 0, 1, 0]
PRE = range(L, L + NPRE)       # timestep indices of the inputs: the env-steps ahead of the call ...
BEHIND = [L + NPRE]            # ... and the one behind it
# lram_amd.engine.context_plan(L, LENGTHS, cap): the token-sequential kernels take chunks of at most 4 timesteps (12, 9, 6 and 3
# tokens per launch all occur), the chunkwise kernels a 21-timestep call whole -- chunks of 7, 6 and 5 timesteps, and behind them
# the chunks of 2 and 1 timesteps on the token-sequential kernels in the same call
PLAN_4 = [0, 4, 7, 10, 13, 16, 18, 20]
PLAN_21 = [0, 7, 13, 18, 20]
MIN_GAP = 1e-3

LAYOUTS = ["s_first", "s_last", "s_pair", "s_all", "one_m", "one_s", "m_one", "alt"]
CHUNKWISE = [c for c in gc.XLSTM_CASES if gc.XLSTM_CASES[c][1] % 128 == 0]     # the cases with a chunkwise form
SLSTM_128 = "pf1_nh2"          # the sLSTM-head-dim-128 case: d_model 256, 2 heads
# id -> (table the model comes from, its id there, env slots, env-tile boundaries the sampled slots straddle)
BIG = {
    "nh8_dh256@35": ("geometry", "nh8_dh256", 35, (16, 18, 32)),    # mLSTM cell: 64 lanes per row; 18: the boundary of two env slices
    "nh8_dh128@35": ("geometry", "nh8_dh128", 35, (16, 32)),        # ... 32 lanes per row
    "pf1_nh2@37": ("geometry", SLSTM_128, 37, (16, 32)),            # sLSTM step kernel: 16 (f16 planes) / 32 (fp32) envs per workgroup
    "mamba_48m_2b@70": ("preset", "mamba_48m", 70, (8, 32, 64)),    # the dt_rank-48 lane kernel (from 64 envs): waves of 8 envs
}
# One geometry neither table has: 4 heads with more than one channel group per front-end thread (inner / 4 = 512 groups for 256
# threads) -- the 16M's and the layouts' 4 heads take the one-group-per-thread instance of mlstm_pre_kernel
OWN = {
    "nh4_dh512": dict(backbone="xlstm", kind="MDDXLSTM", d_model=1024, n_heads=4, n_blocks=2, slstm_at=[1], state_dim=20, act_dim=4),
}
CASES = {**{c: ("geometry", c, 7, ()) for c in gc.ALL_CASES}, **{c: ("layout", c, 7, ()) for c in LAYOUTS}, **BIG,
         **{c: ("own", c, 7, ()) for c in OWN}}


def case_spec(key):
    table, cid, _, _ = CASES[key]
    if table == "geometry":
        return gc.case_spec(cid)
    if table == "layout":
        return lc.case_spec(cid)
    if table == "own":
        return ModelSpec(**OWN[cid])
    return dataclasses.replace(preset(cid), n_blocks=2)


def case_batch(key):
    return CASES[key][2]


def lengths(B):
    return [LENGTHS[b % 7] for b in range(B)]


def restart(B):
    return [RESTART[b % 7] for b in range(B)]


def sampled_slots(key):
    """The slots the oracle and the stepping engine are consulted on: all of 7; of more, the first 7, the last 7 and both sides of
    each env-tile boundary."""
    _, _, B, bounds = CASES[key]
    s = set(range(min(B, 7))) | set(range(B - 7, B))
    for k in bounds:
        s |= {k - 1, k}
    return sorted(s)


def plan_cap(key, chunk_env=None):
    """Timesteps per chunk of the case's call: 21 where the chunkwise kernels take it (mLSTM head dim a multiple of 128, unless
    LRAM_PREFILL_CHUNK=0 keeps the token-sequential ones), else 4."""
    spec = case_spec(key)
    chunkwise = spec.backbone == "xlstm" and spec.head_dim % 128 == 0 and chunk_env != "0"
    return 21 if chunkwise else 4


def case_plan(key, chunk_env=None):
    return PLAN_21 if plan_cap(key, chunk_env) == 21 else PLAN_4


def case_data(key):
    """(spec, weights, inputs): timesteps 0 .. L - 1 the contexts, PRE the env-steps ahead of the call, BEHIND the one behind."""
    seed = SEEDS[key][0]
    spec = case_spec(key)
    return spec, init_state_dict(spec, seed=seed), make_inputs(spec, case_batch(key), L + NPRE + 1, seed=700 + seed, reset_prob=0.0)


def env_refs(key, spec, sd, seq):
    """The oracle's run of every sampled slot: a restarted slot from an empty state over its own context, a continuing one with the
    env-steps ahead of it, a held one over the env-steps alone; each with the env-step behind the call."""
    from tests.context_cases import EnvRef
    n, r = lengths(case_batch(key)), restart(case_batch(key))
    return {b: EnvRef(spec, sd, seq, b, n[b], pre=() if (r[b] and n[b]) else PRE, cont=BEHIND) for b in sampled_slots(key)}


def case_gap(key, seed):
    """The oracle's smallest top-2 logit gap over every row the case compares, for the seed pair (seed, 700 + seed)."""
    spec = case_spec(key)
    sd = init_state_dict(spec, seed=seed)
    seq = make_inputs(spec, case_batch(key), L + NPRE + 1, seed=700 + seed, reset_prob=0.0)
    return min(r.min_gap for r in env_refs(key, spec, sd, seq).values())


# Seeds (weights: seed; inputs: 700 + seed), chosen on the CPU as the first seed whose smallest oracle gap over the compared rows
# (every sampled slot: the context's last timestep and the env-step behind the call) is at least 1e-3 -- five times the 2e-4 tie
# rule of helpers.assert_actions_match -- and for nothing else, with the one exception recorded at its entry (nh1_dh1024: the
# oracle's own conditioning).  Value: (seed, the measured gap).
SEEDS = {
    "nh1_dh128": (1, 5.3e-03),
    "nh2_dh128": (1, 4.5e-03),
    "nh2_dh512": (1, 5.1e-03),
    # nh1_dh1024, seed 1 (gap 2.8e-3): passed over for its conditioning, not for its gap.  With ONE head the stabiliser state m of
    # a block is one number per env, and slot 2's m of block 2 is 8.4e-3 on those weights: the fp32 oracle's own m is 5.9e-5
    # (helpers.rel_err) from its float64 evaluation, more than half the 1e-4 bar the continuing slots are held to, and three
    # engine forms land at 5.7e-5, 7.8e-5 and 1.1e-4 from the stepping engine there.  On seed 2 the fp32 oracle is within 9.3e-7
    # of float64 on every state tensor of both continuing slots (at most 5.3e-6 on every other xLSTM case of this table).
    "nh1_dh1024": (2, 1.3e-02),
    "nh1_sdh384": (1, 1.3e-02),
    "nh8_dh128": (1, 6.5e-03),
    "nh8_dh256": (1, 1.1e-02),
    "nh8_dh16": (1, 4.9e-03),
    "pf3_dh96": (1, 6.8e-03),
    "pf1_nh2": (2, 1.0e-02),   # (tried, with their gaps: (1, 0.00071))
    "m_ds4": (1, 2.2e-03),
    "m_ds8": (2, 1.5e-02),   # (tried, with their gaps: (1, 0.00037))
    "m_ds32_e3_r7": (1, 2.8e-02),
    "m_ds64_e1_r1": (2, 1.7e-03),   # (tried, with their gaps: (1, 0.00033))
    "m_ds16_di144": (1, 1.2e-02),
    "m_r128": (1, 4.0e-03),
    "m_r129": (1, 3.8e-03),
    "s_first": (1, 2.0e-03),
    "s_last": (1, 5.4e-03),
    "s_pair": (1, 2.3e-02),
    "s_all": (1, 2.4e-03),
    "one_m": (1, 1.6e-02),
    "one_s": (1, 1.8e-03),
    "m_one": (1, 1.6e-02),
    "alt": (1, 2.3e-02),
    "nh8_dh256@35": (4, 1.6e-02),   # (tried, with their gaps: (1, 0.00029), (2, 0.00039), (3, 0.00035))
    "nh8_dh128@35": (1, 9.6e-03),
    "pf1_nh2@37": (1, 6.4e-03),
    "mamba_48m_2b@70": (1, 1.4e-03),
    "nh4_dh512": (1, 6.7e-03),
}
