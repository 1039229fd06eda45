"""The block layouts and stack depths of the layout sweep (tests/test_gpu_layouts.py on the GPU, tests/test_layout_cases.py on the
CPU): where the sLSTM blocks sit in an xLSTM stack -- first, last, adjacent, alternating, behind three mLSTM blocks, everywhere,
nowhere -- and how deep the stack is, from one block to the cap of LRAM_MAX_BLOCKS = 64.  The layout selects host code (the
schedule of the lazy folds in run_xlstm_stack, the per-slot record, the chunk lanes' per-block events, the keys of
past_key_values), so one geometry serves all: d_model 256 with 4 heads gives an mLSTM head dim of 128 (lazy matrix memory, fused
scores, lean front end, chunkwise kernels) and an sLSTM head dim of 64 (token, step and GEMM forms).  state_dim 20, act_dim 4."""
from lram_amd.config import ModelSpec

MAX_BLOCKS = 64          # LRAM_MAX_BLOCKS (include/lram_hip.h)
FOLD_BUBBLES = 2         # lram_engine::fold_bubbles (csrc/engine.h): folds ahead of the first read pass with two env slices
FOLD_TAIL_BLOCKS = 2     # lram_engine::fold_tail_blocks: mLSTM blocks whose next fold runs at the end of the step


def _x(n_blocks, slstm_at):
    return dict(backbone="xlstm", kind="MDDXLSTM", d_model=256, n_heads=4, n_blocks=n_blocks, slstm_at=list(slstm_at),
                state_dim=20, act_dim=4)


def _m(n_blocks):
    return dict(backbone="mamba", kind="MDDMamba", d_model=64, n_blocks=n_blocks, state_dim=20, act_dim=4)


# id -> ModelSpec kwargs
XLSTM_CASES = {
    "s_first": _x(3, [0]),          # sLSTM ahead of any mLSTM block: both folds ahead of the first read pass
    "s_last": _x(3, [2]),           # the post-blocks norm after an FFN; the last mLSTM block is not the last block
    "s_pair": _x(4, [1, 2]),        # adjacent sLSTM blocks: nothing must fold in the first stretch
    "s_head_pair": _x(4, [0, 1]),   # two stretches before any read pass
    "s_ends": _x(4, [0, 3]),        # both ends
    "alt": _x(6, [0, 2, 4]),        # every mLSTM block between sLSTM blocks
    "m3_s": _x(5, [3]),             # three mLSTM blocks ahead of the first sLSTM block: the third folds right ahead of its read passes
    "s_all": _x(3, [0, 1, 2]),      # no mLSTM block at all
    "one_m": _x(1, []),             # first = last = only block; fewer mLSTM blocks than FOLD_TAIL_BLOCKS
    "one_s": _x(1, [0]),            # the same for sLSTM
    "deep64": _x(64, [1, 33]),      # the cap: per-block arrays, event rings, lane events
}
MAMBA_CASES = {
    "m_one": _m(1),
    "m_64": _m(64),                 # the loader's default n_layer
}
ALL_CASES = list(XLSTM_CASES) + list(MAMBA_CASES)
# deep64 and the oracle: on the `exercise` and `trained_like` weights the fp32 recurrence of 64 xLSTM blocks is ill-conditioned --
# the fp32 oracle is 5.6e-2 from its float64 evaluation on the step-parity inputs (2e-4 .. 3e-3 at 32 blocks, about 1e-5 at 10),
# and run twice over the 30-step inputs, the second time with every weight moved by one unit in the last place, it differs from
# itself by 1.4 in the actions and 2.5e-2 in C of block 63 (1.7 and 2.8e-1 on trained_like).  No bar, against the oracle or
# between two engine runs that round differently, measures an engine there, so deep64 has no place in the tables of the two
# schemes (ORACLE_CASES).  It runs on the reference's own initialisation instead (scheme "reference", the weights a training run
# starts from): fp32 to float64 6.1e-7, one unit in the last place moves the hidden states by 9.4e-7 -- and a 1 % change of ONE
# block's proj_down (block 40) still moves them by 6.4e-4, three times the hidden bar, so a wrong block shows.  Its logits are
# nearly flat on those weights (top-2 gaps of 1e-4): one seed with a gap of 1e-3 serves the step parity (DEEP64_STEP), every
# other deep64 run compares engine with engine.  m_64 is well conditioned on every scheme (1.8e-6).
DEEP64_SCHEME = "reference"
ORACLE_CASES = [c for c in ALL_CASES if c != "deep64"]
LAZY_CASES = [c for c in XLSTM_CASES if len(XLSTM_CASES[c]["slstm_at"]) < XLSTM_CASES[c]["n_blocks"]]   # (with an mLSTM block)
DISCRETE_CASES = ["s_first", "s_all", "m_one"]

STEP_STEPS, RESET_PROB = 8, 0.15
CONTEXT_B, CONTEXT_L, CONTEXT_AT = 3, 21, (5, 21)
LAZY_B, LAZY_STEPS, LAZY_PERIODS = 7, 30, (13, 3)
GAP_MIN, DIST_MAX, ELEM_MAX = 1e-3, 2e-5, 5e-3 / 3


def step_batch(cid):
    return 7 if cid in XLSTM_CASES else 5


def case_spec(cid):
    return ModelSpec(**(XLSTM_CASES[cid] if cid in XLSTM_CASES else MAMBA_CASES[cid]))


def case_scheme(cid):
    """The weight distribution of a case's runs other than the step parity on both schemes."""
    return DEEP64_SCHEME if cid == "deep64" else "exercise"


def mlstm_blocks(spec):
    return [i for i in range(spec.n_blocks) if i not in spec.slstm_at] if spec.backbone == "xlstm" else []


def oracle_figures(spec, sd, seq, discrete=False, at=None):
    """(smallest top-2 logit gap of the fp32 oracle over seq -- over the 1-based timesteps `at` where given --, largest rel_err of
    its hidden states against the float64 evaluation of the same weights and inputs, largest per-element error
    (helpers.elem_rel_err) of C and n of its mLSTM blocks against the float64 ones at the end -- and at the timesteps `at`)."""
    from oracle.dt_ref import OraclePolicy
    from tests.helpers import Fp64Oracle, elem_rel_err, rel_err
    ora, o64 = OraclePolicy(spec, sd), Fp64Oracle(spec, sd)
    gap, dist, elem = float("inf"), 0.0, 0.0
    for t, (obs, rtg, rew, mask) in enumerate(seq):
        _, dbg = ora.step(obs, rtg, rew, mask, discrete=discrete, return_debug=True)
        _, d64 = o64.step(obs, rtg, rew, mask, discrete=discrete, return_debug=True)
        dist = max(dist, rel_err(dbg["hidden"], d64["hidden"]))
        if at is not None and t + 1 not in at:
            continue
        if at is not None or t + 1 == len(seq):
            for i in mlstm_blocks(spec):
                for w in (0, 1):
                    elem = max(elem, elem_rel_err(ora.state[f"block_{i}"]["mlstm_state"][w], o64.ora.state[f"block_{i}"]["mlstm_state"][w]))
        lg = dbg["logits"]
        if discrete:
            lg = lg.reshape(obs.shape[0], -1)[:, :spec.n_discrete]
        top2 = lg.topk(2, dim=-1).values
        gap = min(gap, float((top2[..., 0] - top2[..., 1]).min()))
    return gap, dist, elem


def step_figures(cid, scheme, seed, discrete=False):
    from lram_amd import init_state_dict
    from tests.helpers import make_inputs
    spec = case_spec(cid)
    B = 7 if discrete else step_batch(cid)
    seq = make_inputs(spec, B, STEP_STEPS, seed=1234 + seed, reset_prob=RESET_PROB)
    return oracle_figures(spec, init_state_dict(spec, seed=seed, scheme=scheme), seq, discrete=discrete)


def lazy_figures(cid, seed):
    from lram_amd import init_state_dict
    from tests.helpers import make_inputs
    spec = case_spec(cid)
    seq = make_inputs(spec, LAZY_B, LAZY_STEPS, seed=1234 + seed, reset_prob=RESET_PROB)
    return oracle_figures(spec, init_state_dict(spec, seed=seed), seq)


def context_figures(cid, seed):
    from lram_amd import init_state_dict
    from tests.helpers import make_inputs
    spec = case_spec(cid)
    seq = make_inputs(spec, CONTEXT_B, CONTEXT_L, seed=300 + seed, reset_prob=0.0)
    return oracle_figures(spec, init_state_dict(spec, seed=seed), seq, at=CONTEXT_AT)


# Seeds of the step-parity runs (weights: seed; inputs: 1234 + seed; step_batch(id) envs, 8 steps, reset probability 0.15), chosen
# on the CPU as the first seed for which (a) the ORACLE's own smallest top-2 logit gap over the run is at least 1e-3 -- five
# times the tie rule of helpers.assert_actions_match, so a wrong action has no tie to hide behind -- and (b) the fp32 oracle's
# hidden states stay within 2e-5 (helpers.rel_err) of helpers.Fp64Oracle's: a tenth of the 2e-4 hidden bar, which then measures
# the engine and not the conditioning of the recurrence -- and (c) C and n of its mLSTM blocks at the end stay, per element
# (helpers.elem_rel_err), within a third of helpers.ELEM_STATE_TOL = 5e-3 of the float64 ones: two fp32 evaluations are at most the
# sum of their own errors apart, so an engine as accurate as the oracle stays inside the bar.  (m3_s / trained_like, seed 4: gap
# and distance fine, but the oracle's own C of block 2 is 5.1e-3 per element from float64 -- past the bar by itself; the
# trained_like scheme's third consecutive mLSTM block has entries that are cancellation noise.)
# Value: (seed, smallest gap, fp32-to-float64 distance of the hidden states, the same of C / n per element), as measured.
# deep64 cannot meet (b) on these two schemes (see DEEP64_SCHEME).
STEP_SEEDS = {
    ("s_first", "exercise"): (2, 3.4e-03, 4.4e-06, 1.1e-04),
    ("s_first", "trained_like"): (2, 3.0e-03, 7.8e-06, 4.1e-04),
    ("s_last", "exercise"): (1, 1.2e-03, 6.1e-06, 4.8e-05),
    ("s_last", "trained_like"): (2, 1.9e-03, 6.6e-06, 2.0e-04),
    ("s_pair", "exercise"): (3, 4.6e-03, 2.3e-06, 1.8e-04),
    ("s_pair", "trained_like"): (2, 2.5e-03, 4.9e-06, 3.6e-04),
    ("s_head_pair", "exercise"): (2, 6.3e-03, 7.0e-07, 1.1e-04),
    ("s_head_pair", "trained_like"): (2, 1.0e-03, 2.3e-06, 1.6e-04),
    ("s_ends", "exercise"): (1, 6.9e-03, 3.1e-06, 7.7e-05),
    ("s_ends", "trained_like"): (1, 2.3e-03, 1.0e-05, 2.6e-04),
    ("alt", "exercise"): (1, 1.1e-03, 1.2e-06, 2.3e-04),
    ("alt", "trained_like"): (1, 2.3e-03, 9.1e-06, 1.5e-03),
    ("m3_s", "exercise"): (1, 2.8e-03, 1.1e-05, 6.2e-04),
    ("m3_s", "trained_like"): (10, 3.9e-03, 9.8e-06, 1.4e-03),
    ("s_all", "exercise"): (5, 1.2e-03, 4.3e-07, 0.0e+00),
    ("s_all", "trained_like"): (3, 1.2e-03, 4.5e-07, 0.0e+00),
    ("one_m", "exercise"): (1, 1.5e-03, 1.3e-06, 3.6e-05),
    ("one_m", "trained_like"): (2, 2.1e-03, 4.7e-06, 8.7e-05),
    ("one_s", "exercise"): (1, 2.5e-03, 3.7e-07, 0.0e+00),
    ("one_s", "trained_like"): (2, 5.2e-03, 3.6e-07, 0.0e+00),
    ("m_one", "exercise"): (1, 2.8e-03, 2.3e-07, 0.0e+00),
    ("m_one", "trained_like"): (4, 2.3e-03, 2.3e-07, 0.0e+00),
    ("m_64", "exercise"): (2, 4.5e-03, 1.5e-06, 0.0e+00),
    ("m_64", "trained_like"): (3, 1.1e-03, 1.6e-06, 0.0e+00),
}
# the same for the discrete head (7 envs; argmax over the first n_discrete logits)
DISCRETE_SEEDS = {
    "s_first": (1, 6.3e-03, 2.8e-06, 7.7e-05),
    "s_all": (1, 6.8e-02, 4.2e-07, 0.0e+00),
    "m_one": (1, 1.0e-01, 3.1e-07, 0.0e+00),
}
# ... and for the stored contexts (3 envs, 21 timesteps without restarts, weights: seed, inputs: 300 + seed): the smallest gap at
# timesteps 5 and 21, where a prefill's actions and states are compared (the per-element figure there too), and the distance over the whole run
CONTEXT_SEEDS = {
    "s_first": (1, 3.3e-02, 8.7e-07, 8.0e-05),
    "s_last": (1, 5.0e-03, 1.2e-06, 6.6e-05),
    "s_pair": (1, 1.3e-02, 1.2e-06, 8.3e-05),
    "s_head_pair": (1, 1.3e-02, 1.1e-06, 8.2e-05),
    "s_ends": (1, 2.5e-02, 9.4e-07, 8.0e-05),
    "alt": (2, 1.1e-02, 1.5e-06, 1.1e-04),
    "m3_s": (1, 1.1e-02, 2.0e-06, 2.0e-04),
    "s_all": (2, 8.3e-02, 4.1e-07, 0.0e+00),
    "one_m": (1, 1.7e-02, 8.6e-07, 5.4e-05),
    "one_s": (3, 1.5e-02, 3.5e-07, 0.0e+00),
    "m_one": (1, 4.1e-02, 2.7e-07, 0.0e+00),
    "m_64": (1, 4.8e-03, 1.8e-06, 0.0e+00),
}
# ... and for the lazy runs (7 envs, 30 steps, reset probability 0.15, weights: seed, inputs: 1234 + seed; seeds 1 .. 60 tried)
LAZY_SEEDS = {
    "s_first": (19, 1.8e-03, 2.6e-06, 8.8e-05),
    "s_last": (1, 1.2e-03, 6.1e-06, 6.7e-05),
    "s_pair": (5, 1.7e-03, 2.7e-06, 1.8e-04),
    "s_head_pair": (15, 1.1e-03, 1.1e-05, 9.1e-05),
    "s_ends": (2, 1.6e-03, 6.3e-06, 1.3e-04),
    "alt": (28, 1.0e-03, 2.6e-06, 1.2e-04),
    "m3_s": (26, 1.2e-03, 1.1e-05, 2.0e-04),
    "one_m": (5, 1.2e-03, 1.1e-06, 8.5e-05),
}
# deep64 on DEEP64_SCHEME: the step-parity figures of its seed, by the same three conditions (seeds 1 .. 4 tried)
DEEP64_SEED = 4
DEEP64_STEP = (DEEP64_SEED, 1.5e-03, 5.7e-07, 2.0e-04)
