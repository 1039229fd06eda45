"""The model geometries of the geometry sweep (tests/test_gpu_geometry.py on the GPU, tests/test_config_weights.py for the
accepted-geometry boundary on the CPU): every head count `validate_config` admits, mLSTM head dims from 16 to the maximum of
1024, the three sLSTM recurrence forms, every Mamba d_state the state-update kernel serves, ragged channel groups, dt_rank
values that are no multiple of 4.  All with state_dim 20, act_dim 4; xLSTM stacks have their sLSTM block at index 1."""
from lram_amd.config import ModelSpec


def _x(d_model, n_heads=4, n_blocks=3, **kw):
    return dict(backbone="xlstm", kind="MDDXLSTM", d_model=d_model, n_heads=n_heads, n_blocks=n_blocks, slstm_at=[1],
                state_dim=20, act_dim=4, **kw)


def _m(d_model, **kw):
    return dict(backbone="mamba", kind="MDDMamba", d_model=d_model, n_blocks=2, state_dim=20, act_dim=4, **kw)


# id -> (ModelSpec kwargs, mLSTM head dim, sLSTM head dim)
XLSTM_CASES = {
    "nh1_dh128": (_x(64, 1), 128, 64),
    "nh2_dh128": (_x(128, 2), 128, 64),
    "nh2_dh512": (_x(512, 2), 512, 256),
    "nh1_dh1024": (_x(512, 1), 1024, 512),
    "nh1_sdh384": (_x(384, 1), 768, 384),
    "nh8_dh128": (_x(512, 8), 128, 64),
    "nh8_dh256": (_x(1024, 8, n_blocks=2), 256, 128),
    "nh8_dh16": (_x(64, 8), 16, 8),
    "pf3_dh96": (_x(128, mlstm_proj_factor=3.0, ffn_proj_factor=2.2), 96, 32),
    "pf1_nh2": (_x(256, 2, mlstm_proj_factor=1.0), 128, 128),
}
# id -> (ModelSpec kwargs, d_inner, d_state, dt_rank)
MAMBA_CASES = {
    "m_ds4": (_m(64, d_state=4), 128, 4, 4),
    "m_ds8": (_m(64, d_state=8), 128, 8, 4),
    "m_ds32_e3_r7": (_m(68, d_state=32, expand=3, dt_rank=7), 204, 32, 7),
    "m_ds64_e1_r1": (_m(64, d_state=64, expand=1, dt_rank=1), 64, 64, 1),
    "m_ds16_di144": (_m(72), 144, 16, 5),
    "m_r128": (_m(64, dt_rank=128), 128, 16, 128),
    "m_r129": (_m(64, dt_rank=129), 128, 16, 129),
}
ALL_CASES = list(XLSTM_CASES) + list(MAMBA_CASES)
STEP_STEPS = 8


def step_batch(cid):
    """Env slots of the step-parity runs: ragged against every kernel's env tile (4, 8, 16, 32)."""
    return 7 if cid in XLSTM_CASES else 5

BIG_CASES = {   # id -> (env slots, steps, env slices, sampled slots: first, last, both sides of the slice boundary, some inside)
    "nh8_dh128": (520, 3, 0, [0, 1, 130, 258, 259, 260, 261, 262, 400, 517, 518, 519]),
    "m_ds32_e3_r7": (130, 4, 2, [0, 1, 30, 63, 64, 65, 66, 67, 100, 127, 128, 129]),
}


def case_spec(cid):
    return ModelSpec(**(XLSTM_CASES[cid] if cid in XLSTM_CASES else MAMBA_CASES[cid])[0])


# Seeds of the step-parity runs (weights: seed; inputs: 1234 + seed), chosen on the CPU so that over the whole trajectory
# (step_batch(id) envs, 8 steps, reset probability 0.15) the ORACLE's own smallest top-2 logit gap is at least 1e-3 -- five times the 2e-4
# tie rule of helpers.assert_actions_match: a wrong action has no tie to hide behind.  Value: (seed, measured smallest gap).
STEP_SEEDS = {
    ("nh1_dh128", "exercise"): (6, 2.1e-03),
    ("nh1_dh128", "trained_like"): (6, 4.0e-03),
    ("nh2_dh128", "exercise"): (1, 3.4e-03),
    ("nh2_dh128", "trained_like"): (1, 4.0e-03),
    ("nh2_dh512", "exercise"): (1, 2.5e-03),
    ("nh2_dh512", "trained_like"): (2, 2.6e-03),
    ("nh1_dh1024", "exercise"): (1, 2.7e-03),
    ("nh1_dh1024", "trained_like"): (1, 3.3e-03),
    ("nh1_sdh384", "exercise"): (1, 2.0e-03),
    ("nh1_sdh384", "trained_like"): (1, 2.1e-03),
    ("nh8_dh128", "exercise"): (2, 1.0e-03),
    ("nh8_dh128", "trained_like"): (3, 1.6e-03),
    ("nh8_dh256", "exercise"): (2, 2.5e-03),
    ("nh8_dh256", "trained_like"): (1, 4.2e-03),
    ("nh8_dh16", "exercise"): (1, 4.4e-03),
    ("nh8_dh16", "trained_like"): (4, 1.4e-03),
    ("pf3_dh96", "exercise"): (2, 3.4e-03),
    ("pf3_dh96", "trained_like"): (1, 1.4e-03),
    ("pf1_nh2", "exercise"): (1, 1.2e-03),
    ("pf1_nh2", "trained_like"): (2, 2.9e-03),
    ("m_ds4", "exercise"): (2, 1.4e-03),
    ("m_ds4", "trained_like"): (1, 2.7e-03),
    ("m_ds8", "exercise"): (1, 4.1e-03),
    ("m_ds8", "trained_like"): (1, 1.6e-03),
    ("m_ds32_e3_r7", "exercise"): (1, 2.0e-03),
    ("m_ds32_e3_r7", "trained_like"): (1, 3.9e-03),
    ("m_ds64_e1_r1", "exercise"): (1, 6.0e-03),
    ("m_ds64_e1_r1", "trained_like"): (1, 4.1e-03),
    ("m_ds16_di144", "exercise"): (1, 1.9e-03),
    ("m_ds16_di144", "trained_like"): (1, 6.8e-03),
    ("m_r128", "exercise"): (2, 1.9e-03),
    ("m_r128", "trained_like"): (1, 3.1e-03),
    ("m_r129", "exercise"): (1, 6.7e-03),
    ("m_r129", "trained_like"): (1, 1.4e-03),
}
# the same for the discrete head (18-way argmax of the first n_discrete logits)
DISCRETE_SEEDS = {
    "nh2_dh128": (1, 9.7e-03),
    "nh8_dh256": (1, 1.2e-02),
    "m_ds32_e3_r7": (1, 1.7e-02),
}
# ... and for the two larger batches: (seed, smallest gap over the sampled slots)
BIG_SEEDS = {
    "nh8_dh128": (1, 2.2e-03),
    "m_ds32_e3_r7": (1, 5.5e-03),
}
# ... and for the stored contexts (3 envs, 21 timesteps without restarts, inputs 300 + seed): smallest gap at timesteps 5, 9 and 21,
# where a prefill's actions are compared
CONTEXT_SEEDS = {
    "nh1_dh128": (1, 8.6e-03),
    "nh2_dh128": (1, 6.3e-03),
    "nh2_dh512": (1, 9.2e-03),
    "nh1_dh1024": (1, 1.1e-02),
    "nh1_sdh384": (1, 2.6e-02),
    "nh8_dh128": (1, 5.5e-03),
    "nh8_dh256": (1, 2.8e-02),
    "nh8_dh16": (1, 1.0e-02),
    "pf3_dh96": (1, 5.9e-03),
    "pf1_nh2": (1, 4.5e-03),
    "m_ds4": (1, 2.8e-02),
    "m_ds8": (1, 6.5e-03),
    "m_ds32_e3_r7": (1, 1.4e-03),
    "m_ds64_e1_r1": (1, 2.0e-02),
    "m_ds16_di144": (1, 1.3e-02),
    "m_r128": (1, 9.5e-03),
    "m_r129": (1, 3.0e-03),
}
