"""The token front-end and action-head geometries of the head sweep (tests/test_gpu_head_geometry.py on the GPU,
tests/test_head_cases.py on the CPU): state_dim, act_dim, action_channels and n_discrete away from the two front ends every other
test uses (20 / 4 / 256 / 18 and the published 204 / 8 / 256 / 18), on both backbones at their smallest useful size.  These
four numbers select code: K of the state Linear (GEMV / few-row / fp32 tile kernel), N = act_dim * n_vocab of the head GEMM
and its row pitch, the PER instance of the sampling kernel (n_vocab <= 64 / 320 / 512), the bin width of the de-tokenisation.

  dmc      the reference's dmcontrol.yaml head: 64 channels, no discrete actions (V = 64: PER 1 at its limit), K = 24 < 32
  mt_disc  the reference's mt_disc.yaml head: V = 82
  two      V = 2, N = 2, K = 4, a discrete head of one logit
  odd      V = 107, N = 321 (odd row pitch), bin width 0.02 (no power of two), K = 36
  v320     V = 320: PER 5 at its limit
  wide     V = 512: PER 8 at its limit, N = 8704, K = 1028 > 1024 (past the few-row kernel)
  over512  V = 518: sampling is refused, K = 12 (no multiple of 8)
  disc300  a discrete head over 300 logits
"""
import torch

from lram_amd.config import ModelSpec
from oracle import dt_ref

# id -> (state_dim, act_dim, action_channels, n_discrete)
CASES = {
    "dmc": (24, 6, 64, 0),
    "mt_disc": (40, 4, 64, 18),
    "two": (4, 1, 1, 1),
    "odd": (36, 3, 100, 7),
    "v320": (20, 2, 302, 18),
    "wide": (1028, 17, 495, 17),
    "over512": (12, 2, 500, 18),
    "disc300": (20, 1, 1, 300),
}
# The two row widths just past a PER class of the staged head kernels (V = 65: PER 5 at its lower edge, V = 321: PER 8 at its),
# which no case above has: for tests/test_gpu_head_one_rule.py only, so the sweeps over CASES stay what they are.
EDGE_CASES = {
    "v65": (20, 3, 47, 18),
    "v321": (20, 2, 303, 18),
}
BACKBONES = {
    "xlstm": dict(backbone="xlstm", kind="MDDXLSTM", d_model=128, n_blocks=2, slstm_at=[1]),
    "mamba": dict(backbone="mamba", kind="MDDMamba", d_model=64, n_blocks=2),
}
ALL_BATCHES = (3, 7, 40, 264, 400)   # GEMV (< 5 rows), few-row kernel, f16x2 head from 256 rows; 264 = 2 slices of 132
SOME_BATCHES = (7, 264)
STEPS = 4
RESET_PROB = 0.15
GAP = 1e-3            # rows whose ORACLE top-2 logit gap is below this are left out of the token comparison (only)
MAX_LEFT_OUT = 0.02   # ... and no run may leave out more than this share of its rows
CONTEXT_L = 9         # stored contexts: two token-sequential chunks on Mamba


def case_spec(cid, backbone, pred_token=1):
    s, a, c, d = CASES[cid] if cid in CASES else EDGE_CASES[cid]
    return ModelSpec(**BACKBONES[backbone], state_dim=s, act_dim=a, action_channels=c, n_discrete=d, pred_token=pred_token)


def batches(cid):
    return ALL_BATCHES if cid in ("dmc", "odd", "wide") else SOME_BATCHES


# (case, backbone, env slots, env slices) of the step-parity runs
STEP_RUNS = [(c, bb, B, 0) for c in CASES for bb in BACKBONES for B in batches(c)] + [("odd", bb, 264, 2) for bb in BACKBONES]


def gaps(logits, n=None):
    """Top-2 gap of every row of the oracle's logits [..., V] over its first n entries (a row of one logit has no runner-up)."""
    lg = logits if n is None else logits[..., :n]
    if lg.shape[-1] < 2:
        return torch.full(lg.shape[:-1], float("inf"))
    top2 = lg.topk(2, dim=-1).values
    return top2[..., 0] - top2[..., 1]


def oracle_steps(spec, sd, seq, discrete=False, **kw):
    """The oracle over seq: per step (actions, tokens int64, logits [B, rows, V], embedded tokens, clear rows [B, rows])."""
    ora = dt_ref.OraclePolicy(spec, sd, **kw)
    out = []
    for obs, rtg, rew, mask in seq:
        a, dbg = ora.step(obs, rtg, rew, mask, discrete=discrete, return_debug=True)
        lg = dbg["logits"]
        n = spec.n_discrete if discrete else spec.n_vocab
        tok = lg[..., :n].argmax(-1)
        out.append((a, tok, lg, dbg["tokens"], gaps(lg, n) >= GAP))
    return out


def left_out_share(steps):
    """Share of the rows of a run (oracle_steps) that the token comparison leaves out."""
    clear = torch.stack([s[4] for s in steps])
    return 1.0 - float(clear.float().mean())


# Weight seed of every step-parity run (weights init_state_dict(spec, seed), inputs make_inputs(spec, B, 4, seed=1234 + seed)) and
# the share of its rows the ORACLE's own top-2 gap leaves out, measured on the CPU (tests/test_head_cases.py recomputes the
# batch-7 ones): every one is <= 1 %, half the bound a GPU run is held to.  Key: (case, backbone, env slots).
SEEDS = {
    ("dmc", "xlstm", 3): (1, 0.0000),
    ("dmc", "xlstm", 7): (1, 0.0000),
    ("dmc", "xlstm", 40): (1, 0.0052),
    ("dmc", "xlstm", 264): (1, 0.0027),
    ("dmc", "xlstm", 400): (1, 0.0032),
    ("dmc", "mamba", 3): (1, 0.0000),
    ("dmc", "mamba", 7): (1, 0.0000),
    ("dmc", "mamba", 40): (1, 0.0010),
    ("dmc", "mamba", 264): (1, 0.0019),
    ("dmc", "mamba", 400): (1, 0.0019),
    ("mt_disc", "xlstm", 7): (1, 0.0000),
    ("mt_disc", "xlstm", 264): (1, 0.0033),
    ("mt_disc", "mamba", 7): (1, 0.0000),
    ("mt_disc", "mamba", 264): (1, 0.0009),
    ("two", "xlstm", 7): (1, 0.0000),
    ("two", "xlstm", 264): (1, 0.0000),
    ("two", "mamba", 7): (1, 0.0000),
    ("two", "mamba", 264): (1, 0.0000),
    ("odd", "xlstm", 3): (2, 0.0000),
    ("odd", "xlstm", 7): (1, 0.0000),
    ("odd", "xlstm", 40): (1, 0.0021),
    ("odd", "xlstm", 264): (1, 0.0016),
    ("odd", "xlstm", 400): (1, 0.0021),
    ("odd", "mamba", 3): (1, 0.0000),
    ("odd", "mamba", 7): (1, 0.0000),
    ("odd", "mamba", 40): (1, 0.0042),
    ("odd", "mamba", 264): (1, 0.0038),
    ("odd", "mamba", 400): (1, 0.0040),
    ("v320", "xlstm", 7): (1, 0.0000),
    ("v320", "xlstm", 264): (1, 0.0028),
    ("v320", "mamba", 7): (1, 0.0000),
    ("v320", "mamba", 264): (1, 0.0052),
    ("wide", "xlstm", 3): (1, 0.0000),
    ("wide", "xlstm", 7): (1, 0.0000),
    ("wide", "xlstm", 40): (1, 0.0033),
    ("wide", "xlstm", 264): (1, 0.0035),
    ("wide", "xlstm", 400): (1, 0.0040),
    ("wide", "mamba", 3): (1, 0.0098),
    ("wide", "mamba", 7): (1, 0.0042),
    ("wide", "mamba", 40): (1, 0.0037),
    ("wide", "mamba", 264): (1, 0.0039),
    ("wide", "mamba", 400): (1, 0.0035),
    ("over512", "xlstm", 7): (1, 0.0000),
    ("over512", "xlstm", 264): (1, 0.0038),
    ("over512", "mamba", 7): (1, 0.0000),
    ("over512", "mamba", 264): (1, 0.0038),
    ("disc300", "xlstm", 7): (1, 0.0000),
    ("disc300", "xlstm", 264): (1, 0.0000),
    ("disc300", "mamba", 7): (1, 0.0000),
    ("disc300", "mamba", 264): (1, 0.0000),
}
# ... of the Mamba repeated-forward runs on `odd` (mamba_repeat = 3), by env slots
REPEAT_SEEDS = {
    3: (1, 0.0000),
    7: (3, 0.0000),
    264: (1, 0.0041),
}
# ... and of the pred_token runs on `mt_disc` (7 env slots), by (pred_token, backbone)
PRED_SEEDS = {
    (0, "xlstm"): (1, 0.0000),
    (0, "mamba"): (1, 0.0000),
    (2, "xlstm"): (1, 0.0000),
    (2, "mamba"): (1, 0.0000),
}
