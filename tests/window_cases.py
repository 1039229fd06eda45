"""The case machinery of the context-window tests (tests/test_gpu_window.py on the GPU, tests/test_window_api.py on the CPU):
the specs, the scripted schedule of resets, a plain-Python model of the per-env history that lram_step_window keeps on the
device (the history "kept by the test"), and the CPU oracle's run of every window.  Not a conftest: imported by name."""
import dataclasses

import numpy as np
import torch

from lram_amd import preset
from lram_amd.config import ModelSpec

# Inputs of the oracle comparison (test_gpu_window.py, test 2): the weights are OracleEngine's (init_state_dict(spec, seed=0)),
# the observations, returns-to-go and rewards come from ORACLE_SEED.  Rows left out of the token comparison because the oracle's
# own top-2 logit gap is below MIN_GAP, counted on the CPU with the oracle alone (test_window_api.py asserts <= 1 %), out of
# 15 steps x 5 envs x 4 action dims = 300 per case:
#   xlstm reference 2 / 300 (0.67 %), xlstm none 1 / 300 (0.33 %), mamba reference 1 / 300 (0.33 %), mamba none 0 / 300
ORACLE_SEED = 2024
MIN_GAP = 1e-3
LOGIT_TOL = 2e-4     # rel_err of a row's logits: the stored-context bar of tests/test_gpu_ragged.py


def spec_of(name):
    """The small two-block specs: xLSTM with one sLSTM block (head dim 64: token-sequential chunks of 4 timesteps), Mamba, and a
    chunkwise-capable xLSTM geometry (head dim 128: chunks of up to 21 timesteps)."""
    if name == "xlstm":
        return dataclasses.replace(preset("xlstm_tiny"), n_blocks=2)
    if name == "mamba":
        return preset("mamba_tiny")
    assert name == "xlstm_chunk", name
    return ModelSpec(backbone="xlstm", kind="MDDXLSTM", d_model=128, n_heads=2, n_blocks=2, slstm_at=[1], state_dim=20, act_dim=4)


def reset_schedule(B, steps):
    """reset[t][b]: env 0 never restarts, env 1 at step 1, env 2 at steps 4 and 5, env b >= 3 at steps 3 b - 2 and 3 b + 4 (env 3: 7
    and 13, env 4: 10 and 16) -- and everybody at step 0, where the windows are empty anyway."""
    at = {0: [], 1: [1], 2: [4, 5]}
    out = []
    for t in range(steps):
        out.append([t == 0 or t in at.get(b, [3 * b - 2, 3 * b + 4]) for b in range(B)])
    return out


def make_steps(B, width, steps, seed):
    """Per step: obs [B, width] U(-1, 1), rtg [B], and the reward [B] the env hands back for that step (the NEXT call's
    prev_reward)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in range(steps):
        obs = torch.rand(B, width, generator=g) * 2 - 1
        rtg = 4.5 - 0.05 * t + 0.2 * torch.rand(B, generator=g)
        rew = torch.rand(B, generator=g) - 0.3
        out.append((obs, rtg, rew))
    return out


class History:
    """The per-env history lram_step_window keeps, as plain lists of (vector, rtg, reward) oldest first: the steps of the
    header, in its order.  Arithmetic in float32 (numpy scalars), the relabel accumulated from the newest entry backwards."""

    def __init__(self, B, K):
        self.B, self.K = B, K
        self.rows = [[] for _ in range(B)]

    def step(self, vec, rtg, prev_reward, reset=None, relabel=None, keep=None):
        for b in range(self.B):
            h = self.rows[b]
            if reset is not None and reset[b]:
                h.clear()
            elif h:
                h[-1][2] = np.float32(prev_reward[b])
            m = min(int(relabel[b]), len(h)) if relabel is not None else 0
            s = np.float32(0)
            for a in range(m):
                e = h[len(h) - 1 - a]
                s = e[2] if a == 0 else np.float32(e[2] + s)
                e[1] = s
            if keep is not None and keep[b] > 0:
                del h[:max(0, len(h) - int(keep[b]))]
            h.append([vec[b].clone(), np.float32(rtg[b]), np.float32(0)])
            del h[:max(0, len(h) - self.K)]

    @property
    def counts(self):
        return [len(h) for h in self.rows]

    def tensors(self, pad_vec=None, left=False, fill=0.0):
        """[B, K, width], [B, K], [B, K]: end-aligned behind (pad_vec or `fill`, rtg `fill` or 0, reward `fill` or 0), or with
        `left` left-aligned with `fill` behind every env's rows."""
        width = self.rows[0][0][0].numel()
        vec = torch.full((self.B, self.K, width), fill)
        rtg, rew = torch.full((self.B, self.K), fill), torch.full((self.B, self.K), fill)
        if pad_vec is not None:
            vec[:], rtg[:], rew[:] = pad_vec, 0.0, 0.0
        for b, h in enumerate(self.rows):
            o = 0 if left else self.K - len(h)
            for i, (v, g, r) in enumerate(h):
                vec[b, o + i], rtg[b, o + i], rew[b, o + i] = v, float(g), float(r)
        return vec, rtg, rew


def oracle_windows(name, pad, B=5, K=6):
    """The oracle's answer to every step of the schedule: per step (logits [B, act_dim, n_vocab], tokens [B, act_dim]) from a
    fresh tests.oracle_engine.OracleEngine stepped through the windows' K call-timesteps -- every env restarted where its own
    window begins, so what it was fed ahead of that is gone.  pad: "reference" (the pad observation, rtg 0, reward 0 ahead of
    a shorter window) or "none"."""
    from tests.oracle_engine import OracleEngine
    spec = spec_of(name)
    steps = 2 * K + 3
    seq, resets = make_steps(B, spec.state_dim, steps, ORACLE_SEED), reset_schedule(B, steps)
    pad_obs = pad_observation(spec)
    hist, out = History(B, K), []
    prev = torch.zeros(B)
    for t, (obs, rtg, rew) in enumerate(seq):
        hist.step(obs, rtg, prev, reset=resets[t])
        prev = rew
        ref = pad == "reference"
        vec, g, r = hist.tensors(pad_vec=pad_obs if ref else None)
        ora = OracleEngine(spec, B, "cpu")
        for l in range(K):
            mask = torch.tensor([1 if (l == 0 if ref else l == K - n) else 0 for n in hist.counts], dtype=torch.uint8)
            _, tok = ora.step(vec[:, l], g[:, l], r[:, l], mask)
        out.append((ora.taps()[2].view(B, spec.act_dim, spec.n_vocab).clone(), tok.clone()))
    return out


def pad_observation(spec):
    """A fixed stand-in for (0 - state_mean) / state_std."""
    return torch.linspace(-0.5, 0.5, spec.state_dim)


def left_out_fraction(rows):
    """Share of (step, env, action dim) entries whose oracle top-2 logit gap is below MIN_GAP."""
    gaps = torch.cat([(lg.topk(2, dim=-1).values[..., 0] - lg.topk(2, dim=-1).values[..., 1]).reshape(-1) for lg, _ in rows])
    return float((gaps < MIN_GAP).float().mean()), int(gaps.numel())
