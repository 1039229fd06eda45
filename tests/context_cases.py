"""The case machinery of the stored-context tests (tests/test_gpu_ragged.py: Engine.prefill / Engine.score with lengths, the
replace entries; tests/test_gpu_append.py and tests/test_gpu_append_geometry.py: the same with append=True): engines, bit-level
comparisons of exported states, [B, L, ...] inputs with NaN in every padded position, the CPU oracle's run of one env, and the
per-slot checks of an appended context.  Not a conftest: imported by name."""
import copy

import torch

from oracle import dt_ref
from tests.helpers import assert_actions_match, rel_err, sampled_state, state_vs_oracle

DEV = "cuda:0"
NAN = float("nan")


def new_engine(spec, sd, B):
    from lram_amd.engine import Engine
    return Engine(spec, sd, B, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def state_kinds(spec, blk):
    return (0, 3) if (spec.backbone == "mamba" or blk in spec.slstm_at) else (0, 1, 2, 3)


def export_state(eng, spec):
    out = [eng.export_state_tensor(blk, w).clone() for blk in range(spec.n_blocks) for w in state_kinds(spec, blk)]
    torch.cuda.synchronize()
    return out


def same_state(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(bits(x), bits(y)), f"{what}: state tensor {i} differs"


def env_slices(eng, spec, b):
    """env b's slice of every exported state tensor (the sLSTM state is [4, B, D]), on the host."""
    out = []
    for blk in range(spec.n_blocks):
        for w in state_kinds(spec, blk):
            t = eng.export_state_tensor(blk, w)
            out.append((t[:, b] if (spec.backbone == "xlstm" and blk in spec.slstm_at and w == 0) else t[b]).clone())
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def stack(seq, L, lengths=None, t0=0):
    """[B, L, ...] device tensors of the timesteps t0 .. t0 + L - 1; with lengths, NaN in every padded position."""
    obs, rtg, rew = (torch.stack([x[i] for x in seq[t0:t0 + L]], 1).contiguous() for i in range(3))
    if lengths is not None:
        for b, n in enumerate(lengths):
            obs[b, n:], rtg[b, n:], rew[b, n:] = NAN, NAN, NAN
    return obs.to(DEV), rtg.to(DEV), rew.to(DEV)


def u8_mask(flags):
    return torch.tensor(flags, dtype=torch.uint8, device=DEV)


def steps(eng, seq, ts):
    for t in ts:
        eng.step(*(x.to(DEV) for x in seq[t][:3]), None)


def min_gap(logits):
    top2 = logits.topk(2, dim=-1).values
    return float((top2[..., 0] - top2[..., 1]).min())


class EnvRef:
    """The oracle's run of ONE env from an empty state: the env-steps `pre` (timestep indices into seq), its context -- the first n
    timesteps of its row of seq -- and then the env-steps `cont`.  act / logits / state: behind the context; cont: (action, logits)
    of every step behind it, cont_state the state they leave.  min_gap: the smallest top-2 logit gap over the rows an engine is
    compared on (the context's last timestep, or the last env-step ahead of it for an env without a context, and every step
    behind)."""

    def __init__(self, spec, sd, seq, b, n, pre=(), cont=(), **oracle_kw):
        ora = dt_ref.OraclePolicy(spec, sd, **oracle_kw)
        row = lambda t: tuple(x[b:b + 1] for x in seq[t][:3])
        self.act = self.logits = None
        for t in list(pre) + list(range(n)):
            self.act, dbg = ora.step(*row(t), return_debug=True)
            self.logits = dbg["logits"]
        self.state = copy.deepcopy(ora.state)
        self.cont = []
        for t in cont:
            a, dbg = ora.step(*row(t), return_debug=True)
            self.cont.append((a, dbg["logits"]))
        self.cont_state = ora.state
        compared = ([self.logits] if n > 0 else []) + [lg for _, lg in self.cont]
        self.min_gap = min(min_gap(lg) for lg in compared) if compared else float("inf")


# ---- the checks of appended contexts (tests/test_gpu_append.py, tests/test_gpu_append_geometry.py) --------------------------------
MIN_GAP = 1e-3


def clear_margins(refs, what):
    """Before the engine is consulted: every compared row of the oracle runs has a clear winner."""
    gap = min(r.min_gap for r in refs)
    print(f"[append] {what}: smallest oracle top-2 logit gap over the compared rows {gap:.3e} (needs >= {MIN_GAP:.0e})")
    assert gap >= MIN_GAP, (what, gap)


def check_restarted(eng, spec, b, actions, ref, what):
    """env b against its oracle run from an empty state: the action (no tie tolerated), every state tensor, block 0's conv state."""
    if actions is not None:
        assert assert_actions_match(actions[b:b + 1], ref.act, ref.logits, spec, what=f"{what} env {b}") == 0
    export = sampled_state(eng, spec, [b])
    state_vs_oracle(export, ref.state, spec, f"{what} env {b}", rows=[b])
    conv = ref.state[0][0] if spec.backbone == "mamba" else ref.state["block_0"]["conv_state"][0]
    err = rel_err(export(0, 3), conv)
    print(f"[append] {what} env {b}: block 0 conv state rel_err {err:.2e} (bar 1e-5)")
    assert err < 1e-5, (what, b, err)


def check_continued(eng, spec, b, actions, ref, snap, what):
    """env b, which continued its state: the action against the oracle, the state against the stepping engine's snapshot."""
    if actions is not None:
        assert assert_actions_match(actions[b:b + 1], ref.act, ref.logits, spec, what=f"{what} env {b}") == 0
    slices, record = snap
    worst = 0.0
    for i, (got, want) in enumerate(zip(env_slices(eng, spec, b), slices)):
        err = rel_err(got, want)
        worst = max(worst, err)
        assert err < 1e-4, (what, b, i, err)
    rec = rel_err(eng.save_slots([b]).cpu(), record)
    print(f"[append] {what} env {b}: state against the stepping engine, worst tensor rel_err {worst:.2e}, record {rec:.2e} (bar 1e-4)")
    assert rec < 1e-4, (what, b, rec)


def stepping_snapshots(spec, sd, B, seq, pre, lengths, restart, L, only=None):
    """A second engine takes the env-steps `pre`, then timesteps 0 .. L - 1 one lram_step at a time (the restart flags on timestep
    0); env b's state -- every exported tensor and its save_slots record -- is taken right after its own last step (of the envs
    `only`, where given)."""
    eng = new_engine(spec, sd, B)
    steps(eng, seq, pre)
    snaps = {}
    for t in range(max(lengths)):
        eng.step(*(x.to(DEV) for x in seq[t][:3]), u8_mask(restart) if t == 0 else None)
        for b, n in enumerate(lengths):
            if n == t + 1 and (only is None or b in only):
                snaps[b] = (env_slices(eng, spec, b), eng.save_slots([b]).cpu())
    eng.close()
    return snaps
