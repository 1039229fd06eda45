"""Shared helpers of the parity tests (oracle = checker, engine = thing under test)."""
import torch


def make_inputs(spec, B, steps, seed=1234, reset_prob=0.15, image=False):
    """Seeded trajectory inputs: obs U(-1,1) (zero beyond a random native dim, as after pad_inputs),
    rtg decreasing by 1/scale per step, reward token 0, random per-env resets."""
    g = torch.Generator().manual_seed(seed)
    seq = []
    rtg = torch.full((B,), 4.5)
    for t in range(steps):
        if image:
            obs = torch.randint(0, 256, (B, *spec.image_shape), generator=g, dtype=torch.uint8)
        else:
            obs = torch.rand(B, spec.state_dim, generator=g) * 2 - 1
            obs[:, spec.state_dim * 3 // 4:] = 0.0
        mask = (torch.rand(B, generator=g) < reset_prob).to(torch.uint8) if t > 0 else torch.ones(B, dtype=torch.uint8)
        rtg = torch.where(mask.bool(), torch.full_like(rtg, 4.5), rtg - 0.01)
        seq.append((obs, rtg.clone(), torch.zeros(B), mask))
    return seq


# Frame sizes (C, H, W) of the image front end's shape tests (tests/test_gpu_image_shapes.py, tests/test_oracle_selfchecks.py):
# (3, 64, 64) is the size every other test uses -- all four maps whole numbers of conv tiles; the others are not.
IMAGE_SHAPE_SWEEP = [(3, 84, 84), (1, 84, 84), (4, 40, 24), (3, 33, 65), (3, 17, 33), (3, 21, 21), (1, 8, 8), (3, 1, 9),
                     (3, 64, 64)]


def pooled_hw(h, w, times=3):
    """(h, w) after `times` MaxPool2d(3, stride 2, padding 1): each extent (n - 1) // 2 + 1."""
    for _ in range(times):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h, w


def assert_actions_match(a_gpu, a_ref, logits_ref, spec, discrete=False, gap_tol=2e-4, what=""):
    """Discrete actions bit-exact, continuous within 1e-4 (= identical bins, bin width 2/256).  A mismatch
    is tolerated only where the oracle's own top-2 logit gap is below `gap_tol` (a numerical tie; a NaN gap is none); the
    number of such ties is returned so tests can assert it is zero on the committed seeds."""
    a_gpu = a_gpu.detach().cpu()
    if discrete:
        bad = (a_gpu.reshape(-1).long() != a_ref.reshape(-1).long())
        lg = logits_ref.reshape(a_ref.shape[0], -1)[:, : spec.n_discrete]
        top2 = lg.topk(2, dim=-1).values
        gap = (top2[:, 0] - top2[:, 1])
    else:
        bad = (a_gpu - a_ref).abs() > 1e-4
        top2 = logits_ref.topk(2, dim=-1).values
        gap = (top2[..., 0] - top2[..., 1])
    bad = bad.reshape(gap.shape)
    real = bad & ~(gap < gap_tol)   # a NaN margin (NaN logits) is no tie
    assert not bool(real.any()), f"{what}: {int(real.sum())} action mismatches with a clear oracle margin " \
                                 f"(min gap among them {float(gap[real].min()):.3e})"
    return int(bad.sum())


def _as_double(x):
    if not torch.is_tensor(x):
        import numpy as np
        x = torch.from_numpy(np.asarray(x))
    return x.detach().cpu().double()


def rel_err(a, b):
    """max |a - b| / max |b|: one number for the whole tensor (a large element sets the scale for all)."""
    a, b = _as_double(a), _as_double(b)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def elem_rel_err(a, b, floor=1e-3):
    """Per-element relative error max_i |a_i - b_i| / (|b_i| + floor * max|b|): for state tensors whose entries span
    orders of magnitude (matrix memory C, normaliser n), where rel_err lets one large element hide relative error
    everywhere else.  The floor keeps entries that are cancellation noise (< floor * max) from dominating."""
    a, b = _as_double(a), _as_double(b)
    return float(((a - b).abs() / (b.abs() + floor * b.abs().max() + 1e-30)).max())


class Fp64Oracle:
    """The oracle evaluated in float64 on the same weights and inputs: the reference point for conditioning.  Some
    inputs are ill-conditioned for ANY fp32 evaluation of the recurrence (the mLSTM normaliser max(|q.n|, e^-m) turns
    a 1e-6 perturbation of q.k into a 1e-3 change of h when |q.n| sits next to e^-m, and 20 blocks carry it on); there
    the fp32 CPU path itself is that far from the exact result, and a fixed tolerance between two fp32 evaluations
    means nothing.  Tests then require the engine to be as close to the fp64 result as the fp32 oracle is (times a
    small factor), wherever the fp32 oracle's own distance exceeds the fixed tolerance."""

    def __init__(self, spec, sd, **kw):
        from oracle.dt_ref import OraclePolicy
        self._prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            self.ora = OraclePolicy(spec, sd, **kw)
            self.ora.sd = {k: v.detach().double().cpu() for k, v in sd.items()}
        finally:
            torch.set_default_dtype(self._prev)

    def step(self, obs, rtg, rew, mask=None, **kw):
        torch.set_default_dtype(torch.float64)
        try:
            obs = obs if obs.dtype == torch.uint8 else obs.double()
            return self.ora.step(obs, rtg.double(), rew.double(), mask, **kw)
        finally:
            torch.set_default_dtype(self._prev)


RELAXED_ROWS = {"rows": 0, "relaxed": 0}   # running count over a test (reset with relaxed_rows_reset)


def relaxed_rows_reset():
    RELAXED_ROWS["rows"] = RELAXED_ROWS["relaxed"] = 0


def relaxed_rows_fraction():
    return RELAXED_ROWS["relaxed"] / max(1, RELAXED_ROWS["rows"])


def assert_close_or_as_close_as_fp32_oracle(got, ref32, ref64, tol=2e-4, factor=8.0, cap=5e-3, what="", pooled=False):
    """|got - ref32| <= tol * scale, or -- per row of the last axis -- got is within `factor` x the fp32 oracle's own
    distance from the fp64 result AND within `cap` * scale of it in absolute terms (the escape hatch is for
    ill-conditioned rows, not for regressions: however far the fp32 oracle itself drifts, the engine may not be further
    than `cap` from the exact result).  Rows that needed the relaxed branch are counted in RELAXED_ROWS so callers can
    bound their share (`relaxed_rows_fraction`)."""
    got, ref32, ref64 = _as_double(got), _as_double(ref32), _as_double(ref64)
    scale = float(ref64.abs().max()) + 1e-12
    err_engine = (got - ref64).abs().amax(dim=-1)
    err_oracle = (ref32 - ref64).abs().amax(dim=-1)
    direct = (got - ref32).abs().amax(dim=-1)
    strict = direct <= tol * scale
    floor = err_oracle.max() if pooled else err_oracle
    relaxed = (err_engine <= torch.clamp(factor * torch.maximum(err_oracle, floor), max=cap * scale)) & ~strict
    RELAXED_ROWS["rows"] += strict.numel()
    RELAXED_ROWS["relaxed"] += int(relaxed.sum())
    ok = strict | relaxed
    assert bool(ok.all()), (f"{what}: engine vs fp32 oracle {float(direct.max() / scale):.2e}, engine vs fp64 "
                            f"{float(err_engine.max() / scale):.2e}, fp32 oracle vs fp64 {float(err_oracle.max() / scale):.2e} "
                            f"(cap {cap:.0e})")
    return float((err_engine / (err_oracle + 1e-30))[~strict].max()) if bool((~strict).any()) else 0.0


# Per-element bar on C / n of an mLSTM block after a trajectory: |err| / (|ref| + 1e-3 max|ref|); measured worst 8.9e-4 (16M, B = 12)
ELEM_STATE_TOL = 5e-3


def sampled_state(eng, spec, sample):
    """export(block, which) of the engine's state at the env slots `sample` (the sLSTM state is [4, B, D]: slots on axis 1)."""
    idx = torch.as_tensor(sample, device=eng.device)

    def export(i, w):
        t = eng.export_state_tensor(i, w)
        return t[:, idx] if (spec.backbone == "xlstm" and i in spec.slstm_at and w == 0) else t[idx]
    return export


def state_vs_oracle(export, ora_state, spec, what, tol=2e-4, rows=None):
    """Every state tensor of the sampled envs (export(block, which), see sampled_state) against the oracle's state
    (OraclePolicy.state over the same envs): rel_err < tol, and C / n of every mLSTM block per element within ELEM_STATE_TOL.
    `rows`: the env slot of each sampled env, named in the message with the env that is furthest off."""
    def check(ok, got, want, name, env_axis=0):
        if ok:
            return
        msg = f"{what}: {name}"
        if rows is not None:
            d = (_as_double(got) - _as_double(want)).abs().transpose(0, env_axis)
            msg += f" (furthest off: row {rows[int(d.reshape(d.shape[0], -1).amax(1).argmax())]})"
        raise AssertionError(msg)

    for i in range(spec.n_blocks):
        if spec.backbone == "mamba":
            for w, j, name in ((3, 0, "conv"), (0, 1, "ssm")):
                got, want = export(i, w), ora_state[i][j]
                check(rel_err(got, want) < tol, got, want, f"layer {i} {name}")
        elif i in spec.slstm_at:
            got, want = export(i, 0), ora_state[f"block_{i}"]["slstm_state"]
            check(rel_err(got, want) < tol, got, want, f"block {i} sLSTM", env_axis=1)
        else:
            ref = ora_state[f"block_{i}"]["mlstm_state"]
            for w in range(3):
                got = export(i, w)
                check(rel_err(got, ref[w]) < tol, got, ref[w], f"block {i} state {w}")
                if w < 2:
                    check(elem_rel_err(got, ref[w]) < ELEM_STATE_TOL, got, ref[w], f"block {i} state {w} per element")
        if spec.backbone == "xlstm":
            got, want = export(i, 3), ora_state[f"block_{i}"]["conv_state"][0]
            check(rel_err(got, want) < tol, got, want, f"block {i} conv")
