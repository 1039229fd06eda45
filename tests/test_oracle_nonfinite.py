"""The oracle on non-finite observations: a diverged simulation (MuJoCo suites do return NaN, Inf or huge observations) costs
its own env alone, a reset gives that env exactly the state of a fresh one (`past_key_values = None`,
src/callbacks/evaluation.py:238-251), and actions follow torch.argmax's NaN rule.  These are the properties the GPU module
tests/test_gpu_env_isolation.py checks the engine against."""
import pytest
import torch

from lram_amd import init_state_dict, preset
from oracle import dt_ref, mamba_ref, xlstm_ref
from tests.helpers import assert_actions_match, make_inputs

B, STEPS, T_POISON, T0 = 4, 8, 2, 4
POISONS = {"nan": float("nan"), "+inf": float("inf"), "3e38": 3e38}


def _flat_state(spec, state):
    """Every state tensor of the oracle, env-major [B, ...], in a fixed order."""
    if spec.backbone == "mamba":
        return [t for i in range(spec.n_blocks) for t in state[i]]
    out = []
    for i in range(spec.n_blocks):
        blk = state[f"block_{i}"]
        if "slstm_state" in blk:
            out.append(blk["slstm_state"].transpose(0, 1))
        else:
            out.extend(blk["mlstm_state"])
        out.append(blk["conv_state"][0])
    return out


def _bits_equal(a, b):
    """Bit-identical, NaN payloads and the sign of zero included."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _run(spec, sd, seq, poison=None, **kw):
    """Step the oracle over seq; env 0 takes `poison` in one observation element at T_POISON (a different element per run
    kind), and every env resets at step 0 and env 0 again at T0.  Returns per-step (actions, logits, state)."""
    ora = dt_ref.OraclePolicy(spec, sd, **kw)
    out = []
    for t, (obs, rtg, rew, mask) in enumerate(seq):
        obs, mask = obs.clone(), mask.clone()
        if t == T_POISON and poison is not None:
            obs[0, 3] = poison
        if t == T0:
            mask[0] = 1
        a, dbg = ora.step(obs, rtg, rew, mask, return_debug=True)
        out.append((a, dbg["logits"], [t.clone() for t in _flat_state(spec, ora.state)]))
    return out


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("name", ["xlstm_tiny", "mamba_tiny"])
def test_poisoned_env_recovers_bit_for_bit_after_its_reset(name, poison):
    spec = preset(name)
    sd = init_state_dict(spec, seed=5)
    seq = make_inputs(spec, B, STEPS, seed=91, reset_prob=0.0)
    clean = _run(spec, sd, seq)
    bad = _run(spec, sd, seq, POISONS[poison])
    # the poison reached env 0's recurrent state (else the test would prove nothing)
    assert not all(_bits_equal(x[:1], y[:1]) for x, y in zip(clean[T_POISON][2], bad[T_POISON][2]))
    if poison != "3e38":
        assert any(not bool(torch.isfinite(x[0]).all()) for x in bad[T0 - 1][2]), "no non-finite state before the reset"
    for t in range(STEPS):
        rows = slice(0, B) if t >= T0 else slice(1, B)   # recovery from the reset on, isolation throughout
        (a, lg, st), (a2, lg2, st2) = clean[t], bad[t]
        assert _bits_equal(a[rows], a2[rows]), f"{name} {poison} step {t}: actions"
        assert _bits_equal(lg[rows], lg2[rows]), f"{name} {poison} step {t}: logits"
        for k, (x, y) in enumerate(zip(st, st2)):
            assert _bits_equal(x[rows], y[rows]), f"{name} {poison} step {t}: state tensor {k}"


def test_mamba_stale_state_reset_clears_layer_0_only():
    """Compat mode `stale_state` (InferenceParams.reset() zeroes the offset only): after the reset layer 0 is the clean run's,
    bit for bit; layers >= 1 keep the previous episode's cache -- the poison with it."""
    spec = preset("mamba_tiny")
    sd = init_state_dict(spec, seed=5)
    seq = make_inputs(spec, B, STEPS, seed=91, reset_prob=0.0)
    clean = _run(spec, sd, seq, stale_state=True)
    bad = _run(spec, sd, seq, float("nan"), stale_state=True)
    for t in range(T0, STEPS):
        st, st2 = clean[t][2], bad[t][2]
        for layer in range(spec.n_blocks):
            for k in (2 * layer, 2 * layer + 1):   # (conv, ssm) of the layer
                if layer == 0:
                    assert _bits_equal(st[k], st2[k]), f"step {t}: layer 0 state {k}"
                else:
                    assert _bits_equal(st[k][1:], st2[k][1:]), f"step {t}: layer {layer} isolation"
                    if k % 2:   # the ssm state (the conv window shifts the poison out after d_conv tokens)
                        assert not bool(torch.isfinite(st2[k][0]).all()), f"step {t}: layer {layer} lost the stale state"


@pytest.mark.parametrize("name", ["xlstm_tiny", "mamba_tiny"])
def test_reset_state_rows_selects_zeros_over_nan_inf_and_minus_inf(name):
    """The reset is a select: NaN, +-Inf and a stabiliser m = -inf become +0; unmasked rows keep every bit."""
    spec = preset(name)
    mod = mamba_ref if spec.backbone == "mamba" else xlstm_ref
    g = torch.Generator().manual_seed(3)
    state = mod.zero_state(spec, 3)
    flat = _flat_state(spec, state)
    for k, t in enumerate(flat):
        t.copy_(torch.randn(t.shape, generator=g))
        first, last = (slice(None),) + (0,) * (t.dim() - 1), (slice(None),) + (-1,) * (t.dim() - 1)
        t[first] = (float("nan"), float("inf"), -float("inf"))[k % 3]
        t[last] = -0.0
    before = [t.clone() for t in flat]
    after = _flat_state(spec, mod.reset_state_rows(state, torch.tensor([True, False, True])))
    for x, y in zip(before, after):
        assert _bits_equal(y[0], torch.zeros_like(y[0])) and _bits_equal(y[2], torch.zeros_like(y[2]))
        assert _bits_equal(y[1], x[1])


def _spec_with_logits(n_discrete=18, channels=256, act_dim=3):
    spec = preset("xlstm_tiny")
    spec.n_discrete, spec.action_channels, spec.act_dim = n_discrete, channels, act_dim
    return spec


def _nan_rule_argmax(lg):
    """torch.argmax's rule restated: the first NaN if any, else the first index of the maximum."""
    out = []
    for row in lg.reshape(-1, lg.shape[-1]):
        nan = torch.isnan(row).nonzero()
        if len(nan):
            out.append(int(nan[0]))
        else:
            out.append(int((row == row.max()).nonzero()[0]))
    return torch.tensor(out).view(lg.shape[:-1])


def _hand_placed_logits(spec, rows):
    g = torch.Generator().manual_seed(0)
    lg = torch.randn(rows, spec.act_dim, spec.n_vocab, generator=g)
    nan, inf = float("nan"), float("inf")
    lg[0, 0, 40], lg[0, 0, 7] = nan, nan                 # two NaNs: the first one wins
    lg[0, 1, 30], lg[0, 1, 200] = inf, inf               # two +Inf: the first one wins
    lg[0, 2, :] = -inf                                   # -Inf everywhere but one
    lg[0, 2, 150] = -5.0
    lg[1, :, :] = nan                                    # all NaN: token 0
    lg[2, 0, :] = -inf                                   # all -Inf: token 0
    lg[2, 1, spec.n_discrete] = nan                      # a NaN at the first continuous token
    lg[2, 2, 100], lg[2, 2, 9] = inf, nan                # NaN beats +Inf
    lg[3, 0, 5], lg[3, 0, 60] = 1e30, 1e30               # an ordinary tie
    return lg


def test_oracle_continuous_actions_follow_the_argmax_nan_rule():
    spec = _spec_with_logits()
    lg = _hand_placed_logits(spec, 5)
    act, _ = dt_ref.actions_from_logits(spec, lg.reshape(5, -1), discrete=False)
    tok = _nan_rule_argmax(lg)
    assert torch.equal(tok, torch.argmax(lg, dim=-1))
    assert tok[0].tolist() == [7, 30, 150] and tok[1].tolist() == [0, 0, 0] and tok[2].tolist() == [0, 18, 9]
    assert int(tok[3, 0]) == 5
    want = dt_ref.minmax_inv_tokenize(tok, spec.action_channels, spec.n_discrete)
    assert _bits_equal(act, want)
    assert bool(torch.isfinite(act).all())


def test_oracle_discrete_actions_follow_the_argmax_nan_rule_within_the_discrete_prefix():
    spec = _spec_with_logits()
    lg = _hand_placed_logits(spec, 5)[:, 0]              # the discrete head reads action dim 0's logits
    lg[4, :] = torch.arange(spec.n_vocab, dtype=torch.float32)
    lg[4, spec.n_discrete] = float("nan")                # beyond the discrete prefix: never chosen
    full = torch.zeros(5, spec.act_dim * spec.n_vocab)
    full[:, : spec.n_vocab] = lg
    act, _ = dt_ref.actions_from_logits(spec, full, discrete=True)
    want = _nan_rule_argmax(lg[:, : spec.n_discrete])
    assert act.view(-1).tolist() == want.tolist() == [7, 0, 0, 5, spec.n_discrete - 1]


def test_assert_actions_match_does_not_forgive_a_nan_margin():
    spec = _spec_with_logits(act_dim=2)
    lg = torch.randn(2, 2, spec.n_vocab, generator=torch.Generator().manual_seed(1))
    lg[1, 1, 3] = float("nan")
    a_ref, _ = dt_ref.actions_from_logits(spec, lg.reshape(2, -1), discrete=False)
    assert assert_actions_match(a_ref.clone(), a_ref, lg, spec) == 0
    wrong = a_ref.clone()
    wrong[1, 1] += 0.5
    with pytest.raises(AssertionError):
        assert_actions_match(wrong, a_ref, lg, spec)
    lgd = lg[:, 0].clone()
    lgd[0, 2] = float("nan")
    full = torch.cat([lgd, torch.zeros(2, spec.n_vocab)], 1)
    d_ref, _ = dt_ref.actions_from_logits(spec, full, discrete=True)
    with pytest.raises(AssertionError):
        assert_actions_match(d_ref + 1, d_ref, full, spec, discrete=True)
