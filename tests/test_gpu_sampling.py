"""GPU: the sampling mode of the action head (lram_set_sampling), through the C ABI.

References: the probabilities recorded from the reference's own sample_from_logits (tests/golden/sampling_reference.npz) for
the row code, a numpy Philox4x32-10 (tests/sampling_ref.py, checked against Random123's known answers on the CPU) for the
uniforms, and -- for the step -- the engine's own logits tap fed through lram_sample_tokens with lram_sample_uniforms, so
that every token of every step is checkable although the reference's torch generator cannot be reproduced.

Bounds (set with the feature, not tuned to its output):
  * a token may differ from the inverse CDF of the recorded probabilities only where u lies within 1e-6 (cumulative
    probability) of the boundary between the two tokens, and in at most 0.2 % of the rows compared;
  * a token of probability 0 is never returned;
  * sampled frequencies over R = 200 000 draws stay within 5 * sqrt(p (1 - p) / R) + 1 / R of the recorded probabilities."""
import os

import numpy as np
import pytest
import torch

from lram_amd import init_state_dict, preset
from oracle.dt_ref import minmax_inv_tokenize
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_reference.npz")
DEV = "cuda:0"
KW = dict(temperature=0.75, top_k=10, top_p=0.5)
KW_DISCRETE = dict(temperature=0.75, top_k=5, top_p=0.5)


def _dev(x, dtype=None):
    return torch.as_tensor(x, dtype=dtype).to(DEV)


# ---- 1. the uniforms ---------------------------------------------------------------------------------------------------------
def test_uniforms_equal_numpy_philox_bit_for_bit(hip_lib):
    from lram_amd.engine import sample_uniforms
    cases = [(0, 0, 0), (20261016, 0, 1), (0x9E3779B97F4A7C15, 2 ** 32 - 8, 2 ** 32 + 5), (2 ** 64 - 1, 12345, 2 ** 63 + 17),
             (7, 2 ** 32 - 8, 2 ** 32 - 1)]
    for seed, base, draw in cases:
        got = sample_uniforms(seed, base, 16, 8, draw, device=DEV).cpu().numpy()
        want = sr.uniforms(seed, base, 16, 8, draw)
        assert got.dtype == np.float64 and np.array_equal(got, want), (seed, base, draw)
        assert (got >= 0).all() and (got < 1).all()
    whole = sample_uniforms(3, 0, 16, 4, 9, device=DEV)
    assert torch.equal(whole[:8], sample_uniforms(3, 0, 8, 4, 9, device=DEV))
    assert torch.equal(whole[8:], sample_uniforms(3, 8, 8, 4, 9, device=DEV))
    assert not torch.equal(whole, sample_uniforms(3, 0, 16, 4, 10, device=DEV))


# ---- 2. the row code against the recorded reference probabilities ----------------------------------------------------------------
def test_tokens_are_the_inverse_cdf_of_the_reference_probabilities(hip_lib):
    from lram_amd.engine import sample_tokens
    g = np.load(GOLDEN)
    rng = np.random.default_rng(20261016)
    R = 2002
    compared = near = 0
    worst = 0.0
    for c in range(len(g["n"])):
        n, t, k, p = int(g["n"][c]), float(g["temperature"][c]), int(g["top_k"][c]), float(g["top_p"][c])
        name = str(g["name"][c])
        probs = g["probs"][c, :n]
        u = np.concatenate([rng.random(R - 2), [0.0, np.nextafter(1.0, 0.0)]])
        want, cdf = sr.inverse_cdf(probs, u)
        row = _dev(g["logits"][c, :n].copy())
        got = sample_tokens(row, _dev(u), t, k, p, rows=R).cpu().numpy().astype(np.int64)
        assert ((got >= 0) & (got < n)).all(), name
        assert (probs[got] > 0).all(), f"{name}: a token of probability 0 was returned"
        compared += R
        for r in np.flatnonzero(got != want):
            lo, hi = sorted((int(got[r]), int(want[r])))
            # the CDF boundary between the two tokens: every boundary from cdf[lo] to cdf[hi - 1] must lie within 1e-6 of u
            dist = max(abs(u[r] - cdf[lo]), abs(u[r] - cdf[hi - 1]))
            worst = max(worst, dist)
            assert dist <= 1e-6, f"{name}: u = {u[r]!r} gave token {got[r]}, the reference distribution gives {want[r]} " \
                                 f"({dist:.3e} from the boundary)"
            near += 1
    print(f"sample_tokens vs reference: {compared} rows, {near} differ (all within {worst:.3e} of a CDF boundary)")
    assert near <= 0.002 * compared, (near, compared)


def test_tokens_agree_with_the_restatement_on_strided_rows_and_edge_rows(hip_lib):
    """Rows with a stride (the discrete head reads the first 18 of 274 * act_dim), the tie rule at the k-th place, non-finite
    rows (argmax rule), -inf entries."""
    from lram_amd.engine import sample_tokens
    rng = np.random.default_rng(5)
    big = (rng.standard_normal((300, 600)) * 2).astype(np.float32)
    u = rng.random(300)
    for n, kw in ((18, (0.75, 5, 0.5)), (274, (1.0, 10, 0.9)), (64, (1.0, 0, 0.3)), (65, (2.0, 3, 0.0)), (320, (1.0, 7, 0.5)),
                  (321, (1.0, 7, 0.5)), (512, (0.5, 100, 0.25)), (1, (1.0, 1, 0.5))):
        got = sample_tokens(_dev(big)[:, :n], _dev(u), *kw).cpu().numpy()
        want = sr.sample_rows(big[:, :n], u, *kw)
        assert (got != want).mean() <= 0.002, (n, kw, np.flatnonzero(got != want)[:5])
    edge = rng.standard_normal((8, 274)).astype(np.float32)
    edge[0, 5] = np.nan                      # NaN: the argmax rule (NaN is the maximum)
    edge[1, 7] = edge[1, 3] = np.inf         # +inf maximum: first index of it
    edge[2, :] = -np.inf                     # nothing has a probability: index 0
    edge[3, 10:200] = -np.inf                # -inf entries: probability 0
    edge[4, [9, 100, 200]] = 50.0            # three equal maxima, k = 2: the two lowest indices stay
    edge[5, :] = 1.25                        # flat
    edge[6, 40] = -0.0                       # -0 and +0 are one value
    edge[6, 41] = 0.0
    ue = np.array([0.3, 0.9, 0.5, 0.99, 0.75, 0.999, 0.5, 0.0])
    for kw in ((1.0, 2, 0.0), (1.0, 0, 0.5), (1.0, 0, 0.0)):
        got = sample_tokens(_dev(edge), _dev(ue), *kw).cpu().numpy()
        want = sr.sample_rows(edge, ue, *kw)
        assert np.array_equal(got, want), (kw, got, want)
    got = sample_tokens(_dev(edge), _dev(ue), 1.0, 2, 0.0).cpu().numpy()
    assert got[0] == 5 and got[1] == 3 and got[2] == 0 and got[4] == 100 and not (10 <= got[3] < 200)


# ---- 3. frequencies with the device's own uniforms ---------------------------------------------------------------------------
def test_frequencies_match_the_reference_probabilities(hip_lib):
    from lram_amd.engine import sample_tokens, sample_uniforms
    g = np.load(GOLDEN)
    c = [str(x) for x in g["name"]].index("normal_n274_s3.0_t0.75_k0_p0.5")
    n, probs = int(g["n"][c]), g["probs"][c, :274]
    R = 200_000
    for draw in (0, 1):
        u = sample_uniforms(20261016, 0, R, 1, draw, device=DEV).view(-1)
        assert np.array_equal(u[:64].cpu().numpy(), sr.uniforms(20261016, 0, 64, 1, draw)[:, 0])
        tok = sample_tokens(_dev(g["logits"][c, :n].copy()), u, 0.75, 0, 0.5, rows=R).cpu().numpy()
        freq = np.bincount(tok, minlength=n) / R
        bound = 5 * np.sqrt(probs * (1 - probs) / R) + 1 / R
        ratio = np.abs(freq - probs) / bound
        print(f"draw {draw}: worst |freq - p| / bound = {ratio.max():.3f}")
        assert not freq[probs == 0].any(), "a token of probability 0 was drawn"
        assert (ratio <= 1.0).all(), (int(ratio.argmax()), float(ratio.max()))


# ---- 4. the step ---------------------------------------------------------------------------------------------------------------
def _check_step(eng, spec, a, tok, discrete, kw, seed, base, d, what, cols=None):
    """tokens == lram_sample_tokens(logits tap of this step, lram_sample_uniforms(seed, base, ., ., d)); actions de-tokenised."""
    from lram_amd.engine import sample_tokens, sample_uniforms
    B, A, V = eng.batch, spec.act_dim, spec.n_vocab
    torch.cuda.synchronize()
    _, _, logits = eng.taps()
    u = sample_uniforms(seed, base, B, A, d, device=DEV)
    if discrete:
        want = sample_tokens(logits[:, : spec.n_discrete], u[:, 0].contiguous(), **kw)
        assert torch.equal(tok[:, 0], want), f"{what}: discrete tokens vs sample_tokens(own logits, uniforms of draw {d})"
        assert torch.equal(a[:, 0], want.float()), f"{what}: discrete actions"
        assert bool(((want >= 0) & (want < spec.n_discrete)).all())
        return want
    want = sample_tokens(logits.view(B * A, V), u.view(-1), **kw).view(B, A)
    assert bool(((tok >= 0) & (tok < V)).all()), f"{what}: token out of range"
    sel = slice(None) if cols is None else cols
    assert torch.equal(tok[:, sel], want[:, sel]), f"{what}: tokens vs sample_tokens(own logits, uniforms of draw {d})"
    assert torch.equal(a, minmax_inv_tokenize(tok.long(), spec.action_channels, spec.n_discrete)), f"{what}: actions"
    return want


def _inputs(spec, B, t, g):
    obs = torch.rand(B, spec.state_dim, generator=g, device=DEV) * 2 - 1
    rtg = torch.full((B,), 4.5 - 0.01 * t, device=DEV)
    mask = torch.ones(B, dtype=torch.uint8, device=DEV) if t == 0 else \
        ((torch.arange(B, device=DEV) % 5) == (t % 5)).to(torch.uint8)      # staggered resets
    return obs, rtg, torch.zeros(B, device=DEV), mask


STEP_CASES = [("xlstm_16m", 12), ("xlstm_16m", 512), ("mamba_48m", 12), ("mamba_48m", 1024)]


@pytest.mark.parametrize("discrete", [False, True], ids=["continuous", "discrete"])
@pytest.mark.parametrize("model,slots", STEP_CASES, ids=[f"{m}_{b}" for m, b in STEP_CASES])
def test_step_tokens_are_drawn_from_the_steps_own_logits(hip_lib, model, slots, discrete):
    from lram_amd.engine import Engine
    spec = preset(model)
    eng = Engine(spec, init_state_dict(spec, seed=0), slots, device=DEV)
    if model == "xlstm_16m":
        assert eng.state_mode == ("lazy" if slots >= 128 else "materialised")
    kw = KW_DISCRETE if discrete else KW
    seed, base = 20261016 + slots, 2 ** 32 - 8 if slots == 12 else 4096
    assert eng.sampling is None
    eng.set_sampling(seed=seed, slot_base=base, **kw)
    assert eng.sampling == dict(kw, seed=seed, slot_base=base, draws=0)
    g = torch.Generator(device=DEV).manual_seed(slots)
    off_argmax = 0
    for t in range(6):
        obs, rtg, rew, mask = _inputs(spec, slots, t, g)
        a, tok = eng.step(obs, rtg, rew, mask, discrete=discrete)
        _check_step(eng, spec, a, tok, discrete, kw, seed, base, t, f"{model} {slots} step {t}")
        _, _, logits = eng.taps()
        lg = logits.view(slots, spec.act_dim, spec.n_vocab)
        am = lg[:, 0, : spec.n_discrete].argmax(-1) if discrete else lg.argmax(-1)
        off_argmax += int(((tok[:, 0] if discrete else tok) != am).sum())
    assert eng.sampling["draws"] == 6
    assert off_argmax > 0, "every sampled token was the argmax: nothing was drawn"
    eng.close()
    torch.cuda.empty_cache()


def test_step_at_the_headline_batch(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    eng = Engine(spec, init_state_dict(spec, seed=0), 4096, device=DEV)
    eng.set_sampling(seed=1, slot_base=0, **KW)
    g = torch.Generator(device=DEV).manual_seed(4096)
    for t in range(3):
        obs, rtg, rew, mask = _inputs(spec, 4096, t, g)
        a, tok = eng.step(obs, rtg, rew, mask)
        _check_step(eng, spec, a, tok, False, KW, 1, 0, t, f"headline step {t}")
    assert eng.sampling["draws"] == 3
    eng.close()
    torch.cuda.empty_cache()


def test_step_images_and_prefill_draw_too(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    B = 6
    eng = Engine(spec, init_state_dict(spec, seed=0, with_image_encoder=True), B, device=DEV)
    eng.set_sampling(seed=9, slot_base=100, **KW)
    g = torch.Generator(device=DEV).manual_seed(3)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    rtg, rew = torch.full((B,), 4.5, device=DEV), torch.zeros(B, device=DEV)
    for t in range(2):
        frames = torch.randint(0, 256, (B, *spec.image_shape), generator=g, device=DEV, dtype=torch.uint8)
        a, tok = eng.step_images(frames, rtg, rew, ones if t == 0 else None)
        _check_step(eng, spec, a, tok, False, KW, 9, 100, t, f"step_images {t}")
    L = 7
    obs = torch.rand(B, L, spec.state_dim, generator=g, device=DEV) * 2 - 1
    seq_rtg = torch.full((B, L), 4.5, device=DEV)
    a, tok = eng.prefill(obs, seq_rtg, torch.zeros(B, L, device=DEV), reset_mask=ones)
    _check_step(eng, spec, a, tok, False, KW, 9, 100, 2, "prefill")
    eng.prefill(obs, seq_rtg, torch.zeros(B, L, device=DEV), want_action=False)   # no action: no draw
    assert eng.sampling["draws"] == 3
    eng.close()


def test_mamba_repeated_forwards_share_one_draw(hip_lib):
    """lram_set_compat_mode(4, stale): forward p writes only its own column block of the logits buffer (the last one every
    column from its own on), so after the step the tap holds, column by column, the logits each column was drawn from."""
    from lram_amd.engine import Engine
    spec = preset("mamba_48m")
    B = 12
    eng = Engine(spec, init_state_dict(spec, seed=0), B, device=DEV)
    eng.set_compat_mode(4, True)
    eng.set_sampling(seed=77, slot_base=8, **KW)
    g = torch.Generator(device=DEV).manual_seed(12)
    for t in range(4):
        obs, rtg, rew, mask = _inputs(spec, B, t, g)
        a, tok = eng.step(obs, rtg, rew, mask)
        _check_step(eng, spec, a, tok, False, KW, 77, 8, t, f"compat step {t}")   # every column
    assert eng.sampling["draws"] == 4     # once per env-step, not once per forward
    eng.close()


# ---- 5. off means off --------------------------------------------------------------------------------------------------------
def test_disarmed_equals_never_armed_and_top_k_1_is_the_argmax(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=0)
    B = 12
    runs = {}
    for name in ("never", "disarmed", "top1"):
        eng = Engine(spec, sd, B, device=DEV)
        if name == "disarmed":
            eng.set_sampling(seed=5, **KW)
            eng.set_sampling(None)
            assert eng.sampling is None
        if name == "top1":
            eng.set_sampling(temperature=1.0, top_k=1, top_p=0.0, seed=5)
        g = torch.Generator(device=DEV).manual_seed(12)
        out = []
        for t in range(6):
            obs, rtg, rew, mask = _inputs(spec, B, t, g)
            a, tok = eng.step(obs, rtg, rew, mask)
            torch.cuda.synchronize()
            out.append((a.cpu().clone(), tok.cpu().clone()))
        runs[name] = out
        eng.close()
    for t in range(6):
        for k in (0, 1):
            assert torch.equal(runs["never"][t][k].view(torch.int32), runs["disarmed"][t][k].view(torch.int32)), t
            assert torch.equal(runs["never"][t][k].view(torch.int32), runs["top1"][t][k].view(torch.int32)), t


def test_bad_settings_are_refused_with_a_text(hip_lib):
    from lram_amd.engine import Engine, LramError
    spec = preset("xlstm_tiny")
    eng = Engine(spec, init_state_dict(spec, seed=0), 2, device=DEV)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                dict(top_p=-0.01), dict(top_p=1.01), dict(top_k=-1), dict(top_k=spec.n_vocab + 1)):
        with pytest.raises(LramError, match="lram_set_sampling"):
            eng.set_sampling(**bad)
        assert eng.sampling is None
    eng.set_sampling(top_k=spec.n_discrete + 1)       # fine for the continuous head, more than the discrete head has
    obs = torch.zeros(2, spec.state_dim, device=DEV)
    z = torch.zeros(2, device=DEV)
    eng.step(obs, z, z, None)
    with pytest.raises(LramError, match="top_k"):
        eng.step(obs, z, z, None, discrete=True)
    eng.close()


# ---- 6. graph mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["xlstm_16m", "mamba_48m"])
def test_graph_replays_draw_afresh(hip_lib, model):
    from lram_amd.engine import Engine
    spec = preset(model)
    B = 8
    eng = Engine(spec, init_state_dict(spec, seed=0), B, device=DEV)
    eng.set_graph_mode(True)
    eng.set_sampling(seed=31, slot_base=16, **KW)
    g = torch.Generator(device=DEV).manual_seed(8)
    obs, rtg, rew, _ = _inputs(spec, B, 0, g)
    mask = torch.zeros(B, dtype=torch.uint8, device=DEV)
    toks = []
    for t in range(4):      # identical inputs and buffers: step 0 captures, the later ones replay
        a, tok = eng.step(obs, rtg, rew, mask)
        toks.append(_check_step(eng, spec, a, tok, False, KW, 31, 16, t, f"{model} graph step {t}").cpu())
    assert eng.sampling["draws"] == 4
    assert any(not torch.equal(toks[0], x) for x in toks[1:])
    eng.close()


# ---- 7. isolation ------------------------------------------------------------------------------------------------------------
def test_non_finite_observations_cost_their_own_slots_only(hip_lib):
    from lram_amd.engine import Engine
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=0)
    B, S = 12, [3, 8]
    runs = []
    for poisoned in (False, True):
        eng = Engine(spec, sd, B, device=DEV)
        eng.set_sampling(seed=2, slot_base=0, **KW)
        g = torch.Generator(device=DEV).manual_seed(12)
        out = []
        for t in range(6):
            obs, rtg, rew, mask = _inputs(spec, B, t, g)
            mask[S] = 1 if t == 0 else 0
            if poisoned and t == 2:
                obs[3] = float("nan")
                obs[8, 5] = float("inf")
            a, tok = eng.step(obs, rtg, rew, mask)
            _check_step(eng, spec, a, tok, False, KW, 2, 0, t, f"isolation step {t}")   # poisoned rows included: a valid index
            out.append((a.cpu().clone(), tok.cpu().clone()))
        runs.append(out)
        eng.close()
    keep = torch.ones(B, dtype=torch.bool)
    keep[S] = False
    for t in range(6):
        for k in (0, 1):
            assert torch.equal(runs[0][t][k][keep].view(torch.int32), runs[1][t][k][keep].view(torch.int32)), t
