"""GPU: context-window inference -- Engine.alloc_window / set_window_pad / step_window / window (lram_window_alloc,
lram_window_set_pad, lram_step_window, lram_window_peek): the reference's cache-off evaluation on a device ring.

Bars (none tuned to the code under test):
  * against the entries it rides on -- Engine.prefill over the history the test keeps in torch (tests/window_cases.History), every
    env reset: actions, tokens and the logits tap bit for bit, after every step;
  * against the CPU oracle run over every window: tokens equal wherever the oracle's top-2 logit gap is at least 1e-3, a row's
    logits within rel_err 2e-4 (the stored-context bar of tests/test_gpu_ragged.py);
  * bookkeeping through window(): the relabel exact against a float32 numpy loop in the stated order and within 1e-5 relative of
    float64, everything else exact;
  * a refused call leaves window() and every exported state tensor bit for bit what they were."""
import dataclasses

import numpy as np
import pytest
import torch

from lram_amd import init_state_dict
from lram_amd.engine import LramError
from tests import window_cases as wc
from tests.context_cases import DEV, NAN, bits, export_state, new_engine, same_state
from tests.helpers import assert_actions_match, rel_err

pytestmark = pytest.mark.gpu


def _dev(*ts):
    return tuple(t.to(DEV).contiguous() for t in ts)


def _ones(B):
    return torch.ones(B, dtype=torch.uint8, device=DEV)


def _logits(eng):
    lg = eng.taps()[2].clone()
    torch.cuda.synchronize()
    return lg


# ---- 1. bit identity with the entries it rides on --------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", ["reference", "none"])
@pytest.mark.parametrize("name,B,K", [("xlstm", 5, 6), ("mamba", 5, 6), ("xlstm_chunk", 3, 23)])
def test_window_step_is_bit_identical_to_prefill_over_the_history(hip_lib, name, B, K, pad):
    """2 K + 3 steps (the ring wraps), staggered resets, embeddings as observations, rewards patched in one step late.  K = 6: two
    token-sequential chunks (4 + 2); K = 23 on the head-dim-128 geometry: chunkwise chunks of 12 and 11."""
    spec = wc.spec_of(name)
    sd = init_state_dict(spec, seed=3)
    steps = 2 * K + 3
    seq, resets = wc.make_steps(B, spec.d_model, steps, seed=11), wc.reset_schedule(B, steps)
    pad_vec = torch.linspace(-1.0, 1.0, spec.d_model)
    eng, ref = new_engine(spec, sd, B), new_engine(spec, sd, B)
    eng.alloc_window(K)
    eng.set_window_pad(pad_vec.to(DEV), is_embedding=True)
    hist, prev = wc.History(B, K), torch.zeros(B)
    for t, (obs, rtg, rew) in enumerate(seq):
        act, tok = eng.step_window(*_dev(obs, rtg, prev), reset=resets[t], pad=pad, obs_is_embedding=True)
        got = (act.clone(), tok.clone(), _logits(eng))
        hist.step(obs, rtg, prev, reset=resets[t])
        prev = rew
        if pad == "reference":
            a, k = ref.prefill(*_dev(*hist.tensors(pad_vec=pad_vec)), reset_mask=_ones(B), obs_is_embedding=True)
        else:
            a, k = ref.prefill(*_dev(*hist.tensors(left=True, fill=NAN)), reset_mask=_ones(B), obs_is_embedding=True,
                               lengths=hist.counts)
        want = (a.clone(), k.clone(), _logits(ref))
        assert eng.window().counts == hist.counts, t
        for i, what in enumerate(("actions", "tokens", "logits")):
            assert torch.equal(bits(got[i]), bits(want[i])), f"{name} K={K} pad={pad} step {t}: {what} differ"
        assert bool(got[0].isfinite().all()) and bool((got[1] >= 0).all())
    same_state(export_state(eng, spec), export_state(ref, spec), f"{name} K={K} pad={pad}: state behind the last step")
    eng.close(), ref.close()


# ---- 2. the CPU oracle over every window -----------------------------------------------------------------------------------------
_ORACLE = {}


@pytest.mark.parametrize("pad", ["reference", "none"])
@pytest.mark.parametrize("name", ["xlstm", "mamba"])
def test_window_step_matches_the_oracle_run_over_every_window(hip_lib, name, pad):
    from tests.oracle_engine import OracleEngine
    B, K = 5, 6
    spec = wc.spec_of(name)
    if (name, pad) not in _ORACLE:
        _ORACLE[name, pad] = wc.oracle_windows(name, pad, B, K)
    rows = _ORACLE[name, pad]
    frac, n = wc.left_out_fraction(rows)
    print(f"[window] {name} pad={pad}: {frac * n:.0f} of {n} oracle rows have a top-2 gap below {wc.MIN_GAP:.0e}")
    assert frac <= 0.01
    steps = 2 * K + 3
    seq, resets = wc.make_steps(B, spec.state_dim, steps, wc.ORACLE_SEED), wc.reset_schedule(B, steps)
    eng = new_engine(spec, OracleEngine(spec, 1, "cpu").sd, B)
    eng.alloc_window(K)
    eng.set_window_pad(wc.pad_observation(spec).to(DEV))
    prev, worst = torch.zeros(B), 0.0
    for t, (obs, rtg, rew) in enumerate(seq):
        _, tok = eng.step_window(*_dev(obs, rtg, prev), reset=resets[t], pad=pad)
        tok, lg = tok.cpu(), _logits(eng).view(B, spec.act_dim, spec.n_vocab).cpu()
        prev = rew
        lg_ref, tok_ref = rows[t]
        top2 = lg_ref.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) >= wc.MIN_GAP
        assert torch.equal(tok[clear].long(), tok_ref[clear].long()), f"{name} pad={pad} step {t}: tokens differ at a clear margin"
        for b in range(B):
            err = rel_err(lg[b], lg_ref[b])
            worst = max(worst, err)
            assert err < wc.LOGIT_TOL, (name, pad, t, b, err)
    print(f"[window] {name} pad={pad}: worst logits rel_err {worst:.2e} (bar {wc.LOGIT_TOL:.0e})")
    eng.close()


# ---- 3. bookkeeping through window() ---------------------------------------------------------------------------------------------
def _same_window(eng, hist, what):
    w = eng.window()
    torch.cuda.synchronize()
    vec, rtg, rew = hist.tensors()
    assert w.counts == hist.counts, what
    for got, want, n in ((w.emb, vec, "emb"), (w.rtg, rtg, "rtg"), (w.reward, rew, "reward")):
        assert torch.equal(bits(got.cpu()), bits(want)), f"{what}: {n} differs"
    return w


def test_reward_patch_relabel_keep_and_wrap_through_window(hip_lib):
    """One scripted run on 6 envs, K = 5: episodes of 3, 7 (longer than K) and 4 steps; at every episode end a relabel of the
    episode length (7 > n_b = 5: clipped) and per env a different keep -- none, smaller than, equal to and larger than n_b."""
    spec = wc.spec_of("xlstm")
    sd = init_state_dict(spec, seed=3)
    B, K = 6, 5
    eng = new_engine(spec, sd, B)
    eng.alloc_window(K)
    seq = wc.make_steps(B, spec.d_model, 16, seed=5)
    hist, prev = wc.History(B, K), torch.zeros(B)
    ends = {3: 3, 10: 7, 14: 4}     # step at which an episode of that length has just ended
    for t, (obs, rtg, rew) in enumerate(seq):
        relabel = keep = None
        if t in ends:
            n = hist.counts
            relabel = [ends[t]] * B
            keep = [0, max(1, n[1] - 2), n[2], n[3] + 3, 1, K][:B]
            before = [[(float(e[1]), float(e[2])) for e in h] for h in hist.rows]
        eng.step_window(*_dev(obs, rtg, prev), relabel=relabel, keep=keep, pad="none", obs_is_embedding=True)
        hist.step(obs, rtg, prev, relabel=relabel, keep=keep)
        w = _same_window(eng, hist, f"step {t}")
        if t in ends:   # every env's relabelled rtg, as window() shows it, against float64 suffix sums of the patched rewards
            got_all = w.rtg.cpu().double().numpy()
            for b in range(B):
                r = np.array([x[1] for x in before[b]], dtype=np.float64)
                r[-1] = float(prev[b])
                m = min(ends[t], len(r), w.counts[b] - 1)     # (keep and the push may have dropped the older relabelled entries)
                want = np.cumsum(r[::-1])[::-1][len(r) - m:]
                got = got_all[b, K - 1 - m:K - 1]               # (end-aligned: the last row is the entry just pushed)
                assert got.shape == want.shape and np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), (t, b, got, want)
        prev = rew
    assert max(hist.counts) == K
    eng.close()


def test_raw_observations_at_600_slots_land_in_the_ring_at_its_pitch(hip_lib):
    """The raw-observation push runs the state Linear straight into the ring, one row every K * d_model floats.  At 600 env slots
    (no multiple of a GEMM tile) the dispatcher takes its many-row kernels, which the 3 - 5 slot cases never reach.  K = 3, 5 steps:
    every ring position is written, and rewritten after the wrap.  After every step the window's embeddings equal the fp64
    Linear of the stored observations (rel_err 1e-5: one projection away from the inputs, the bar tests/test_gpu_ragged.py holds
    block 0's conv state to), rtg and reward rows are exact, and a second engine that is handed the first one's newest
    embeddings through the embedding push produces the same actions, tokens and logits bit for bit."""
    spec = wc.spec_of("xlstm")
    sd = init_state_dict(spec, seed=3)
    B, K = 600, 3
    W, bias = sd["embed_state.weight"].double(), sd["embed_state.bias"].double()
    eng, twin = new_engine(spec, sd, B), new_engine(spec, sd, B)
    for e in (eng, twin):
        e.alloc_window(K)
    seq = wc.make_steps(B, spec.state_dim, 5, seed=8)
    hist, prev = wc.History(B, K), torch.zeros(B)
    for t, (obs, rtg, rew) in enumerate(seq):
        reset = [t == 0 or (t == 3 and b % 7 == 0) for b in range(B)]
        act, tok = eng.step_window(*_dev(obs, rtg, prev), reset=reset, pad="none")
        got = (act.clone(), tok.clone(), _logits(eng))
        w = eng.window()
        hist.step(obs, rtg, prev, reset=reset)
        vec, g, r = hist.tensors()
        assert w.counts == hist.counts, t
        assert torch.equal(bits(w.rtg.cpu()), bits(g)) and torch.equal(bits(w.reward.cpu()), bits(r)), t
        want = vec.double() @ W.T + bias
        for b, n in enumerate(hist.counts):
            want[b, :K - n] = 0.0
        err = rel_err(w.emb.cpu(), want)
        assert err < 1e-5, (t, err)
        a2, k2 = twin.step_window(w.emb[:, -1].contiguous(), *_dev(rtg, prev), reset=reset, pad="none", obs_is_embedding=True)
        for i, (x, y) in enumerate(zip(got, (a2.clone(), k2.clone(), _logits(twin)))):
            assert torch.equal(bits(x), bits(y)), (t, i)
        prev = rew
    print(f"[window] raw observations at {B} slots: last embeddings rel_err {err:.2e} (bar 1e-5)")
    eng.close(), twin.close()


@pytest.mark.parametrize("name", ["xlstm", "mamba"])
def test_nan_beyond_the_counts_reaches_no_output(hip_lib, name):
    """A ring full of NaN entries, then a reset: every entry beyond n_b = 1 is NaN (embedding, rtg and reward).  Neither pad mode
    lets one through: outputs equal those of an engine whose ring never held a NaN, bit for bit, and window() shows zeros."""
    spec = wc.spec_of(name)
    sd = init_state_dict(spec, seed=3)
    B, K = 3, 4
    obs, rtg, rew = wc.make_steps(B, spec.d_model, 1, seed=9)[0]
    pad_vec = torch.linspace(-1.0, 1.0, spec.d_model)
    nan = torch.full((B, spec.d_model), NAN)
    for pad in ("reference", "none"):
        out = []
        for poison in (True, False):
            eng = new_engine(spec, sd, B)
            eng.alloc_window(K)
            eng.set_window_pad(pad_vec.to(DEV), is_embedding=True)
            for _ in range(K + 1 if poison else 0):
                eng.step_window(*_dev(nan, nan[:, 0], nan[:, 0]), pad=pad, obs_is_embedding=True)
            act, tok = eng.step_window(*_dev(obs, rtg, nan[:, 0]), reset=[True] * B, pad=pad, obs_is_embedding=True)
            w = eng.window()
            out.append((act.clone(), tok.clone(), _logits(eng), w.emb, w.rtg, w.reward))
            assert w.counts == [1] * B
            assert all(bool(x.isfinite().all()) for x in out[-1][:1] + out[-1][2:]), (name, pad, poison)
            assert float(w.emb[:, :K - 1].abs().max()) == 0.0 and float(w.rtg[:, :K - 1].abs().max()) == 0.0
            eng.close()
        for x, y in zip(*out):
            assert torch.equal(bits(x), bits(y)), (name, pad)


# ---- 4. sampling armed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", ["reference", "none"])
def test_sampling_draws_once_per_window_step_and_as_prefill(hip_lib, pad):
    spec = wc.spec_of("xlstm")
    sd = init_state_dict(spec, seed=3)
    B, K = 4, 6
    seq = wc.make_steps(B, spec.d_model, 4, seed=21)
    pad_vec = torch.linspace(-1.0, 1.0, spec.d_model)
    eng, ref = new_engine(spec, sd, B), new_engine(spec, sd, B)
    for e in (eng, ref):
        e.set_sampling(temperature=1.3, top_k=0, top_p=0.0, seed=7)
    eng.alloc_window(K)
    eng.set_window_pad(pad_vec.to(DEV), is_embedding=True)
    hist, prev = wc.History(B, K), torch.zeros(B)
    for t, (obs, rtg, rew) in enumerate(seq):
        _, tok = eng.step_window(*_dev(obs, rtg, prev), reset=[t == 0, False, t == 2, False], pad=pad, obs_is_embedding=True)
        hist.step(obs, rtg, prev, reset=[t == 0, False, t == 2, False])
        prev = rew
        if pad == "reference":
            _, k = ref.prefill(*_dev(*hist.tensors(pad_vec=pad_vec)), reset_mask=_ones(B), obs_is_embedding=True)
        else:
            _, k = ref.prefill(*_dev(*hist.tensors(left=True)), reset_mask=_ones(B), obs_is_embedding=True, lengths=hist.counts)
        torch.cuda.synchronize()
        assert torch.equal(tok, k), (pad, t)
        assert eng.sampling["draws"] == ref.sampling["draws"] == t + 1
    eng.close(), ref.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def _refused(eng, spec, call, needle):
    w0 = eng.window()
    s0 = export_state(eng, spec)
    snap = [x.clone() for x in (w0.emb, w0.rtg, w0.reward)]
    with pytest.raises(LramError, match=needle):
        call()
    w1 = eng.window()
    assert w1.counts == w0.counts, needle
    for x, y in zip(snap, (w1.emb, w1.rtg, w1.reward)):
        assert torch.equal(bits(x), bits(y)), needle
    same_state(s0, export_state(eng, spec), f"refused ({needle})")


@pytest.mark.parametrize("name", ["xlstm", "mamba"])
def test_every_refusal_leaves_ring_and_state_alone(hip_lib, name):
    import ctypes
    from lram_amd.engine import _ptr, _stream_ptr
    spec = wc.spec_of(name)
    sd = init_state_dict(spec, seed=3)
    B, K = 4, 3
    eng = new_engine(spec, sd, B)
    obs, rtg, rew = _dev(*wc.make_steps(B, spec.d_model, 1, seed=2)[0])
    step = lambda **kw: eng.step_window(obs, rtg, rew, obs_is_embedding=True, **kw)
    with pytest.raises(LramError, match="no window ring"):     # (nothing to compare a ring with yet)
        step(pad="none")
    with pytest.raises(LramError, match="no window ring"):
        eng.set_window_pad(torch.zeros(spec.d_model, device=DEV), is_embedding=True)
    eng.alloc_window(K)
    step(pad="none"), step(pad="none")
    _refused(eng, spec, lambda: step(pad="reference"), "lram_window_set_pad")
    eng.set_window_pad(torch.zeros(spec.d_model, device=DEV), is_embedding=True)

    def raw(pad_mode=1, reset=None, relabel=None, keep=None, discrete=0, actions=eng._actions):
        i32 = lambda v: None if v is None else (ctypes.c_int32 * B)(*v)
        rc = eng.lib.lram_step_window(eng._h, _ptr(obs), 1, _ptr(rtg), _ptr(rew), None if reset is None else (ctypes.c_uint8 * B)(*reset),
                                      i32(relabel), i32(keep), pad_mode, discrete, _ptr(actions), _ptr(eng._tokens), _stream_ptr(eng.device))
        if rc != 0:
            raise LramError(eng.lib.lram_last_error().decode())
    _refused(eng, spec, lambda: raw(pad_mode=2), "pad_mode")
    _refused(eng, spec, lambda: raw(reset=[0, 1, 0, 0], relabel=[0, 2, 0, 0]), "reset and relabelled")
    _refused(eng, spec, lambda: raw(relabel=[0, 0, -1, 0]), "negative")
    _refused(eng, spec, lambda: raw(keep=[-3, 0, 0, 0]), "negative")
    _refused(eng, spec, lambda: raw(actions=None), "null device pointer")
    _refused(eng, spec, lambda: raw(discrete=2), "slot table")     # (LRAM_HEAD_PER_SLOT without a table: what lram_prefill refuses)
    eng.set_live(B - 1)
    _refused(eng, spec, lambda: raw(), "parked")
    eng.set_live(B)
    for mode in ("live", "started"):
        eng.set_context_rows(mode)
        _refused(eng, spec, lambda: raw(), "LRAM_CONTEXT_ROWS_ALL")
    eng.set_context_rows("all")
    if name == "mamba":
        for rep, stale in ((3, False), (1, True)):
            eng.set_compat_mode(rep, stale)
            _refused(eng, spec, lambda: raw(), "lram_set_compat_mode")
        eng.set_compat_mode(1, False)
    eng.set_graph_mode(True)     # graph mode: never captured, runs launch by launch as prefill does
    step(pad="reference")
    eng.set_graph_mode(False)
    # the ring itself: K beyond 2 GiB of windows, a negative K; the ring is still there afterwards
    for bad, needle in ((((1 << 29) // (B * spec.d_model)) + 1, "2 GiB"), (-1, "timesteps")):
        with pytest.raises(LramError, match=needle):
            if eng.lib.lram_window_alloc(eng._h, bad) != 0:
                raise LramError(eng.lib.lram_last_error().decode())
    assert eng.window().counts == [3] * B
    eng.alloc(B)                 # lram_state_alloc frees the ring
    with pytest.raises(LramError, match="no window ring"):
        eng.window()
    eng.close()


def test_geometries_without_the_front_end_get_no_ring(hip_lib):
    """tokens_per_step != 3 is refused where the ring would be made.  (d_model % 4 != 0, which lram_window_alloc refuses as well,
    cannot be reached: lram_create admits no such model.)"""
    for kw, needle in ((dict(tokens_per_step=2, pred_token=1), "tokens_per_step == 3"),):
        spec = dataclasses.replace(wc.spec_of("mamba"), **kw)
        eng = new_engine(spec, init_state_dict(spec, seed=3), 2)
        with pytest.raises(LramError, match=needle):
            if eng.lib.lram_window_alloc(eng._h, 4) != 0:
                raise LramError(eng.lib.lram_last_error().decode())
        eng.close()


# ---- 6. the agent on the real engine ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [False, True])
def test_agent_in_window_mode_feeds_the_reference_padded_windows(hip_lib, image):
    """RecurrentAgent(use_inference_cache=False): 7 steps at K = 4 with a reset, against Engine.prefill over the windows the test
    keeps -- observations padded and normalised (frames: embedded) as the agent does it, left-padded with the embedded
    (0 - mean) / std (frames: the embedding of an all-zero frame), rtg 0 and reward 0.  Frames: bit for bit; vectors: the actions
    under the tie rule of helpers.assert_actions_match."""
    from lram_amd.agent import RecurrentAgent
    spec = wc.spec_of("xlstm")
    sd = init_state_dict(spec, seed=3, with_image_encoder=image)
    B, K = 3, 4
    mean, std = torch.linspace(-1, 1, spec.state_dim), torch.linspace(0.5, 2, spec.state_dim)
    agent = RecurrentAgent(spec, sd, n_envs=B, device=DEV, state_mean=None if image else mean, state_std=None if image else std,
                           use_inference_cache=False, eval_context_len=K)
    ref = new_engine(spec, sd, B)
    g = torch.Generator().manual_seed(4)
    if image:
        pad_vec = ref.embed_images(torch.zeros(B, *spec.image_shape, dtype=torch.uint8, device=DEV))[0].clone().cpu()
    else:
        pad_vec = (-mean / std).contiguous()
    hist, prev = wc.History(B, K), torch.zeros(B)
    for t in range(7):
        if image:
            obs = torch.randint(0, 256, (B, *spec.image_shape), generator=g, dtype=torch.uint8)
            vec = ref.embed_images(obs.to(DEV)).clone().cpu()
        else:
            obs = torch.rand(B, 12, generator=g) * 2 - 1
            vec = (torch.cat([obs, torch.zeros(B, spec.state_dim - 12)], 1) - mean) / std
        rtg, rew = 4.0 - 0.1 * t + torch.rand(B, generator=g), torch.rand(B, generator=g)
        reset = [t == 0, t == 0 or t == 3, t == 0]
        act = agent.predict_batch(obs, rtg, None, torch.tensor(reset, dtype=torch.uint8), None, prev_rewards=prev).clone()
        hist.step(vec, rtg, prev, reset=reset)
        prev = rew
        want, _ = ref.prefill(*_dev(*hist.tensors(pad_vec=pad_vec)), reset_mask=_ones(B), obs_is_embedding=image)
        torch.cuda.synchronize()
        if image:   # embeddings in, the same launches
            assert torch.equal(bits(act), bits(want)), t
        else:       # (the state Linear runs at B rows here and at B * K rows there: another kernel, another rounding)
            lg = _logits(ref).view(B, spec.act_dim, spec.n_vocab).cpu()
            assert_actions_match(act.cpu(), want.cpu(), lg, spec, what=f"vector agent, step {t}")
    agent.engine.close(), ref.close()
