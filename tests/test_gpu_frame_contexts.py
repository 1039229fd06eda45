"""GPU: stored contexts from uint8 frames -- Engine.embed_frames / prefill_frames / score_frames (lram_embed_frames,
lram_prefill_frames, lram_score_frames, lram_image_counts; the frame list in csrc/impala_cnn.hip and csrc/engine_image.hip) and the
agent calls on top of them.

Shapes, the smallest at which the path can still go wrong: the image tests' model (xLSTM d_model 128, 2 blocks, sLSTM at 1,
init_state_dict(spec, seed, with_image_encoder=True)) on (3, 21, 21) frames -- every map ragged or below one conv tile -- with
7 envs x 21 timesteps and the lengths 0, 21, 14, 8, 3, 1, 0 of the append sweep (tests/append_cases.py), and one control at
(3, 64, 64) with 5 envs x 4 timesteps.

Bars, all the project's own:
  * embed_frames against oracle.dt_ref.impala_cnn in float64: max |out - ref| <= 2e-5 * max |ref| (tests/test_gpu_image_shapes.py);
  * contexts: tests.context_cases.check_restarted (state_vs_oracle 2e-4, block 0's conv state 1e-5) and check_continued (1e-4
    against an engine that took the same timesteps one lram_step_images at a time), actions by helpers.assert_actions_match with
    the tolerated-tie count asserted 0, after clear_margins has asserted, on the oracle alone, a top-2 logit gap of at least 1e-3
    on every compared row;
  * logp of windowed against single-call scoring: 2 * 2e-4 * max |logits| (tests/test_gpu_append.py);
  * bit for bit wherever two engine runs make the same launches: the tile size, the dense identity, held and kept slots, padded
    frames of another value, a step behind a frames call.
Seeds (weights / inputs), chosen on the CPU for the 1e-3 gap rule alone: SEED_W / SEED_IN below with the gaps they give.

Every test prints what it measured (run with -s).  Measured on an MI355X:

    embed_frames   (3,21,21) x 3 5.2e-7   x 147 5.0e-7   x 300 5.7e-7   (3,64,64) x 20 3.3e-7          (bar 2e-5)
    append         restarted envs: block 0 conv state 3.9e-7 .. 5.4e-7 (bar 1e-5); continued envs against the stepping engine
                   2.1e-7 .. 2.8e-7, tensors and records (bar 1e-4); oracle gap 9.3e-3
    replace        block 0 conv state 3.9e-7 .. 6.1e-7 (bar 1e-5); oracle gap 1.1e-2
    mixed table    block 0 conv state 2.0e-7 .. 5.7e-7 (bar 1e-5); oracle gap 3.9e-3
    agent          logp of windows of 8 off the single call's by 0 .. 1.4e-6 (bar 1.4e-3 .. 1.5e-3); state 1.9e-7 (bar 1e-4)

The lists of 147 and 300 frames reach GEMM instances the image tests' batch of 5 never did (300 rows: f16x2); they are as close to
float64 as that batch is (5.2e-7 at this size in tests/test_gpu_image_shapes.py), so no case is held to anything but the bar.
"""
import ctypes

import pytest
import torch

from lram_amd import init_state_dict
from lram_amd.config import ModelSpec
from lram_amd.engine import context_plan
from oracle.dt_ref import impala_cnn
from tests.context_cases import (DEV, MIN_GAP, NAN, EnvRef, bits, check_continued, check_restarted, clear_margins, env_slices,
                                 export_state, min_gap, new_engine, same_state, u8_mask)
from tests.helpers import assert_actions_match, make_inputs, rel_err

pytestmark = pytest.mark.gpu

BAR = 2e-5                      # of max |ref|, against float64
SHAPE, CONTROL = (3, 21, 21), (3, 64, 64)
B, L, NPRE = 7, 21, 3
LENGTHS = [0, 21, 14, 8, 3, 1, 0]
RESTART = [1, 1, 0, 1, 0, 1, 0]
PRE, BEHIND = range(L, L + NPRE), [L + NPRE]
# weights / inputs, the first pair tried; the oracle's smallest top-2 logit gap over the compared rows: append case 9.3e-3, replace
# case 1.1e-2, mixed case 3.9e-3 (discrete slots: over their n_discrete logits)
SEED_W, SEED_IN = 41, 702
MIX_W, MIX_IN = 41, 703
N_IMG, N_VEC = 3, 4

_CACHE = {}


def _spec(shape=SHAPE):
    return ModelSpec(backbone="xlstm", d_model=128, n_blocks=2, slstm_at=[1], image_shape=tuple(shape))


def _rand_frames(n, shape, seed):
    return torch.randint(0, 256, (n, *shape), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _ref64(sd, img):
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith("embed_image.")}
    with torch.no_grad():
        return impala_cnn(sd64, "embed_image.", img.double() / 255.0)


def _ratio(out, ref):
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    return float((out.detach().cpu().double() - ref).abs().max()) / float(ref.abs().max())


def frame_stack(seq, n_steps, lengths=None, pad=0, rows=None):
    """frames uint8 [n, L, C, H, W], rtg and rew [B, L] on the device: timesteps 0 .. L - 1 of seq; with lengths, every padded frame
    holds `pad` and every padded rtg / reward NaN.  rows: the env rows whose frames are handed in (None: all)."""
    frames, rtg, rew = (torch.stack([x[i] for x in seq[:n_steps]], 1).contiguous() for i in range(3))
    if lengths is not None:
        for b, n in enumerate(lengths):
            frames[b, n:], rtg[b, n:], rew[b, n:] = pad, NAN, NAN
    if rows is not None:
        frames = frames[rows].contiguous()
    return frames.to(DEV), rtg.to(DEV), rew.to(DEV)


def image_steps(eng, seq, ts):
    for t in ts:
        eng.step_images(*(x.to(DEV) for x in seq[t][:3]), None)


def stepping_snapshots_frames(spec, sd, seq, pre, lengths, restart):
    """tests.context_cases.stepping_snapshots with lram_step_images: a second engine takes the env-steps `pre`, then timesteps
    0 .. one frame at a time (the restart flags on timestep 0); env b's state right after its own last step."""
    eng = new_engine(spec, sd, len(lengths))
    image_steps(eng, seq, pre)
    snaps = {}
    for t in range(max(lengths)):
        eng.step_images(*(x.to(DEV) for x in seq[t][:3]), u8_mask(restart) if t == 0 else None)
        for b, n in enumerate(lengths):
            if n == t + 1:
                snaps[b] = (env_slices(eng, spec, b), eng.save_slots([b]).cpu())
    eng.close()
    return snaps


def case_refs(seed_w=SEED_W, seed_in=SEED_IN):
    """(spec, weights, inputs, append refs, replace refs): the oracle's run of every env.  Append: a restarted env from an empty
    state over its own context, a continuing one with the env-steps ahead, a held one over the env-steps alone, each with the
    env-step behind the call.  Replace: every env with a context from an empty state, the others over the env-steps alone.
    Pure CPU: the seeds were chosen with it."""
    key = ("case", seed_w, seed_in)
    if key not in _CACHE:
        spec = _spec()
        sd = init_state_dict(spec, seed=seed_w, with_image_encoder=True)
        seq = make_inputs(spec, B, L + NPRE + 1, seed=seed_in, reset_prob=0.0, image=True)
        app = [EnvRef(spec, sd, seq, b, n, pre=() if (RESTART[b] and n) else PRE, cont=BEHIND) for b, n in enumerate(LENGTHS)]
        rep = [app[b] if (RESTART[b] or not n) else EnvRef(spec, sd, seq, b, n, cont=BEHIND) for b, n in enumerate(LENGTHS)]
        _CACHE[key] = (spec, sd, seq, app, rep)
    return _CACHE[key]


# ---- a. embed_frames against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [(SHAPE, 3), (SHAPE, 147), (SHAPE, 300), (CONTROL, 20)], ids=lambda v: str(v).replace(" ", ""))
def test_embed_frames_against_float64(hip_lib, shape, n):
    """3 frames (below the batch of 5), 147 = 7 x 21 (the contexts' dense list) and 300 (past the f16x2 threshold of 256 rows; one
    tile of the default 2048) against float64; a second call is bit-equal; the counts say what ran."""
    spec = _spec(shape)
    sd = init_state_dict(spec, seed=7, with_image_encoder=True)
    img = _rand_frames(n, shape, seed=3)
    ref = _ref64(sd, img)
    eng = new_engine(spec, sd, 5)
    eng.image_counts(reset=True)
    out = eng.embed_frames(img.to(DEV))
    out2 = eng.embed_frames(img.to(DEV).view(1, n, *shape))
    torch.cuda.synchronize()
    counts = eng.image_counts()
    eng.close()
    r = _ratio(out, ref)
    print(f"[frames] embed_frames {shape} x {n}: max|out - ref64| / max|ref64| = {r:.3e} (bar {BAR:.0e}); counts {counts}")
    assert r <= BAR, (shape, n, r)
    assert out2.shape == (1, n, spec.d_model) and torch.equal(bits(out), bits(out2[0]))
    assert counts == {"frames": 2 * n, "tiles": 2, "linear": 2}, counts


# ---- b. the tile size changes nothing ----------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_tile(hip_lib, monkeypatch):
    """LRAM_IMG_TILE = 4, 5 and the default, each on a fresh engine: embed_frames of 147 frames and the exported state after a
    ragged prefill_frames are bit-identical; the tiles launched are ceil(frames / tile)."""
    spec, sd, seq, _, _ = case_refs()
    img = _rand_frames(147, SHAPE, seed=11).to(DEV)
    frames, rtg, rew = frame_stack(seq, L, LENGTHS)
    runs = []
    for tile in ("4", "5", None):
        if tile is not None:
            monkeypatch.setenv("LRAM_IMG_TILE", tile)
        eng = new_engine(spec, sd, B)
        if tile is not None:
            monkeypatch.delenv("LRAM_IMG_TILE")
        eng.image_counts(reset=True)
        emb = eng.embed_frames(img).cpu()
        tiles_embed = eng.image_counts(reset=True)["tiles"]
        act, tok = eng.prefill_frames(frames, rtg, rew, lengths=LENGTHS, reset_mask=u8_mask([1] * B))
        torch.cuda.synchronize()
        counts = eng.image_counts()
        f = int(tile) if tile else 2048
        assert tiles_embed == -(-147 // f) and counts == {"frames": sum(LENGTHS), "tiles": -(-sum(LENGTHS) // f), "linear": 1}, (tile, counts)
        runs.append((emb, act.cpu().clone(), tok.cpu().clone(), [t.cpu() for t in export_state(eng, spec)]))
        eng.close()
    for k in (1, 2):
        assert torch.equal(bits(runs[0][0]), bits(runs[k][0])), f"embed_frames, run {k}"
        assert torch.equal(bits(runs[0][1]), bits(runs[k][1])) and torch.equal(runs[0][2], runs[k][2]), f"actions, run {k}"
        same_state(runs[0][3], runs[k][3], f"tile run {k} against tile 4")


# ---- c. the dense call is prefill / score of the embeddings ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n_env,n_steps", [(SHAPE, B, L), (CONTROL, 5, 4)], ids=["3x21x21", "3x64x64"])
def test_dense_calls_are_bit_identical_to_the_calls_on_embeddings(hip_lib, shape, n_env, n_steps):
    spec = _spec(shape)
    sd = init_state_dict(spec, seed=SEED_W, with_image_encoder=True)
    seq = make_inputs(spec, n_env, n_steps, seed=SEED_IN, reset_prob=0.0, image=True)
    frames, rtg, rew = frame_stack(seq, n_steps)
    ones = u8_mask([1] * n_env)
    target = (torch.rand(n_env, n_steps, spec.act_dim, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    e_f, e_e = new_engine(spec, sd, n_env), new_engine(spec, sd, n_env)
    emb = e_e.embed_frames(frames)
    assert emb.shape == (n_env, n_steps, spec.d_model)
    a_f, t_f = e_f.prefill_frames(frames, rtg, rew, reset_mask=ones)
    a_e, t_e = e_e.prefill(emb, rtg, rew, reset_mask=ones, obs_is_embedding=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(a_f), bits(a_e)) and torch.equal(t_f, t_e)
    same_state(export_state(e_f, spec), export_state(e_e, spec), "prefill_frames against prefill of the embeddings")
    # ... and score, continuing the state (no reset)
    s_f = e_f.score_frames(frames, rtg, rew, actions=target)
    s_e = e_e.score(emb, rtg, rew, actions=target, obs_is_embedding=True)
    torch.cuda.synchronize()
    for name in ("actions", "tokens", "logp"):
        assert torch.equal(bits(getattr(s_f, name)), bits(getattr(s_e, name))), name
    assert bool(s_f.logp.isfinite().all())
    same_state(export_state(e_f, spec), export_state(e_e, spec), "score_frames against score of the embeddings")
    # full lengths: the dense launches
    a_l, t_l = e_f.prefill_frames(frames, rtg, rew, reset_mask=ones, lengths=[n_steps] * n_env, append=True)
    a_d, t_d = e_e.prefill_frames(frames, rtg, rew, reset_mask=ones)
    torch.cuda.synchronize()
    assert torch.equal(bits(a_l), bits(a_d)) and torch.equal(t_l, t_d)
    same_state(export_state(e_f, spec), export_state(e_e, spec), "full lengths against the dense call")
    e_f.close(), e_e.close()


# ---- d. per-env lengths: append and replace ------------------------------------------------------------------------------------------
def _append_run(pad):
    spec, sd, seq, _, _ = case_refs()
    eng = new_engine(spec, sd, B)
    image_steps(eng, seq, PRE)
    held = {b: (env_slices(eng, spec, b), eng.save_slots([b]).cpu()) for b, n in enumerate(LENGTHS) if n == 0}
    eng.image_counts(reset=True)
    act, tok = eng.prefill_frames(*frame_stack(seq, L, LENGTHS, pad=pad), lengths=LENGTHS, append=True, reset_mask=u8_mask(RESTART))
    torch.cuda.synchronize()
    return eng, act.cpu().clone(), tok.cpu().clone(), held


def test_appended_frame_contexts_continue_or_restart_each_env(hip_lib):
    """3 env-steps from frames, then ONE lram_prefill_frames(append) call with the sweep's lengths and mask: slots 0 and 6 are held
    bit for bit, slots 1, 3, 5 restart (against the oracle), slots 2, 4 continue (action against the oracle, state against the
    stepping engine); exactly sum(lengths) frames are convolved; padded frames of 0 and of 255 give the same bits; the env-step
    behind the call follows the oracle."""
    spec, sd, seq, refs, _ = case_refs()
    clear_margins(refs, "frames append")
    assert context_plan(L, LENGTHS, 21) == [0, 7, 13, 18, 20]
    snaps = stepping_snapshots_frames(spec, sd, seq, PRE, LENGTHS, [r if n else 0 for r, n in zip(RESTART, LENGTHS)])
    eng, act, tok, held = _append_run(pad=0)
    counts = eng.image_counts()
    assert counts["frames"] == sum(LENGTHS) == 47 and counts["linear"] == 1, counts
    assert bool(act.isfinite().all())
    for b, n in enumerate(LENGTHS):
        if n == 0:
            for i, (x, y) in enumerate(zip(held[b][0], env_slices(eng, spec, b))):
                assert torch.equal(bits(x), bits(y)), (b, i)
            assert torch.equal(bits(held[b][1]), bits(eng.save_slots([b]).cpu())), b
            assert bool((act[b] == 0).all()) and bool((tok[b] == -1).all()), b
        elif RESTART[b]:
            check_restarted(eng, spec, b, act, refs[b], "frames append")
        else:
            check_continued(eng, spec, b, act, refs[b], snaps[b], "frames append")
    state = [t.cpu() for t in export_state(eng, spec)]
    a_next, _ = eng.step_images(*(x.to(DEV) for x in seq[BEHIND[0]][:3]), None)
    torch.cuda.synchronize()
    for b in range(B):
        assert assert_actions_match(a_next[b:b + 1].cpu(), *refs[b].cont[-1], spec, what=f"step behind the call, env {b}") == 0
    eng.close()
    eng2, act2, tok2, _ = _append_run(pad=255)
    assert torch.equal(bits(act), bits(act2)) and torch.equal(tok, tok2)
    same_state(state, [t.cpu() for t in export_state(eng2, spec)], "padded frames of 255 against padded frames of 0")
    eng2.close()


def test_ragged_frame_contexts_replace_each_env(hip_lib):
    """The replace rule (append=False) after 3 env-steps, every env restarting (a shorter context always does; the mask decides
    for the one of full length): every env with a context holds the state of its own frames from an empty state; slots of
    length 0 are kept bit for bit; score_frames with the same lengths leaves the same state and masks the padded rows."""
    spec, sd, seq, _, refs = case_refs()
    clear_margins(refs, "frames replace")
    eng = new_engine(spec, sd, B)
    image_steps(eng, seq, PRE)
    kept = {b: eng.save_slots([b]).cpu() for b, n in enumerate(LENGTHS) if n == 0}
    eng.image_counts(reset=True)
    inputs = frame_stack(seq, L, LENGTHS, pad=255)
    act, tok = eng.prefill_frames(*inputs, lengths=LENGTHS, reset_mask=u8_mask([1] * B))
    torch.cuda.synchronize()
    act, tok = act.cpu().clone(), tok.cpu().clone()
    assert eng.image_counts()["frames"] == sum(LENGTHS)
    for b, n in enumerate(LENGTHS):
        if n == 0:
            assert torch.equal(bits(kept[b]), bits(eng.save_slots([b]).cpu())), b
            assert bool((act[b] == 0).all()) and bool((tok[b] == -1).all()), b
        else:
            check_restarted(eng, spec, b, act, refs[b], "frames replace")
    state = export_state(eng, spec)
    eng2 = new_engine(spec, sd, B)
    image_steps(eng2, seq, PRE)
    res = eng2.score_frames(*inputs, lengths=LENGTHS, reset_mask=u8_mask([1] * B), want=("actions", "tokens"))
    torch.cuda.synchronize()
    same_state(state, export_state(eng2, spec), "score_frames against prefill_frames")
    for b, n in enumerate(LENGTHS):
        assert bool((res.tokens[b, n:] == -1).all()) and bool((res.tokens[b, :n] >= 0).all()), b
        if n:
            assert torch.equal(bits(res.actions[b, n - 1].cpu()), bits(act[b])), b
    eng.close(), eng2.close()


# ---- e. a mixed slot table -----------------------------------------------------------------------------------------------------------
def mixed_case(seed_w=MIX_W, seed_in=MIX_IN):
    """3 image slots (discrete head) ahead of 4 vector slots (3 action dims), lengths as above: per-slot oracle runs from an empty
    state, each on its own kind of observation.  gap: the smallest top-2 gap over the logits each slot's head picks from."""
    key = ("mixed", seed_w, seed_in)
    if key not in _CACHE:
        from lram_amd.domains import Domain, SlotTable
        spec = _spec()
        sd = init_state_dict(spec, seed=seed_w, with_image_encoder=True)
        tab = SlotTable.from_domains([(Domain("procgen", True, 1, image=True), N_IMG), (Domain("metaworld", False, 3), N_VEC)],
                                     max_act_dim=spec.act_dim)
        img = make_inputs(spec, B, L, seed=seed_in, reset_prob=0.0, image=True)
        vec = make_inputs(spec, B, L, seed=seed_in + 1, reset_prob=0.0)
        refs = [EnvRef(spec, sd, img if b < N_IMG else vec, b, n) for b, n in enumerate(LENGTHS)]
        gaps = []
        for b, n in enumerate(LENGTHS):
            if n:
                lg = refs[b].logits
                gaps.append(min_gap(lg.reshape(1, -1)[:, :spec.n_discrete]) if b < N_IMG else min_gap(lg[..., :3, :]))
        _CACHE[key] = (spec, sd, tab, img, vec, refs, min(gaps))
    return _CACHE[key]


def test_mixed_table_of_image_and_vector_slots(hip_lib):
    """lram_prefill_frames with a slot table: frames [3, L, ...] for the image slots, observations [7, L, state_dim] whose rows of
    image slots and whose padded positions all hold NaN.  Every slot's state and action follow its own oracle; the frames
    convolved are the image slots' lengths alone."""
    spec, sd, tab, img, vec, refs, gap = mixed_case()
    print(f"[frames] mixed table: smallest oracle top-2 gap over the compared rows {gap:.3e} (needs >= {MIN_GAP:.0e})")
    assert gap >= MIN_GAP
    frames, rtg, rew = frame_stack(img, L, LENGTHS, pad=255, rows=list(range(N_IMG)))
    obs = torch.stack([x[0] for x in vec[:L]], 1).contiguous()
    obs[:N_IMG] = NAN
    for b, n in enumerate(LENGTHS):
        obs[b, n:] = NAN
    eng = new_engine(spec, sd, B)
    eng.set_slot_table(*tab.engine_arrays())
    eng.image_counts(reset=True)
    act, tok = eng.prefill_frames(frames, rtg, rew, obs_seq=obs.to(DEV), lengths=LENGTHS, reset_mask=u8_mask([1] * B), discrete="per_slot")
    torch.cuda.synchronize()
    act = act.cpu().clone()
    assert eng.image_counts()["frames"] == sum(LENGTHS[:N_IMG]) == 35
    assert bool(act.isfinite().all())
    for b, n in enumerate(LENGTHS):
        if n == 0:
            continue
        ref = refs[b]
        if b < N_IMG:
            want = torch.argmax(ref.logits.reshape(1, -1)[:, :spec.n_discrete], dim=-1)
            assert assert_actions_match(act[b:b + 1, :1], want, ref.logits, spec, discrete=True, what=f"mixed, image slot {b}") == 0
        else:
            assert assert_actions_match(act[b:b + 1, :3], ref.act[:, :3], ref.logits[..., :3, :], spec, what=f"mixed, vector slot {b}") == 0
        check_restarted(eng, spec, b, None, ref, "mixed table")
    eng.close()


# ---- f. refusals ---------------------------------------------------------------------------------------------------------------------
def _c_calls(eng, frames, rtg, rew, shape, n_steps):
    """The two C entries called directly (shapes Python would refuse first): fn(timesteps=, lengths=, obs=, shape=) -> rc."""
    from lram_amd.engine import _ptr, _stream_ptr
    n_env = eng.batch
    logp = torch.zeros(n_env, n_steps, eng.spec.act_dim, device=DEV)
    tokens = torch.zeros(n_env, n_steps, eng.spec.act_dim, dtype=torch.int32, device=DEV)

    def prefill(timesteps=n_steps, lengths=None, obs=None, shape=shape, append=0):
        arr = (ctypes.c_int32 * n_env)(*lengths) if lengths is not None else None
        return eng.lib.lram_prefill_frames(eng._h, _ptr(frames), *shape, _ptr(obs), _ptr(rtg), _ptr(rew), timesteps, arr, append, None, 0,
                                           _ptr(eng._actions), _ptr(eng._tokens), _stream_ptr(eng.device))

    def score(timesteps=n_steps, lengths=None, obs=None, shape=shape, append=0):
        arr = (ctypes.c_int32 * n_env)(*lengths) if lengths is not None else None
        return eng.lib.lram_score_frames(eng._h, _ptr(frames), *shape, _ptr(obs), _ptr(rtg), _ptr(rew), timesteps, arr, append, None, 0,
                                         None, _ptr(tokens), None, 0, 1.0, None, None, _ptr(logp), None, _stream_ptr(eng.device))
    return (prefill, "lram_prefill_frames"), (score, "lram_score_frames")


def _refused(eng, calls, needles, **kw):
    n_env = eng.batch
    for call, entry in calls:
        before = eng.save_slots(list(range(n_env))).clone()
        torch.cuda.synchronize()
        assert call(**kw) != 0, (entry, kw)
        msg = eng.lib.lram_last_error().decode()
        assert entry in msg and all(n in msg for n in needles), msg
        after = eng.save_slots(list(range(n_env)))
        torch.cuda.synchronize()
        assert torch.equal(bits(before), bits(after)), msg


def test_refused_calls_name_the_entry_and_leave_the_state_alone(hip_lib):
    from lram_amd.domains import Domain, SlotTable
    from lram_amd.engine import LramError
    spec, sd, seq, _, _ = case_refs()
    n_env, n_steps = 5, 4
    frames, rtg, rew = frame_stack([tuple(x[:n_env] for x in s) for s in seq], n_steps)
    eng = new_engine(spec, sd, n_env)
    eng.prefill_frames(frames, rtg, rew, reset_mask=u8_mask([1] * n_env), want_action=False)    # a state that is not empty
    calls = _c_calls(eng, frames, rtg, rew, SHAPE, n_steps)
    _refused(eng, calls, ["image size", "64 x 64"], shape=CONTROL)                               # a size the Linear does not fit
    _refused(eng, calls, ["channel count"], shape=(1, 21, 21))
    _refused(eng, calls, ["channels, height and width"], shape=(3, 0, 21))
    big = (1 << 29) // (n_env * spec.d_model) + 1                                                # B * L * d_model past 2 GiB
    _refused(eng, calls, ["state embeddings", "2 GiB"], timesteps=big)
    _refused(eng, calls, ["outside 0 .. timesteps"], lengths=[4, 5, 0, 1, 2])                    # ... and the ragged entries' own
    _refused(eng, calls, ["every length is 0"], lengths=[0] * n_env, append=1)
    _refused(eng, calls, ["append must be"], append=2)
    eng.set_live(3)
    _refused(eng, calls, ["parked"])
    eng.set_live(n_env)
    # a slot table: vector slots need their observations, and a table without an image slot has no frame to take
    tab = SlotTable.from_domains([(Domain("procgen", True, 1, image=True), 2), (Domain("metaworld", False, 3), 3)], max_act_dim=spec.act_dim)
    eng.set_slot_table(*tab.engine_arrays())
    _refused(eng, calls, ["dev_obs_seq is NULL"])
    tab = SlotTable.from_domains([(Domain("metaworld", False, 3), n_env)], max_act_dim=spec.act_dim)
    eng.set_slot_table(*tab.engine_arrays())
    _refused(eng, calls, ["no image slot"])
    eng.set_slot_table(None)
    # the flattened maps of too many frames: lram_embed_frames, nothing launched
    from lram_amd.engine import _ptr, _stream_ptr
    out = torch.zeros(4, spec.d_model, device=DEV)
    too_many = (1 << 29) // (32 * 3 * 3) + 1
    assert eng.lib.lram_embed_frames(eng._h, _ptr(frames), too_many, *SHAPE, _ptr(out), _stream_ptr(eng.device)) != 0
    msg = eng.lib.lram_last_error().decode()
    assert "lram_embed_frames" in msg and "2 GiB" in msg, msg
    # ... and the engine takes the same calls afterwards
    assert all(call() == 0 for call, _ in calls)
    torch.cuda.synchronize()
    eng.close()
    # no image encoder in the state dict
    plain = init_state_dict(spec, seed=SEED_W)
    eng = new_engine(spec, plain, n_env)
    _refused(eng, _c_calls(eng, frames, rtg, rew, SHAPE, n_steps), ["no embed_image.* weights"])
    with pytest.raises(LramError, match="lram_embed_frames: no embed_image"):
        eng.embed_frames(frames)
    eng.close()


def test_mamba_trajectory_modes_and_other_token_layouts_are_refused(hip_lib):
    """The modes and geometries without the state-embedding pass ahead of the chunks: both Mamba modes of lram_set_compat_mode, and
    a model that is not (state, rtg, reward) per timestep."""
    import dataclasses
    from lram_amd import preset
    n_env, n_steps = 5, 4
    spec = dataclasses.replace(preset("mamba_tiny"), image_shape=SHAPE)
    sd = init_state_dict(spec, seed=17, with_image_encoder=True)
    seq = make_inputs(spec, n_env, n_steps, seed=31, reset_prob=0.0, image=True)
    frames, rtg, rew = frame_stack(seq, n_steps)
    eng = new_engine(spec, sd, n_env)
    eng.prefill_frames(frames, rtg, rew, reset_mask=u8_mask([1] * n_env), want_action=False)
    calls = _c_calls(eng, frames, rtg, rew, SHAPE, n_steps)
    for kw in (dict(mamba_repeat=2), dict(stale_state=True)):
        eng.set_compat_mode(**kw)
        _refused(eng, calls, ["lram_set_compat_mode"])
        _refused(eng, calls, ["lram_set_compat_mode"], lengths=[4, 3, 0, 1, 2], append=1)
        eng.set_compat_mode()
    assert all(call() == 0 for call, _ in calls)
    torch.cuda.synchronize()
    eng.close()
    two = dataclasses.replace(_spec(), tokens_per_step=2, pred_token=1)
    sd = init_state_dict(two, seed=17, with_image_encoder=True)
    eng = new_engine(two, sd, n_env)
    _refused(eng, _c_calls(eng, frames, rtg, rew, SHAPE, n_steps), ["tokens_per_step == 3"])
    eng.close()


# ---- g. the agent ----------------------------------------------------------------------------------------------------------------------
def test_agent_scores_and_primes_frame_contexts(hip_lib):
    """RecurrentAgent.score_trajectories(frames, window=8) against the single call (tokens equal, logp within the append tests' bar,
    state within 1e-4), and prime_contexts(frames) followed by predict_batch(frame) against the oracle."""
    from lram_amd.agent import RecurrentAgent
    spec, sd, seq, _, refs = case_refs()     # (the replace refs: every env with a context starts from an empty state)
    clear_margins(refs, "agent, frames")
    frames, rtg, _ = (x.cpu() for x in frame_stack(seq, L, LENGTHS, pad=255))
    rec = torch.rand(B, L, spec.act_dim, generator=torch.Generator().manual_seed(3)) * 2 - 1
    a_one, a_win, a_pri = (RecurrentAgent(spec, sd, n_envs=B, device=DEV) for _ in range(3))
    for a in (a_one, a_win):            # the slots of length 0 keep what three env-steps left
        for t in PRE:
            a.predict_batch(seq[t][0], seq[t][1])
    one = a_one.score_trajectories(frames, rtg, actions=rec, lengths=LENGTHS, logits=True)
    win = a_win.score_trajectories(frames, rtg, actions=rec, lengths=LENGTHS, window=8)
    torch.cuda.synchronize()
    assert torch.equal(win.tokens.cpu(), one.tokens.cpu())
    for b, n in enumerate(LENGTHS):
        assert bool((win.tokens[b, n:] == -1).all()) and bool((win.logp[b, n:] == 0).all()), b
        if n == 0:
            continue
        bar = 2 * 2e-4 * float(one.logits[b, :n].abs().max())
        err = float((win.logp[b, :n].cpu().double() - one.logp[b, :n].cpu().double()).abs().max())
        print(f"[frames] agent score env {b} (n = {n}): logp of windows of 8 off the single call's by {err:.2e} (bar {bar:.2e})")
        assert bool(win.logp[b, :n].isfinite().all()) and err <= bar, (b, err, bar)
        assert assert_actions_match(win.actions[b, n - 1:n].cpu(), refs[b].act, refs[b].logits, spec, what=f"windowed score env {b}") == 0
    worst = max(rel_err(g, w) for g, w in zip(export_state(a_win.engine, spec), export_state(a_one.engine, spec)))
    print(f"[frames] agent: state after windows of 8 against the single call, worst tensor rel_err {worst:.2e} (bar 1e-4)")
    assert worst < 1e-4
    # prime, then continue stepping: envs with a context against the oracle from an empty state
    act = a_pri.prime_contexts(frames, rtg, lengths=LENGTHS, want_action=True).clone()
    nxt = a_pri.predict_batch(seq[BEHIND[0]][0], seq[BEHIND[0]][1]).clone()
    torch.cuda.synchronize()
    for b, n in enumerate(LENGTHS):
        if n:
            assert assert_actions_match(act[b:b + 1].cpu(), refs[b].act, refs[b].logits, spec, what=f"prime_contexts env {b}") == 0
            assert assert_actions_match(nxt[b:b + 1].cpu(), *refs[b].cont[-1], spec, what=f"predict_batch behind prime_contexts, env {b}") == 0
    for a in (a_one, a_win, a_pri):
        a.engine.close()


# ---- h. an env-step behind a frames call ---------------------------------------------------------------------------------------------
def test_step_images_is_unmoved_by_a_larger_tile_before_it(hip_lib):
    """embed_frames of 300 frames grows the work buffers to a tile of 300 frames; step_images of 7 envs in 1 and in 3 env slices then
    finds its regions where a fresh engine finds them: actions, tokens and state bit for bit."""
    spec, sd, seq, _, _ = case_refs()
    img = _rand_frames(300, SHAPE, seed=5).to(DEV)
    for slices in (1, 3):
        runs = []
        for before in (False, True):
            eng = new_engine(spec, sd, B)
            eng.set_micro_batches(slices)
            out = []
            for t in range(3):
                if before and t in (0, 2):
                    eng.embed_frames(img)
                a, tok = eng.step_images(*(x.to(DEV) for x in seq[t][:3]), u8_mask([1] * B) if t == 0 else None)
                torch.cuda.synchronize()
                out.append((a.cpu().clone(), tok.cpu().clone()))
            runs.append((out, [t.cpu() for t in export_state(eng, spec)]))
            eng.close()
        for t in range(3):
            assert torch.equal(bits(runs[0][0][t][0]), bits(runs[1][0][t][0])) and torch.equal(runs[0][0][t][1], runs[1][0][t][1]), (slices, t)
        same_state(runs[0][1], runs[1][1], f"{slices} env slices: step_images behind embed_frames")
