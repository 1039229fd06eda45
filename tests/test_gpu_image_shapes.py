"""GPU: the image front end (csrc/impala_cnn.hip, `image_buffers` / `embed_images` in csrc/engine_image.hip) at frame sizes other
than 64 x 64, through lram_embed_images, lram_step_images and the image slots of lram_step_slots.

At 64 x 64 the maps are 64 / 32 / 16 / 8 wide: whole numbers of conv tiles (16 x 16; 8 x 8 for 32-channel maps of at most 256
pixels), even extents under every pool, as many tiles in x as in y, three input channels.  The sizes here reach what that size
cannot: a ragged last tile, a map below one tile, an odd extent under the pool, a tile grid with different counts in x and y,
1 and 4 input channels, work buffers whose per-frame sizes are odd, and a frame size that changes between calls.

Reference: oracle.dt_ref.impala_cnn evaluated in float64 (weights .double(), frames .double() / 255).
Bar: max |out - ref| <= 2e-5 * max |ref| over the batch, the bar tests/test_gpu_golden.py holds this path to at 64 x 64.  The
float32 oracle is itself 2.9e-7 .. 5.0e-7 from float64 on that metric (tests/test_oracle_selfchecks.py holds it below 1e-6), so
the bar leaves about 40 x over fp32 rounding.  Model: xLSTM d_model 128, 2 blocks (sLSTM at 1), init_state_dict(spec, seed,
with_image_encoder=True), batch 5.

Every test prints its worst max |out - ref| / max |ref| (run with -s).  Measured on an MI355X, against the bar of 2e-5:

    shape sweep    (3,84,84) 5.9e-7   (1,84,84) 5.7e-7   (4,40,24) 8.1e-7   (3,33,65) 5.3e-7   (3,17,33) 3.9e-7
                   (3,21,21) 5.2e-7   (1,8,8)   3.7e-7   (3,1,9)   2.1e-7   (3,64,64) 2.9e-7
    border frames  (3,21,21) 4.5e-7   (3,33,65) 4.9e-7
    size changes   5.9e-7 (worst of the five calls)
    token tap at (3,21,27), rel_err against the bar of 2e-4: step_images 8.0e-7, step_slots 9.0e-7 (hidden tap 3.3e-6)

The engine is as close to float64 as the float32 oracle is.  With one comparison of impala_cnn.hip changed the same tests are
5.5e-2 .. 8.4e-1 of max |ref| off: the halo staged up to x < W - 1, or the pool window cut at yy < H - 1, fails every size of
the sweep (64 x 64 included) and both border tests; tiles_x taken from H fails exactly the sizes with H != W.
"""
import pytest
import torch

from lram_amd import init_state_dict
from lram_amd.config import ModelSpec
from oracle.dt_ref import OraclePolicy, impala_cnn
from tests.helpers import IMAGE_SHAPE_SWEEP, assert_actions_match, make_inputs, pooled_hw, rel_err
from tests.test_gpu_slots import _check_against_oracle, _check_fill, _frames_of, _oracle_groups, _same, _set

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 2e-5          # of max |ref|, against float64
TOK_TOL = 2e-4      # rel_err of the embed_ln token tap, the suite's bar
B = 5
_id = lambda s: "x".join(map(str, s))


def _spec(shape):
    return ModelSpec(backbone="xlstm", d_model=128, n_blocks=2, slstm_at=[1], image_shape=tuple(shape))


def _engine(spec, sd, batch=B):
    from lram_amd.engine import Engine
    return Engine(spec, sd, batch, device=DEV)


def _frames(shape, seed, n=B):
    return torch.randint(0, 256, (n, *shape), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _ref64(sd, img):
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith("embed_image.")}
    with torch.no_grad():
        return impala_cnn(sd64, "embed_image.", img.double() / 255.0)


def _ratio(out, ref):
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    scale = float(ref.abs().max())
    assert scale > 0.0
    return float((out.detach().cpu().double() - ref).abs().max()) / scale


def _embed(eng, img):
    out = eng.embed_images(img.to(DEV))
    torch.cuda.synchronize()
    return out.cpu()


# ---- a. shape sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", IMAGE_SHAPE_SWEEP, ids=_id)
def test_embed_images_shape_sweep(hip_lib, shape):
    """lram_embed_images against float64 at every frame size of the sweep; a second call on the same buffers is bit-equal.
    (3, 84, 84): ragged 16-tiles, odd extents under the pool, a 21 x 21 32-channel map on the 16-tile kernel, an 11 x 11 map on
    ragged 8-tiles.  (1, 84, 84): one input channel.  (4, 40, 24): four channels, H != W, a 240-pixel 32-channel map just below
    the 8-tile rule.  (3, 33, 65) / (3, 17, 33): tile grids with different counts in x and y at every stage, both ways round.
    (3, 21, 21): every map ragged or below one tile.  (1, 8, 8): a 1 x 1 final map.  (3, 1, 9): stages 2 and 3 need more of
    the stage-conv buffer than stage 1 (32 * 1 * 5 > 16 * 1 * 9 floats per frame).  (3, 64, 64): control."""
    spec = _spec(shape)
    sd = init_state_dict(spec, seed=7, with_image_encoder=True)
    h, w = pooled_hw(shape[1], shape[2])
    assert sd["embed_image.linear.0.weight"].shape == (128, 32 * h * w)
    img = _frames(shape, seed=3)
    ref = _ref64(sd, img)
    eng = _engine(spec, sd)
    out = _embed(eng, img)
    out2 = _embed(eng, img)
    eng.close()
    r = _ratio(out, ref)
    print(f"embed_images {_id(shape)}: max|out - ref64| / max|ref64| = {r:.3e}")
    assert r <= BAR, f"{_id(shape)}: {r:.3e} of max |ref|"
    _same(out, out2, f"{_id(shape)}: second call")


# ---- b. frames on which a wrong border pixel shows ----------------------------------------------------------------------------------
def _border_frames(shape):
    """All 255, all 0, one 255 pixel (every channel) at each corner and at the first pixel of the second 16-tile in x and in y,
    a checkerboard; padded with random frames to a whole number of batches."""
    C, H, W = shape
    frames = [torch.full(shape, 255, dtype=torch.uint8), torch.zeros(shape, dtype=torch.uint8)]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 16), (16, 0)):
        f = torch.zeros(shape, dtype=torch.uint8)
        f[:, y, x] = 255
        frames.append(f)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    frames.append((((yy + xx) % 2) * 255).to(torch.uint8).expand(C, H, W).contiguous())
    pad = -len(frames) % B
    frames += list(_frames(shape, seed=5, n=pad))
    return torch.stack(frames)


@pytest.mark.parametrize("shape", [(3, 21, 21), (3, 33, 65)], ids=_id)
def test_embed_images_border_frames(hip_lib, shape):
    """The first conv is followed directly by a 3 x 3 max-pool, so random frames can hide a wrong border pixel: constant frames,
    single lit pixels at the corners and on the tile seams, and a checkerboard against float64."""
    assert shape[1] > 16 and shape[2] > 16
    spec = _spec(shape)
    sd = init_state_dict(spec, seed=7, with_image_encoder=True)
    frames = _border_frames(shape)
    assert frames.shape[0] % B == 0 and frames.shape[0] >= 9
    eng = _engine(spec, sd)
    worst = 0.0
    for k in range(0, frames.shape[0], B):
        img = frames[k:k + B]
        r = _ratio(_embed(eng, img), _ref64(sd, img))
        worst = max(worst, r)
        assert r <= BAR, f"{_id(shape)} border frames {k} .. {k + B - 1}: {r:.3e} of max |ref|"
    eng.close()
    print(f"border frames {_id(shape)}: max|out - ref64| / max|ref64| = {worst:.3e}")


# ---- c. one engine, changing sizes --------------------------------------------------------------------------------------------------
def test_frame_size_changes_between_calls(hip_lib):
    """Weights for a pooled 8 x 7 map; sizes in an order in which the pixel count falls while the pooled map grows (62 x 56 ->
    63 x 55: 3472 -> 3465 pixels, 31 x 28 -> 32 x 28 pooled), grows, falls again.  Every result is within the bar of float64 and
    bit-equal to a fresh engine's at that size; the last call repeats the first, bit for bit."""
    sizes = [(3, 62, 56), (3, 63, 55), (3, 64, 56), (3, 57, 49), (3, 62, 56)]
    assert all(pooled_hw(s[1], s[2]) == (8, 7) for s in sizes)
    assert 62 * 56 > 63 * 55 and 31 * 28 < 32 * 28
    spec = _spec(sizes[0])
    sd = init_state_dict(spec, seed=9, with_image_encoder=True)
    imgs = {s: _frames(s, seed=100 + s[1]) for s in set(sizes)}
    refs = {s: _ref64(sd, im) for s, im in imgs.items()}
    eng = _engine(spec, sd)
    outs, worst = [], 0.0
    for i, s in enumerate(sizes):
        out = _embed(eng, imgs[s])
        r = _ratio(out, refs[s])
        worst = max(worst, r)
        assert r <= BAR, f"call {i} at {_id(s)}: {r:.3e} of max |ref|"
        outs.append(out)
    eng.close()
    _same(outs[-1], outs[0], "the last call against the first")
    for s in set(sizes):
        fresh = _engine(spec, sd)
        want = _embed(fresh, imgs[s])
        fresh.close()
        for i, t in enumerate(sizes):
            if t == s:
                _same(outs[i], want, f"call {i} at {_id(s)} against a fresh engine")
    print(f"changing sizes: max|out - ref64| / max|ref64| = {worst:.3e}")


# ---- d. the env-slice paths at an odd size --------------------------------------------------------------------------------------------
ODD = (3, 21, 27)   # maps 21x27 / 11x14 / 6x7 / 3x4: 16 * 567 and 32 * 154 floats per frame in the work buffers
# On this seed the oracle's smallest top-2 logit gap is 1.4e-2 (step_images) and 6.9e-3 (step_slots): 34 x the 2e-4 tie rule
# and more, so "no ties" is a property of the inputs, not of the engine.
STEP_SEED = 20261021


def test_step_images_env_slices_at_an_odd_size(hip_lib):
    """lram_step_images with 1, 2 and 3 env slices (batch 7: slices of 3 + 2 + 2 frames, each in its own region of the work
    buffers): actions follow the oracle with no ties, the embed_ln token tap is within 2e-4 of the oracle's tokens, and the three
    slicings give the same actions."""
    spec = _spec(ODD)
    sd = init_state_dict(spec, seed=41, with_image_encoder=True)
    n, steps = 7, 4
    seq = make_inputs(spec, n, steps, seed=STEP_SEED, image=True)
    assert bool(seq[0][3].all())   # reset on step 0
    ora = OraclePolicy(spec, sd)
    want = [ora.step(*inp, discrete=True, return_debug=True) for inp in seq]
    runs, worst = [], 0.0
    for slices in (1, 2, 3):
        eng = _engine(spec, sd, n)
        eng.set_micro_batches(slices)
        ties, acts = 0, []
        for t, inp in enumerate(seq):
            obs, rtg, rew, mask = (x.to(DEV) for x in inp)
            a, _ = eng.step_images(obs, rtg, rew, mask, discrete=True)
            torch.cuda.synchronize()
            tok, _, _ = eng.taps()
            a_ref, dbg = want[t]
            ties += assert_actions_match(a[:, :1], a_ref, dbg["logits"], spec, discrete=True, what=f"{slices} slices step {t}")
            err = rel_err(tok, dbg["tokens"])
            worst = max(worst, err)
            assert err < TOK_TOL, f"{slices} slices step {t}: token tap rel err {err:.3e}"
            acts.append(a[:, :1].cpu().clone())
        eng.close()
        assert ties == 0
        runs.append(acts)
    for k in (1, 2):
        for t in range(steps):
            _same(runs[0][t], runs[k][t], f"1 slice against {k + 1} slices, step {t}: actions")
    print(f"step_images {_id(ODD)}: worst token tap rel err {worst:.3e}")


def test_step_slots_image_slots_at_an_odd_size(hip_lib):
    """lram_step_slots, batch 9 with image slots 1, 2, 5, 8 in two env slices (5 + 4 slots: frames 0, 1 and frames 2, 3): image
    rows against the image oracle, vector rows against the vector oracle, as tests/test_gpu_slots.py does at 64 x 64."""
    spec = _spec(ODD)
    sd = init_state_dict(spec, seed=41, with_image_encoder=True)
    n, steps, A = 9, 4, spec.act_dim
    img_slots = [1, 2, 5, 8]
    kinds = [(0, 0, A), (1, 1, 1), (1, 0, 2), (0, 1, 1), (0, 0, 3), (1, 1, 1), (0, 0, 1), (0, 1, 1), (1, 0, 2)]
    assert [b for b, k in enumerate(kinds) if k[0]] == img_slots
    vec = make_inputs(spec, n, steps, seed=STEP_SEED)
    img = make_inputs(spec, n, steps, seed=STEP_SEED + 1, image=True)
    groups = _oracle_groups(kinds)
    assert sorted(groups) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    runs, worst_tok, worst_hid = [], 0.0, 0.0
    for slices in (1, 2):
        oracles = {k: OraclePolicy(spec, sd) for k in groups}
        eng = _engine(spec, sd, n)
        eng.set_micro_batches(slices)
        _set(eng, kinds)
        assert eng.n_image_slots == 4
        ties, acts = 0, []
        for t in range(steps):
            obs, rtg, rew, mask = (x.to(DEV) for x in vec[t])
            a, tok = eng.step_slots(obs, _frames_of(img[t][0], kinds).to(DEV), rtg, rew, mask)
            torch.cuda.synchronize()
            tap, hid, _ = eng.taps()
            tap = tap.cpu()
            _check_fill(a, tok, kinds, f"{slices} slices step {t}")
            dbg = {}
            k, err = _check_against_oracle(spec, oracles, groups, kinds, vec[t], img[t], a.cpu(), hid.cpu(),
                                           f"{slices} slices step {t}", dbg_out=dbg)
            ties += k
            worst_hid = max(worst_hid, err)
            for g, idx in groups.items():   # image rows against the image oracles' tokens, vector rows against the vector oracles'
                err = rel_err(tap[torch.tensor(idx)], dbg[g]["tokens"])
                worst_tok = max(worst_tok, err)
                assert err < TOK_TOL, f"{slices} slices step {t} group {g}: token tap rel err {err:.3e}"
            acts.append(a.cpu().clone())
        eng.close()
        assert ties == 0
        runs.append(acts)
    for t in range(steps):
        _same(runs[0][t], runs[1][t], f"1 slice against 2 slices, step {t}: actions")
    print(f"step_slots {_id(ODD)}: worst token tap rel err {worst_tok:.3e}, worst hidden tap rel err {worst_hid:.3e}")


# ---- e. loud misuse -------------------------------------------------------------------------------------------------------------------
def test_a_frame_size_that_does_not_fit_the_weights_is_refused(hip_lib):
    from lram_amd.engine import LramError
    shape = (3, 21, 21)   # pooled 3 x 3
    spec = _spec(shape)
    sd = init_state_dict(spec, seed=7, with_image_encoder=True)
    img = _frames(shape, seed=3)
    ref = _ref64(sd, img)
    eng = _engine(spec, sd)
    first = _embed(eng, img)
    rtg, rew = torch.full((B,), 4.5, device=DEV), torch.zeros(B, device=DEV)
    for bad in ((3, 64, 64), (3, 25, 21), (3, 1, 9)):   # pooled 8 x 8, 4 x 3, 1 x 2
        assert pooled_hw(bad[1], bad[2]) != (3, 3)
        wrong = torch.zeros(B, *bad, dtype=torch.uint8, device=DEV)
        for call in (lambda: eng.embed_images(wrong), lambda: eng.step_images(wrong, rtg, rew, None, discrete=True)):
            with pytest.raises(LramError) as ei:
                call()
            assert "image size" in str(ei.value) and f"{bad[1]} x {bad[2]}" in str(ei.value), str(ei.value)
    with pytest.raises(LramError) as ei:
        eng.embed_images(torch.zeros(B, 1, 21, 21, dtype=torch.uint8, device=DEV))
    assert "channel count" in str(ei.value)
    again = _embed(eng, img)
    eng.close()
    _same(again, first, "a correct call after the refusals")
    assert _ratio(again, ref) <= BAR
