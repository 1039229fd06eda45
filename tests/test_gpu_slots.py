"""GPU: mixed-domain env batches -- the slot table (lram_set_slot_table), the per-slot action head
(discrete = LRAM_HEAD_PER_SLOT), the mixed front end of lram_step_slots and lram_pad_obs_slots, through the C ABI.

Bars (the project's existing ones): discrete actions exact, continuous within 1e-4, hidden states within
2e-4 of the oracle's scale; an action mismatch is tolerated only where the oracle's own top-2 logit gap is below 2e-4, and on
the committed inputs there is none (`ties == 0`).  Everything that compares two engine runs is bit for bit.

The oracle (oracle/dt_ref.py) knows one head mode and one observation kind per call: a mixed batch is checked by driving one
OraclePolicy per (observation kind, head mode) group on that group's slots -- env slots are independent.

Inputs of the oracle tests: slot kinds cyclic over (vector, continuous, act_dim), (vector, discrete), (image, discrete),
(image, continuous, 2), (vector, continuous, 1), (vector, continuous, 3); weights init_state_dict(spec, seed=41,
with_image_encoder=True); make_inputs(spec, 24, 8, 20261020) for vectors / rtg / reward / reset masks and seed + 1 with
image=True for frames.  On these the oracle ALONE keeps its smallest top-2 gap over the compared rows at 1.45e-3 (xLSTM d128,
2 blocks) and 1.13e-3 (mamba_tiny), more than five times the 2e-4 tie rule (seeds 20261016 / 18 / 19 put the oracle itself
inside or next to the rule on one model or the other and are not used)."""
import pytest
import torch

from lram_amd import init_state_dict, preset
from lram_amd.config import ModelSpec
from oracle.dt_ref import OraclePolicy
from tests.helpers import assert_actions_match, make_inputs, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 20261020
HID_TOL = 2e-4
KINDS = lambda A: [(0, 0, A), (0, 1, 1), (1, 1, 1), (1, 0, 2), (0, 0, 1), (0, 0, 3)]   # (image, discrete, act_dim), cyclic


def _spec(model):
    if model == "xlstm_d128":
        return ModelSpec(backbone="xlstm", d_model=128, n_blocks=2, slstm_at=[1], state_dim=20, act_dim=4)
    return preset(model)


def _kinds(spec, B):
    k = KINDS(spec.act_dim)
    return [k[b % len(k)] for b in range(B)]


def _set(eng, kinds):
    eng.set_slot_table([bool(k[1]) for k in kinds], [k[2] for k in kinds], [bool(k[0]) for k in kinds])


def _engine(spec, sd, B):
    from lram_amd.engine import Engine
    return Engine(spec, sd, B, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(x, y, what):
    assert x.shape == y.shape and torch.equal(_bits(x), _bits(y)), f"{what}: {int((_bits(x) != _bits(y)).sum())} of {x.numel()} words differ"


def _snap(eng, a, tok):
    torch.cuda.synchronize()
    _, hid, lg = eng.taps()
    return a.clone(), tok.clone(), hid, lg


def _image_rows(kinds):
    return [b for b, k in enumerate(kinds) if k[0]]


def _defined(kinds, A):
    """bool [B, A]: the action columns the table defines."""
    m = torch.zeros(len(kinds), A, dtype=torch.bool)
    for b, k in enumerate(kinds):
        m[b, : k[2]] = True
    return m


def _check_fill(a, tok, kinds, what):
    m = _defined(kinds, a.shape[1]).to(a.device)
    assert torch.equal(_bits(a[~m]), torch.zeros_like(_bits(a[~m]))), f"{what}: an unused action column is not +0.0"
    assert bool((tok[~m] == -1).all()), f"{what}: an unused token column is not -1"
    assert bool((tok[m] >= 0).all()), f"{what}: a defined token is negative"


# ---- 1. degenerate tables are the existing calls, bit for bit ------------------------------------------------------------
def _pair_runs(spec, sd, B, steps, kinds, plain, what, seed=1234, image=False):
    """The same inputs through step_slots with `kinds` and through the plain call `plain(eng, obs, rtg, rew, mask)`; outputs,
    logits tap and hidden tap equal on the defined columns at every step."""
    seq = make_inputs(spec, B, steps, seed=seed, image=image)
    e1, e2 = _engine(spec, sd, B), _engine(spec, sd, B)
    _set(e1, kinds)
    m = _defined(kinds, spec.act_dim).to(DEV)
    junk = torch.full((B, spec.state_dim), float("nan"), device=DEV)
    for t, (obs, rtg, rew, mask) in enumerate(seq):
        obs, rtg, rew, mask = obs.to(DEV), rtg.to(DEV), rew.to(DEV), mask.to(DEV)
        if image:
            a1, t1, h1, l1 = _snap(e1, *e1.step_slots(junk if t % 2 else None, obs, rtg, rew, mask))
        else:
            a1, t1, h1, l1 = _snap(e1, *e1.step_slots(obs, None, rtg, rew, mask))
        a2, t2, h2, l2 = _snap(e2, *plain(e2, obs, rtg, rew, mask))
        _same(h1, h2, f"{what} step {t}: hidden tap")
        _same(l1, l2, f"{what} step {t}: logits tap")
        _same(a1[m], a2[m], f"{what} step {t}: actions")
        _same(t1[m], t2[m], f"{what} step {t}: tokens")
        _check_fill(a1, t1, kinds, f"{what} step {t}")
    e1.close(), e2.close()


@pytest.mark.parametrize("model", ["xlstm_tiny", "mamba_tiny"])
def test_degenerate_tables_equal_the_existing_calls(hip_lib, model):
    spec = preset(model)
    sd = init_state_dict(spec, seed=41, with_image_encoder=True)
    B, A = 12, spec.act_dim
    _pair_runs(spec, sd, B, 6, [(0, 0, A)] * B, lambda e, o, g, r, m: e.step(o, g, r, m, discrete=False), f"{model} all-vector continuous")
    _pair_runs(spec, sd, B, 6, [(0, 1, 1)] * B, lambda e, o, g, r, m: e.step(o, g, r, m, discrete=True), f"{model} all-vector discrete")
    _pair_runs(spec, sd, B, 6, [(1, 1, 1)] * B, lambda e, o, g, r, m: e.step_images(o, g, r, m, discrete=True),
               f"{model} all-image discrete", image=True)
    _pair_runs(spec, sd, B, 6, [(1, 0, A)] * B, lambda e, o, g, r, m: e.step_images(o, g, r, m, discrete=False),
               f"{model} all-image continuous", image=True)


@pytest.mark.parametrize("model", ["xlstm_tiny", "mamba_tiny"])
def test_per_slot_head_with_a_uniform_table_equals_the_scalar_heads(hip_lib, model):
    """discrete="per_slot" through step / step_images / prefill (the observation kind is the call's own) against discrete = 0 / 1."""
    spec = preset(model)
    sd = init_state_dict(spec, seed=41, with_image_encoder=True)
    B, A = 12, spec.act_dim
    for disc in (False, True):
        kinds = [(0, int(disc), 1 if disc else A)] * B
        m = _defined(kinds, A).to(DEV)
        for image in (False, True):
            seq = make_inputs(spec, B, 6, seed=77, image=image)
            e1, e2 = _engine(spec, sd, B), _engine(spec, sd, B)
            _set(e1, kinds)
            call = (lambda e, *a, **k: e.step_images(*a, **k)) if image else (lambda e, *a, **k: e.step(*a, **k))
            for t, inp in enumerate(seq):
                obs, rtg, rew, mask = (x.to(DEV) for x in inp)
                a1, t1, h1, l1 = _snap(e1, *call(e1, obs, rtg, rew, mask, discrete="per_slot"))
                a2, t2, h2, l2 = _snap(e2, *call(e2, obs, rtg, rew, mask, discrete=disc))
                what = f"{model} discrete={disc} image={image} step {t}"
                _same(h1, h2, what + ": hidden"), _same(l1, l2, what + ": logits")
                _same(a1[m], a2[m], what + ": actions"), _same(t1[m], t2[m], what + ": tokens")
                _check_fill(a1, t1, kinds, what)
            if not image:   # prefill: head of the last timestep
                ctx = make_inputs(spec, B, 5, seed=78)
                obs_seq = torch.stack([c[0] for c in ctx], 1).to(DEV).contiguous()
                rtg_seq = torch.stack([c[1] for c in ctx], 1).to(DEV).contiguous()
                rew_seq = torch.stack([c[2] for c in ctx], 1).to(DEV).contiguous()
                full = torch.ones(B, dtype=torch.uint8, device=DEV)
                a1, t1 = (x.clone() for x in e1.prefill(obs_seq, rtg_seq, rew_seq, full, discrete="per_slot"))
                a2, t2 = (x.clone() for x in e2.prefill(obs_seq, rtg_seq, rew_seq, full, discrete=disc))
                _same(a1[m], a2[m], f"{model} discrete={disc}: prefill actions"), _same(t1[m], t2[m], f"{model} discrete={disc}: prefill tokens")
                _check_fill(a1, t1, kinds, f"{model} discrete={disc}: prefill")
            e1.close(), e2.close()


def test_all_vector_table_equals_step_at_the_headline_configuration(hip_lib):
    """16M, 4096 slots, lazy matrix memory, two env slices (the automatic choices): lram_step_slots with an all-vector table
    against lram_step."""
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=41)
    B, A = 4096, spec.act_dim
    outs = []
    for use_table in (True, False):
        eng = _engine(spec, sd, B)
        assert eng.state_mode == "lazy"
        if use_table:
            _set(eng, [(0, 0, A)] * B)
        run = []
        for t, inp in enumerate(make_inputs(spec, B, 6, seed=4096)):
            obs, rtg, rew, mask = (x.to(DEV) for x in inp)
            a, tok = eng.step_slots(obs, None, rtg, rew, mask) if use_table else eng.step(obs, rtg, rew, mask)
            torch.cuda.synchronize()
            _, hid, lg = eng.taps()
            run.append((a.cpu(), tok.cpu(), hid.cpu(), lg.cpu()))
        outs.append(run)
        eng.close()
        torch.cuda.empty_cache()
    for t, (x, y) in enumerate(zip(*outs)):
        for name, u, v in zip(("actions", "tokens", "hidden", "logits"), x, y):
            _same(u, v, f"headline step {t}: {name}")


# ---- 2. the per-slot head is the homogeneous heads, slot by slot ---------------------------------------------------------------
@pytest.mark.parametrize("sampling", [False, True])
def test_mixed_head_table_equals_the_homogeneous_heads(hip_lib, sampling):
    spec = preset("xlstm_tiny")
    sd = init_state_dict(spec, seed=41)
    B, A = 12, spec.act_dim
    kinds = [(0, k[1], k[2]) for k in _kinds(spec, B)]          # the cyclic head kinds, all-vector observations
    engs = [_engine(spec, sd, B) for _ in range(3)]             # per-slot, continuous, discrete
    _set(engs[0], kinds)
    if sampling:
        for e in engs:
            e.set_sampling(temperature=0.75, top_k=5, top_p=0.5, seed=20261016)
    seq = make_inputs(spec, B, 4, seed=99)
    for t, inp in enumerate(seq):
        obs, rtg, rew, mask = (x.to(DEV) for x in inp)
        if t == 2:   # a table change between steps takes effect on the next call, and reads back
            kinds = kinds[1:] + kinds[:1]
            _set(engs[0], kinds)
            tab = engs[0].slot_table()
            assert tab["discrete"].tolist() == [bool(k[1]) for k in kinds] and tab["act_dim"].tolist() == [k[2] for k in kinds]
            assert tab["image"].tolist() == [False] * B and tab["n_image"] == 0
        am, tm = (x.clone() for x in engs[0].step(obs, rtg, rew, mask, discrete="per_slot"))
        ac, tc = (x.clone() for x in engs[1].step(obs, rtg, rew, mask, discrete=False))
        ad, td = (x.clone() for x in engs[2].step(obs, rtg, rew, mask, discrete=True))
        torch.cuda.synchronize()
        taps = [e.taps() for e in engs]
        for k in (1, 2):   # the head does not feed back: the recurrent state is the same in all three
            _same(taps[0][1], taps[k][1], f"step {t}: hidden tap"), _same(taps[0][2], taps[k][2], f"step {t}: logits tap")
        for b, (_, disc, n) in enumerate(kinds):
            if disc:
                _same(am[b, :1], ad[b, :1], f"step {t} slot {b}: discrete action"), _same(tm[b, :1], td[b, :1], f"step {t} slot {b}: discrete token")
                assert 0 <= int(tm[b, 0]) < spec.n_discrete
            else:
                _same(am[b, :n], ac[b, :n], f"step {t} slot {b}: continuous actions"), _same(tm[b, :n], tc[b, :n], f"step {t} slot {b}: tokens")
        _check_fill(am, tm, kinds, f"step {t}")
    if sampling:
        assert [e.sampling["draws"] for e in engs] == [4, 4, 4]
    for e in engs:
        e.close()


# ---- 3. mixed observations against the oracle -------------------------------------------------------------------------------------
def _oracle_groups(kinds, rows=None):
    groups = {}
    for b, (im, di, _) in enumerate(kinds):
        if rows is None or b in rows:
            groups.setdefault((im, di), []).append(b)
    return groups


def _frames_of(img_obs, kinds):
    return img_obs[torch.tensor(_image_rows(kinds), dtype=torch.long)].contiguous()


def _check_against_oracle(spec, oracles, groups, kinds, vec_t, img_t, a, hid, what, dbg_out=None):
    """One step: the engine's actions / hidden tap (host tensors, all slots) against one oracle per group.  dbg_out: a dict
    that receives every group's oracle debug tensors, for callers that check more taps."""
    _, rtg, rew, mask = vec_t
    ties, worst = 0, 0.0
    for (im, di), idx in groups.items():
        ix = torch.tensor(idx)
        obs = (img_t if im else vec_t)[0][ix]
        a_ref, dbg = oracles[(im, di)].step(obs, rtg[ix], rew[ix], mask[ix], discrete=bool(di), return_debug=True)
        got = a[ix]
        if dbg_out is not None:
            dbg_out[(im, di)] = dbg
        if di:
            ties += assert_actions_match(got[:, :1], a_ref, dbg["logits"], spec, discrete=True, what=f"{what} group {(im, di)}")
        else:
            own = _defined([kinds[b] for b in idx], spec.act_dim)
            got = torch.where(own, got, a_ref.float())            # only the action dims the slot uses are compared
            ties += assert_actions_match(got, a_ref, dbg["logits"], spec, discrete=False, what=f"{what} group {(im, di)}")
        err = rel_err(hid[ix], dbg["hidden"])
        worst = max(worst, err)
        assert err < HID_TOL, f"{what} group {(im, di)}: hidden rel err {err:.3e}"
    return ties, worst


@pytest.mark.parametrize("model", ["xlstm_d128", "mamba_tiny"])
def test_mixed_batch_against_the_oracle(hip_lib, model):
    spec = _spec(model)
    sd = init_state_dict(spec, seed=41, with_image_encoder=True)
    B, steps = 24, 8
    kinds = _kinds(spec, B)
    vec = make_inputs(spec, B, steps, seed=SEED)
    img = make_inputs(spec, B, steps, seed=SEED + 1, image=True)
    groups = _oracle_groups(kinds)
    assert sorted(groups) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    oracles = {k: OraclePolicy(spec, sd) for k in groups}
    eng = _engine(spec, sd, B)
    _set(eng, kinds)
    assert eng.n_image_slots == len(_image_rows(kinds)) == 8
    ties, worst = 0, 0.0
    for t in range(steps):
        obs, rtg, rew, mask = (x.to(DEV) for x in vec[t])
        a, tok = eng.step_slots(obs, _frames_of(img[t][0], kinds).to(DEV), rtg, rew, mask)
        torch.cuda.synchronize()
        _, hid, _ = eng.taps()
        _check_fill(a, tok, kinds, f"{model} step {t}")
        n, w = _check_against_oracle(spec, oracles, groups, kinds, vec[t], img[t], a.cpu(), hid.cpu(), f"{model} step {t}")
        ties, worst = ties + n, max(worst, w)
    print(f"{model}: mixed batch vs oracle, worst hidden rel err {worst:.3e}, ties {ties}")
    assert ties == 0
    eng.close()


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------------
def test_mixed_batch_isolation(hip_lib):
    spec = _spec("xlstm_d128")
    sd = init_state_dict(spec, seed=41, with_image_encoder=True)
    B, steps = 24, 4
    kinds = _kinds(spec, B)
    img_rows = torch.tensor(_image_rows(kinds))
    vec = make_inputs(spec, B, steps, seed=SEED)
    img = make_inputs(spec, B, steps, seed=SEED + 1, image=True)

    def run(fill=None, edit=None, swap=None):
        eng = _engine(spec, sd, B)
        _set(eng, kinds)
        out = []
        for t in range(steps):
            obs, rtg, rew, mask = (x.clone() for x in vec[t])
            frames = _frames_of(img[t][0], kinds)
            if fill is not None:
                obs[img_rows] = fill(len(img_rows), spec.state_dim)
            if edit is not None and t == 1:
                obs[edit] = obs[edit] + 0.25
            if swap is not None and t == 0:
                frames[list(swap)] = frames[list(reversed(swap))]
            a, tok = eng.step_slots(obs.to(DEV), frames.to(DEV), rtg.to(DEV), rew.to(DEV), mask.to(DEV))
            out.append(tuple(x.cpu() for x in _snap(eng, a, tok)))
        eng.close()
        return out

    base = run()
    nonfinite = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38])
    poisoned = run(fill=lambda n, d: nonfinite[torch.arange(n * d) % 4].reshape(n, d))
    zeros = run(fill=lambda n, d: torch.zeros(n, d))
    for name, other in (("NaN / Inf", poisoned), ("zero", zeros)):
        for t in range(steps):
            for k, what in enumerate(("actions", "tokens", "hidden", "logits")):
                _same(base[t][k], other[t][k], f"{name} rows under the image slots, step {t}: {what}")
    # one vector slot's observation changes nothing outside that slot
    slot = 4
    assert not kinds[slot][0]
    edited = run(edit=slot)
    others = torch.arange(B) != slot
    changed = False
    for t in range(steps):
        for k, what in enumerate(("actions", "tokens", "hidden", "logits")):
            _same(base[t][k][others], edited[t][k][others], f"edited slot {slot}, step {t}: {what} of the other slots")
        changed |= not torch.equal(base[t][2][slot], edited[t][2][slot])
    assert changed, "the edit did not reach its own slot"
    # frames are matched to slots by ascending slot order: swapping frames i and j swaps exactly those two slots' results at step 0
    i, j = 1, 5
    bi, bj = int(img_rows[i]), int(img_rows[j])
    swapped = run(swap=(i, j))
    rest = torch.ones(B, dtype=torch.bool)
    rest[[bi, bj]] = False
    for k, what in ((2, "hidden"), (3, "logits")):
        _same(base[0][k][rest], swapped[0][k][rest], f"frame swap: {what} of the other slots")
        _same(base[0][k][bi], swapped[0][k][bj], f"frame swap: {what} of slot {bi} -> {bj}")
        _same(base[0][k][bj], swapped[0][k][bi], f"frame swap: {what} of slot {bj} -> {bi}")
    assert not torch.equal(base[0][2][bi], base[0][2][bj])


# ---- 5. production size ---------------------------------------------------------------------------------------------------------
def _production_kinds(B, A, image_slots):
    img = set(image_slots)
    out = []
    for b in range(B):
        if b in img:
            out.append((1, 1, 1) if (b // 2) % 2 == 0 else (1, 0, 2))
        else:
            out.append((0, 1, 1) if b % 3 == 1 else (0, 0, A if b % 3 == 0 else 3))
    return out


@pytest.mark.parametrize("variant", ["straddle", "one_slice_without_frames"])
def test_mixed_batch_at_production_size(hip_lib, variant):
    """16M with an image encoder, 4096 slots, lazy, two env slices (2048 + 2048).  96 image slots: `straddle` puts 48 either
    side of the slice boundary (slots 2000 .. 2095); in the other variant all 96 sit in the second slice (the first launches no
    CNN)."""
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=41, with_image_encoder=True)
    B, A, steps = 4096, spec.act_dim, 6
    image_slots = list(range(2000, 2096)) if variant == "straddle" else list(range(2048, 2048 + 192, 2))
    kinds = _production_kinds(B, A, image_slots)
    first = sum(1 for b in image_slots if b < 2048)
    assert len(image_slots) == 96 and first == (48 if variant == "straddle" else 0)
    # 16 sampled slots: both slices, all four (observation, head) kinds
    want = {(im, di): 2 for im in (0, 1) for di in (0, 1)}
    sample = []
    for lo, hi in ((0, 2048), (2048, B)):
        need = dict(want)
        cand = [b for b in image_slots if lo <= b < hi] + list(range(lo + 5, hi, 97))
        for b in cand:
            k = kinds[b][:2]
            if need.get(k, 0) > 0:
                need[k] -= 1
                sample.append(b)
    if variant == "straddle":
        assert len(sample) == 16
    else:   # no image slot in the first slice: 4 + 8
        assert len(sample) == 12
        sample += [b for b in range(2100, B, 211) if b not in sample][:4]
    sample = sorted(sample)
    groups = _oracle_groups(kinds, rows=set(sample))
    assert len(groups) == 4
    g = torch.Generator().manual_seed(SEED)
    runs = []
    inputs = []
    rtg = torch.full((B,), 4.5)
    for t in range(steps):
        obs = torch.zeros(B, spec.state_dim)
        obs[:, : spec.state_dim * 3 // 4] = torch.rand(B, spec.state_dim * 3 // 4, generator=g) * 2 - 1
        frames = torch.randint(0, 256, (len(image_slots), *spec.image_shape), generator=g, dtype=torch.uint8)
        mask = (torch.rand(B, generator=g) < 0.15).to(torch.uint8) if t > 0 else torch.ones(B, dtype=torch.uint8)
        rtg = torch.where(mask.bool(), torch.full_like(rtg, 4.5), rtg - 0.01)
        inputs.append((obs, frames, rtg.clone(), torch.zeros(B), mask))
    for rep in range(2):
        eng = _engine(spec, sd, B)
        assert eng.state_mode == "lazy"
        _set(eng, kinds)
        assert eng.n_image_slots == 96
        run = []
        for obs, frames, r, rew, mask in inputs:
            a, tok = eng.step_slots(obs.to(DEV), frames.to(DEV), r.to(DEV), rew.to(DEV), mask.to(DEV))
            torch.cuda.synchronize()
            _, hid, _ = eng.taps()
            run.append((a.cpu(), tok.cpu(), hid.cpu()))
        runs.append(run)
        eng.close()
        torch.cuda.empty_cache()
    oracles = {k: OraclePolicy(spec, sd) for k in groups}
    ties, worst = 0, 0.0
    rest = torch.ones(B, dtype=torch.bool)
    rest[sample] = False
    for t, (obs, frames, r, rew, mask) in enumerate(inputs):
        a, tok, hid = runs[0][t]
        _check_fill(a, tok, kinds, f"{variant} step {t}")
        # frames scattered to a [B, ...] tensor so that the per-group indexing of the oracle helper applies
        img_full = torch.zeros(B, *spec.image_shape, dtype=torch.uint8)
        img_full[torch.tensor(image_slots)] = frames
        n, w = _check_against_oracle(spec, oracles, groups, kinds, (obs, r, rew, mask), (img_full,), a, hid, f"{variant} step {t}")
        ties, worst = ties + n, max(worst, w)
        for k, what in enumerate(("actions", "tokens", "hidden")):   # determinism: every other slot, bit for bit
            _same(runs[0][t][k][rest], runs[1][t][k][rest], f"{variant} step {t}: {what} of two runs")
    print(f"{variant}: 16 sampled slots vs oracle, worst hidden rel err {worst:.3e}, ties {ties}")
    assert ties == 0


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(hip_lib):
    from lram_amd.engine import LramError
    spec = preset("mamba_tiny")
    A, B = spec.act_dim, 6
    sd = init_state_dict(spec, seed=41)                       # no image encoder
    eng = _engine(spec, sd, B)
    obs, rtg, rew, mask = (x.to(DEV) for x in make_inputs(spec, B, 1, seed=5)[0])
    frames = torch.zeros(2, *spec.image_shape, dtype=torch.uint8, device=DEV)

    def refused(fn, text):
        with pytest.raises(LramError) as ei:
            fn()
        assert text in str(ei.value), str(ei.value)

    # no table yet
    refused(lambda: eng.step(obs, rtg, rew, mask, discrete="per_slot"), "slot table")
    refused(lambda: eng.prefill(obs.view(B, 1, -1), rtg.view(B, 1), rew.view(B, 1), mask, discrete="per_slot"), "slot table")
    assert eng.slot_table() is None
    rc = hip_lib.lram_step_slots(eng._h, obs.data_ptr(), None, 0, 0, 0, rtg.data_ptr(), rew.data_ptr(), None,
                                 eng._actions.data_ptr(), None, None)
    assert rc != 0 and b"no slot table" in hip_lib.lram_last_error()
    # tables the engine refuses: act_dim out of range, a discrete slot with act_dim != 1
    refused(lambda: eng.set_slot_table([False] * B, [A + 1] + [1] * (B - 1), None), "act_dim")
    refused(lambda: eng.set_slot_table([False] * B, [0] + [1] * (B - 1), None), "act_dim")
    refused(lambda: eng.set_slot_table([True] + [False] * (B - 1), [2] + [1] * (B - 1), None), "discrete slot")
    assert eng.slot_table() is None                            # a refused table changes nothing
    with pytest.raises(ValueError):
        eng.set_slot_table([False] * (B - 1), [1] * (B - 1), None)
    # image slots without embed_image.* weights: at the first call that needs them
    eng.set_slot_table([False] * B, [A] * B, [True, True] + [False] * (B - 2))
    refused(lambda: eng.step_slots(obs, frames, rtg, rew, mask), "embed_image")
    with pytest.raises(ValueError):
        eng.step_slots(obs, frames[:1], rtg, rew, mask)        # frame count != the table's image count
    # sampling armed with top_k > n_discrete while the table holds a discrete slot: at that call
    eng.set_slot_table([True] + [False] * (B - 1), [1] + [A] * (B - 1), None)
    eng.set_sampling(temperature=1.0, top_k=spec.n_discrete + 1, top_p=0.0, seed=1)
    refused(lambda: eng.step(obs, rtg, rew, mask, discrete="per_slot"), "top_k")
    refused(lambda: eng.step_slots(obs, None, rtg, rew, mask), "top_k")
    eng.set_sampling(None)
    # the Mamba repeated-forward mode
    eng.set_compat_mode(2, False)
    refused(lambda: eng.step(obs, rtg, rew, mask, discrete="per_slot"), "repeated-forward")
    refused(lambda: eng.step_slots(obs, None, rtg, rew, mask), "repeated-forward")
    eng.set_compat_mode(1, False)
    # ... and after all of it the engine still steps, as a fresh one does
    eng.reset()
    a, tok = (x.clone() for x in eng.step_slots(obs, None, rtg, rew, mask))
    fresh = _engine(spec, sd, B)
    a2, t2 = fresh.step(obs, rtg, rew, mask, discrete=False)
    _same(a[1:], a2[1:], "after the refusals: continuous slots")
    fresh.reset()
    a3, t3 = fresh.step(obs, rtg, rew, mask, discrete=True)
    _same(a[:1, :1], a3[:1, :1], "after the refusals: the discrete slot")
    # lram_state_alloc clears the table
    eng.alloc(B)
    assert eng.slot_table() is None
    eng.close(), fresh.close()
    # a model without discrete actions (n_discrete == 0) takes no discrete slot
    import dataclasses
    spec0 = dataclasses.replace(spec, n_discrete=0)
    e0 = _engine(spec0, init_state_dict(spec0, seed=41), 2)
    refused(lambda: e0.set_slot_table([True, False], [1, 1], None), "n_discrete")
    e0.set_slot_table([False, False], [1, A], None)
    e0.close()


# ---- 7. pad_obs_slots -----------------------------------------------------------------------------------------------------------
def test_pad_obs_slots(hip_lib):
    from lram_amd.engine import pad_obs, pad_obs_slots
    from lram_amd.obs import CHEETAH_RUN_SPEC, apply_inverse_index, dmc_inverse_index
    S, n, B = 204, 17, 37
    g = torch.Generator().manual_seed(7)
    native = (torch.rand(B, n, generator=g) * 2 - 1).to(DEV)
    dmc = dmc_inverse_index(CHEETAH_RUN_SPEC, S)
    pad = torch.where(torch.arange(S) < n, torch.arange(S), torch.full((S,), -1)).to(torch.int32)   # zero-pad as an index row
    inv = torch.stack([dmc, pad, dmc.flip(0)]).to(DEV).contiguous()
    mean = (torch.rand(3, S, generator=g) - 0.5).to(DEV)
    std = (torch.rand(3, S, generator=g) + 0.5).to(DEV)
    rows = (torch.arange(B) * 7 % 3).to(torch.int32).to(DEV)
    for norm in (False, True):
        m, s = (mean, std) if norm else (None, None)
        got = pad_obs_slots(native, S, rows, inv, m, s)
        for r in range(3):   # per group of slots sharing a row: the existing call, bit for bit
            sel = (rows == r).nonzero().view(-1)
            want = pad_obs(native[sel].contiguous(), S, inv[r].contiguous(), None if m is None else m[r].contiguous(),
                           None if s is None else s[r].contiguous())
            _same(got[sel], want, f"row {r} norm={norm}")
        # n_rows = 1, all-zero slot rows: the existing call
        zero = torch.zeros(B, dtype=torch.int32, device=DEV)
        one = pad_obs_slots(native, S, zero, inv[:1].contiguous(), None if m is None else m[:1].contiguous(),
                            None if s is None else s[:1].contiguous())
        _same(one, pad_obs(native, S, inv[0].contiguous(), None if m is None else m[0].contiguous(),
                           None if s is None else s[0].contiguous()), f"n_rows = 1 norm={norm}")
    # no index table: zero-pad for every slot, with per-slot normalisation rows
    _same(pad_obs_slots(native, S, torch.zeros(B, dtype=torch.int32, device=DEV), None), pad_obs(native, S), "zero-pad, no tables")
    # a DMControl row and a zero-pad row in one batch against the host statement of the mapping
    two = (torch.arange(B) % 2).to(torch.int32).to(DEV)
    got = pad_obs_slots(native, S, two, inv[:2].contiguous()).cpu()
    host = native.cpu()
    assert torch.equal(got[0::2], apply_inverse_index(host[0::2], dmc))
    assert torch.equal(got[1::2], torch.cat([host[1::2], torch.zeros(host[1::2].shape[0], S - n)], dim=1))
    # a slot row outside the tables gives zeros, never a read outside them
    wild = two.clone()
    wild[3], wild[4] = 2, -1
    got = pad_obs_slots(native, S, wild, inv[:2].contiguous()).cpu()
    assert not got[3].any() and not got[4].any() and torch.equal(got[5], apply_inverse_index(host[5:6], pad)[0])


# ---- 8. agent level -------------------------------------------------------------------------------------------------------------
def test_mixed_rollout_through_the_agent_against_the_oracle(hip_lib):
    """Two SyntheticVecEnvs -- image-discrete and vector-continuous -- concatenated into one BatchedRollout over two episode ends
    per slot; per-slot rtg follows rtg - r / reward_scale[b]."""
    from lram_amd.agent import RecurrentAgent
    from lram_amd.domains import Domain, SlotTable
    from lram_amd.rollout import BatchedRollout, SyntheticVecEnv
    spec = _spec("xlstm_d128")
    sd = init_state_dict(spec, seed=41, with_image_encoder=True)
    n_img, n_vec, ep_len, steps = 3, 5, 3, 8
    tab = SlotTable.from_domains([(Domain("procgen", True, 1, image=True, reward_scale=2.0, target_return=9.0), n_img),
                                  (Domain("metaworld", False, 3, reward_scale=8.0, target_return=36.0), n_vec)],
                                 max_act_dim=spec.act_dim)
    B = tab.n_slots

    class MixedEnv:
        """The two vector envs side by side: observations as the pair (vector rows for every slot, frames of the image slots)."""
        def __init__(self):
            self.img = SyntheticVecEnv(n_img, ep_len=ep_len, image_shape=spec.image_shape, seed=SEED, stagger=True)
            self.vec = SyntheticVecEnv(n_vec, obs_dim=12, act_dim=3, ep_len=ep_len, seed=SEED + 1, stagger=True)
            self.n_envs, self.device = B, torch.device("cpu")

        def _pair(self, frames, v):
            return (torch.cat([torch.zeros(n_img, v.shape[1]), v]), frames)

        def reset(self):
            return self._pair(self.img.reset(), self.vec.reset())

        def step(self, actions):
            f, r1, d1 = self.img.step(actions[:n_img])
            v, r2, d2 = self.vec.step(actions[n_img:])
            return self._pair(f, v), torch.cat([r1, r2]), torch.cat([d1, d2])

    agent = RecurrentAgent(spec, sd, n_envs=B, device=DEV, slot_table=tab)
    assert agent.slot_is_discrete.tolist() == [True] * n_img + [False] * n_vec
    ro = BatchedRollout(agent, MixedEnv(), tab.target_return, tab.reward_scale)
    kinds = [(1, 1, 1)] * n_img + [(0, 0, 3)] * n_vec
    groups = _oracle_groups(kinds)
    oracles = {k: OraclePolicy(spec, sd) for k in groups}
    ties, ends = 0, torch.zeros(B)
    want_rtg = tab.rtg0.clone()
    for t in range(steps):
        (vec_obs, frames), rtg, mask = ro.obs, ro.rtg.clone(), ro.reset_mask.clone()
        assert torch.equal(rtg, want_rtg), f"step {t}: per-slot rtg"
        a = ro.step().cpu().clone()
        torch.cuda.synchronize()
        _, hid, _ = agent.engine.taps()
        padded = torch.cat([vec_obs, torch.zeros(B, spec.state_dim - vec_obs.shape[1])], dim=1)
        img_full = torch.zeros(B, *spec.image_shape, dtype=torch.uint8)
        img_full[:n_img] = frames
        n, _ = _check_against_oracle(spec, oracles, groups, kinds, (padded, rtg, torch.zeros(B), mask), (img_full,), a, hid.cpu(),
                                     f"agent step {t}")
        ties += n
        assert not a[:n_img, 1:].any() and not a[n_img:, 3:].any()
        done = ro.last_done
        ends += done.float()
        want_rtg = torch.where(done, tab.rtg0, want_rtg - ro.last_reward / tab.reward_scale.float())
    assert ties == 0 and bool((ends >= 2).all()), ends.tolist()
    agent.engine.close()
