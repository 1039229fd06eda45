"""After any kind of call, the next plain Engine.step depends only on the recurrent state and its own arguments.

Engine A runs two plain steps and then a call X of another kind (frames, a mixed batch, a stored context through the chunk
lanes, a refused call, repeated forwards).  A's state goes through save_slots(all) / load_slots into a fresh engine B with the
same weights, which has never seen X; both then run the same plain step.  Actions, tokens and the hidden tap must be equal bit
for bit: nothing X was given (frames, slot kinds, pass counts, lane events, a workspace swap) may outlive the call.

Materialised state (the automatic choice at 8 env slots), so both engines run the same kernels on the same state bits -- the
exactness tests/test_gpu_slot_state.py::test_round_trip_and_migration already holds the records to."""
import pytest
import torch

from lram_amd import init_state_dict, preset
from tests.helpers import make_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 8
IMAGE_SLOTS, DISCRETE_SLOTS = (0, 3, 6), (1, 4)   # 3 image slots, 5 vector slots, 2 of them discrete


def _dev(step):
    return tuple(x.to(DEV) for x in step)


def _set_table(eng, spec):
    disc = [b in DISCRETE_SLOTS for b in range(B)]
    act = [1 if d else spec.act_dim for d in disc]
    eng.set_slot_table(disc, act, [b in IMAGE_SLOTS for b in range(B)])


def _x_step_images(eng, spec, seq, img):
    frames, rtg, rew, mask = _dev(img)
    eng.step_images(frames, rtg, rew, mask)


def _x_step_slots(eng, spec, seq, img):
    _set_table(eng, spec)
    obs, rtg, rew, mask = _dev(seq[2])
    eng.step_slots(obs, _dev(img)[0][list(IMAGE_SLOTS)].contiguous(), rtg, rew, mask)


def _x_prefill(eng, spec, seq, img):
    steps = [_dev(s) for s in seq[2:11]]   # 9 timesteps: three chunks of the token-sequential path
    eng.prefill(torch.stack([s[0] for s in steps], 1).contiguous(), torch.stack([s[1] for s in steps], 1).contiguous(),
                torch.stack([s[2] for s in steps], 1).contiguous(), steps[0][3])


def _x_refused_step_slots(eng, spec, seq, img):
    from lram_amd.engine import _ptr, _stream_ptr
    _set_table(eng, spec)
    obs, rtg, rew, mask = _dev(seq[2])
    with pytest.raises((ValueError, RuntimeError)):
        eng.step_slots(obs, None, rtg, rew, mask)
    # ... and the library's own refusal of the same call (the wrapper above refuses before it reaches the library)
    a = torch.empty(B, spec.act_dim, dtype=torch.float32, device=DEV)
    tok = torch.empty(B, spec.act_dim, dtype=torch.int32, device=DEV)
    rc = eng.lib.lram_step_slots(eng._h, _ptr(obs), None, 0, 0, 0, _ptr(rtg), _ptr(rew), _ptr(mask), _ptr(a), _ptr(tok),
                                 _stream_ptr(eng.device))
    assert rc != 0 and b"frames needed" in eng.lib.lram_last_error()


def _x_compat_repeat(eng, spec, seq, img):
    eng.set_compat_mode(mamba_repeat=4)
    eng.step(*_dev(seq[2]))
    eng.set_compat_mode(1)


CASES = {
    "step_images": ("xlstm_tiny", _x_step_images),
    "step_slots": ("xlstm_tiny", _x_step_slots),
    "prefill_9": ("xlstm_tiny", _x_prefill),
    "refused_step_slots": ("xlstm_tiny", _x_refused_step_slots),
    "mamba_repeat_4": ("mamba_tiny", _x_compat_repeat),
}


@pytest.mark.parametrize("case", list(CASES))
def test_next_plain_step_depends_on_state_and_arguments_only(hip_lib, case):
    from lram_amd.engine import Engine
    model, call_x = CASES[case]
    spec = preset(model)
    sd = init_state_dict(spec, seed=97, with_image_encoder=True)
    seq = make_inputs(spec, B, 12, seed=4242, reset_prob=0.1)
    img = make_inputs(spec, B, 1, seed=4243, image=True)[0]
    last = _dev(seq[11])
    last[3].zero_()   # the compared step resets nothing: it reads every slot's migrated state
    ea, eb = Engine(spec, sd, B, device=DEV), Engine(spec, sd, B, device=DEV)
    assert ea.state_mode == eb.state_mode == "materialised"
    for t in range(2):
        ea.step(*_dev(seq[t]))
    call_x(ea, spec, seq, img)
    eb.load_slots(list(range(B)), ea.save_slots(list(range(B))))
    out = []
    for eng in (ea, eb):
        a, tok = eng.step(*last)
        torch.cuda.synchronize()
        out.append((a.clone(), tok.clone(), eng.taps()[1]))
    for k, what in enumerate(("actions", "tokens", "hidden tap")):
        x, y = out[0][k], out[1][k]
        assert not bool(torch.isnan(x.float()).any()), f"{case}: NaN in {what}"
        assert x.shape == y.shape and torch.equal(x, y), f"{case}: {what} of the step after the call differ from a fresh engine's"
    ea.close(), eb.close()
