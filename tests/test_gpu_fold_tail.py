"""Tail fold (csrc/engine_xlstm.hip): with two env slices the first mLSTM block's fold of step n + 1 runs at the end of step n,
behind the last read pass on the state-pass stream, and step n + 1 skips that launch.  The fold's arithmetic and its inputs are
the same, so everything is compared BIT FOR BIT (torch.equal) between an engine created with LRAM_FOLD_TAIL=0 (the schedule
without it) and one with the default: actions and tokens of every step, and the exported C / n / m of every mLSTM block at the end.
Every entry other than the matching next step completes the early fold first (lazy_finish_prefold); each of them is placed between
two steps, after a step that left a pre-fold pending, and the trajectory goes on for at least one fold period."""
import pytest
import torch

from lram_amd import init_state_dict, preset
from lram_amd.config import ModelSpec
from tests.helpers import make_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


def _model(name):
    """(spec, weights) of the models the cases share, built once."""
    if name not in _CACHE:
        if name == "16m":
            spec = preset("xlstm_16m")
            _CACHE[name] = (spec, init_state_dict(spec, seed=71, with_image_encoder=True))
        else:   # the 206M head geometry (DH = 640: five column slices per head, scores from the score kernel), three sLSTM blocks
            spec = ModelSpec(backbone="xlstm", d_model=1280, n_blocks=6, slstm_at=[1, 3, 5])
            _CACHE[name] = (spec, init_state_dict(spec, seed=72))
    return _CACHE[name]


def _engine(monkeypatch, spec, sd, B, period, tail):
    from lram_amd.engine import Engine
    if tail:
        monkeypatch.delenv("LRAM_FOLD_TAIL", raising=False)
    else:
        monkeypatch.setenv("LRAM_FOLD_TAIL", "0")
    eng = Engine(spec, sd, B, device=DEV)     # (the switch is read at lram_create)
    monkeypatch.delenv("LRAM_FOLD_TAIL", raising=False)
    eng.set_state_mode("lazy", period)
    eng.set_micro_batches(2)
    assert eng.state_mode == "lazy"
    return eng


def _steps(eng, seq, image=False):
    out = []
    for obs, rtg, rew, mask in seq:
        call = eng.step_images if image else eng.step
        a, t = call(obs.to(DEV), rtg.to(DEV), rew.to(DEV), mask.to(DEV))
        out.append((a.clone(), t.clone()))
    torch.cuda.synchronize()
    return out


def _state(eng, spec):
    return [eng.export_state_tensor(i, w).clone() for i in range(spec.n_blocks) if i not in spec.slstm_at for w in (0, 1, 2)]


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, (tuple, list)):
            _same(g, w, f"{what}[{k}]")
        else:
            assert torch.equal(g, w), f"{what}[{k}]: {int((g != w).sum())} of {g.numel()} elements differ"


def _both(monkeypatch, model, B, period, run):
    """run(engine) -> nested lists of tensors, on the engine without and with the tail fold."""
    spec, sd = _model(model)
    outs = []
    for tail in (False, True):
        eng = _engine(monkeypatch, spec, sd, B, period, tail)
        outs.append(run(eng, spec))
        eng.close()
    return outs


# B = 27, P = 13: uneven slices of 14 + 13 envs, 2-3 envs per fold class; B = 5: steps whose due class is empty (the fold
# launcher's early return); P = 1: every env folds every step
@pytest.mark.parametrize("B,period,steps", [(27, 13, 32), (5, 13, 30), (8, 5, 14), (8, 1, 8)])
def test_tail_fold_changes_no_bit_16m(hip_lib, monkeypatch, B, period, steps):
    seq = make_inputs(_model("16m")[0], B, steps, seed=31, reset_prob=0.1)
    off, on = _both(monkeypatch, "16m", B, period, lambda eng, spec: [_steps(eng, seq), _state(eng, spec)])
    _same(on, off, f"B {B} period {period}")


def test_tail_fold_changes_no_bit_206m_geometry(hip_lib, monkeypatch):
    B, period = 6, 5
    seq = make_inputs(_model("206m")[0], B, 13, seed=32, reset_prob=0.1)
    off, on = _both(monkeypatch, "206m", B, period, lambda eng, spec: [_steps(eng, seq), _state(eng, spec)])
    _same(on, off, "206M geometry")


def test_tail_fold_changes_no_bit_step_images(hip_lib, monkeypatch):
    B, period = 6, 5
    seq = make_inputs(_model("16m")[0], B, 13, seed=33, reset_prob=0.1, image=True)
    off, on = _both(monkeypatch, "16m", B, period, lambda eng, spec: [_steps(eng, seq, image=True), _state(eng, spec)])
    _same(on, off, "step_images")


# ---- every other entry between two steps, with a pre-fold pending ------------------------------------------------------------
IB, IP, BEFORE, AFTER = 27, 13, 15, 14
# after BEFORE steps the next step folds the envs b with (BEFORE + b) % IP == 0
DUE = [b for b in range(IB) if (BEFORE + b) % IP == 0]
OTHER = 3
assert DUE and all(b not in DUE for b in (OTHER, OTHER + 1, OTHER + 2))


def _op_save_load(eng, spec, seq):
    rec = eng.save_slots([OTHER, OTHER + 2]).clone()
    eng.load_slots([OTHER + 1, DUE[-1]], rec)
    return [rec]


def _op_copy_due_slot(eng, spec, seq):
    eng.copy_slots([DUE[0]], [OTHER])
    return []


def _op_export_import(eng, spec, seq):
    out = []
    for blk in (0, 2):
        t = eng.export_state_tensor(blk, 0).clone()
        eng.import_state_tensor(blk, 0, t)
        out.append(t)
    return out


def _op_reset(eng, spec, seq):
    mask = torch.zeros(IB, dtype=torch.uint8)
    mask[DUE[0]] = 1
    mask[OTHER] = 1
    eng.reset(mask.to(DEV))
    return []


def _op_period(eng, spec, seq):
    eng.set_state_mode("lazy", 5)
    return []


def _op_eager_and_back(eng, spec, seq):
    eng.set_state_mode("eager")
    out = _steps(eng, seq[1:3])
    eng.set_state_mode("lazy", IP)
    return out


def _op_one_slice_and_back(eng, spec, seq):
    eng.set_micro_batches(1)
    out = _steps(eng, seq[1:3])
    eng.set_micro_batches(2)
    return out


def _op_encoder(tokens):
    def op(eng, spec, seq):
        x = torch.randn(IB, tokens, spec.d_model, generator=torch.Generator().manual_seed(5))
        return [eng.encoder_step(x.to(DEV)).clone()]
    return op


def _op_prefill(eng, spec, seq):
    ctx = seq[:3]
    obs = torch.stack([c[0] for c in ctx], 1).contiguous().to(DEV)
    rtg = torch.stack([c[1] for c in ctx], 1).contiguous().to(DEV)
    rew = torch.stack([c[2] for c in ctx], 1).contiguous().to(DEV)
    a, t = eng.prefill(obs, rtg, rew)
    return [a.clone(), t.clone()]


OPS = {"save_load": _op_save_load, "copy_due_slot": _op_copy_due_slot, "export_import": _op_export_import, "reset": _op_reset, "period": _op_period,
       "eager_and_back": _op_eager_and_back, "one_slice_and_back": _op_one_slice_and_back, "encoder_1": _op_encoder(1),
       "encoder_3": _op_encoder(3), "prefill": _op_prefill}


@pytest.mark.parametrize("op", sorted(OPS))
def test_other_entries_complete_the_early_fold(hip_lib, monkeypatch, op):
    spec = _model("16m")[0]
    seq = make_inputs(spec, IB, BEFORE + AFTER, seed=34, reset_prob=0.08)
    extra = make_inputs(spec, IB, 3, seed=35, reset_prob=0.0)

    def run(eng, spec):
        first = _steps(eng, seq[:BEFORE])
        mid = OPS[op](eng, spec, extra)
        return [first, mid, _steps(eng, seq[BEFORE:]), _state(eng, spec)]

    off, on = _both(monkeypatch, "16m", IB, IP, run)
    _same(on, off, op)


def test_lazy_peek_sees_the_early_fold_completed(hip_lib, monkeypatch):
    """lazy_peek completes the pending early fold before it looks: the envs due at the next step show an empty window and g = 1
    (what they show after their fold), where the engine without the tail fold still shows their pending tokens -- the one
    difference there is, and the evidence that the earlier step did launch the fold early.  Every other env reads the same, and so
    does everything after."""
    spec = _model("16m")[0]
    seq = make_inputs(spec, IB, BEFORE + AFTER, seed=36, reset_prob=0.0)

    def run(eng, spec):
        first = _steps(eng, seq[:BEFORE])
        peek = [eng.lazy_peek(0, "pending").clone(), eng.lazy_peek(2, "g").clone(), eng.lazy_peek(0, "m").clone()]
        again = [eng.lazy_peek(0, "pending").clone(), eng.lazy_peek(2, "g").clone(), eng.lazy_peek(0, "m").clone()]
        _same(again, peek, "looking twice")
        return [first, peek, _steps(eng, seq[BEFORE:]), _state(eng, spec)]

    off, on = _both(monkeypatch, "16m", IB, IP, run)
    rest = [b for b in range(IB) if b not in DUE]
    assert float(off[1][0][DUE].min()) > 0.0 and float(on[1][0][DUE].max()) == 0.0
    assert bool((on[1][1][DUE] == 1.0).all())
    assert torch.equal(on[1][0][rest], off[1][0][rest]) and torch.equal(on[1][1][rest], off[1][1][rest])
    assert torch.equal(on[1][2], off[1][2])
    for k in (0, 2, 3):
        _same(on[k], off[k], f"peek part {k}")


def test_record_of_a_slot_folded_early(hip_lib, monkeypatch):
    """save_slots of a slot whose fold is pending early: the early fold is completed first, so the record's C is the folded C_base
    (matrix cores) where the engine without the tail fold computes g C_base + window on the fly (plain fp32 FMAs).  The two differ
    as a record and an export always have (tests/test_gpu_slot_state.py: C within 2e-4 of the tensor's max-abs); every other tensor
    of the record is bit-identical, and so is the whole record of a slot that is not due."""
    spec = _model("16m")[0]
    seq = make_inputs(spec, IB, BEFORE, seed=38, reset_prob=0.0)

    def run(eng, spec):
        _steps(eng, seq)
        return [eng.save_slots([DUE[0], OTHER]).clone()]

    off, on = _both(monkeypatch, "16m", IB, IP, run)
    off, on = off[0].cpu(), on[0].cpu()
    assert torch.equal(on[1], off[1])
    dh, at, n_c = spec.head_dim, 0, 0
    for i in range(spec.n_blocks):
        if i in spec.slstm_at:
            size = spec.d_model * (4 + spec.conv_k)
            assert torch.equal(on[0, at:at + size], off[0, at:at + size]), i
        else:
            c = spec.n_heads * dh * dh
            size = c + spec.inner + spec.n_heads + spec.conv_k * spec.inner
            got, want = on[0, at:at + c].double(), off[0, at:at + c].double()
            assert float((got - want).abs().max()) <= 2e-4 * float(want.abs().max()), i
            assert torch.equal(on[0, at + c:at + size], off[0, at + c:at + size]), i
            n_c += 1
        at += size
    assert at == on.shape[1] and n_c == spec.n_blocks - len(spec.slstm_at)


def test_fold_launches_per_step_stay_one_per_mlstm_block(hip_lib, monkeypatch):
    spec = _model("16m")[0]
    n_mlstm = spec.n_blocks - len(spec.slstm_at)
    steps = 5
    seq = make_inputs(spec, IB, BEFORE + steps, seed=37, reset_prob=0.05)

    def run(eng, spec):
        _steps(eng, seq[:BEFORE])
        eng.profile_begin()
        _steps(eng, seq[BEFORE:])
        _, n_main, _, n_aux = eng.profile_end_split()
        assert n_aux == steps * n_mlstm and n_main == steps * n_mlstm * 2, (n_main, n_aux)
        return []

    _both(monkeypatch, "16m", IB, IP, run)
