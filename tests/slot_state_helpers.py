"""Helpers of the per-slot state tests (tests/test_gpu_slot_state.py): the record layout restated from the header, records
rebuilt from whole-batch exports, and the step loops the scenarios share."""
import torch


def record_layout(spec):
    """[(block, which, per-env shape, offset in floats)] in record order (include/lram_hip.h: blocks in order, tensors in
    `which` order, reference layout) and the record's length."""
    out, off = [], 0

    def add(block, which, shape):
        nonlocal off
        n = 1
        for s in shape:
            n *= s
        out.append((block, which, tuple(shape), off))
        off += n

    for i in range(spec.n_blocks):
        if spec.backbone == "mamba":
            add(i, 0, (spec.d_inner, spec.d_state))
            add(i, 3, (spec.d_inner, spec.d_conv))
        elif i in spec.slstm_at:
            add(i, 0, (4, spec.d_model))
            add(i, 3, (spec.conv_k, spec.d_model))
        else:
            dh = spec.head_dim
            add(i, 0, (spec.n_heads, dh, dh))
            add(i, 1, (spec.n_heads, dh))
            add(i, 2, (spec.n_heads,))
            add(i, 3, (spec.conv_k, spec.inner))
    return out, off


def is_slstm_state(spec, block, which):
    return spec.backbone == "xlstm" and block in spec.slstm_at and which == 0


def exported_slice(eng, spec, block, which, slots):
    """Env slices, flattened per env [n, numel], of one whole-batch export (folds every pending window in lazy mode)."""
    idx = torch.as_tensor(list(slots), device=eng.device)
    t = eng.export_state_tensor(block, which)
    if is_slstm_state(spec, block, which):
        return t[:, idx].permute(1, 0, 2).reshape(len(idx), -1).contiguous()          # [4, B, D] -> [n, 4 * D]
    return t[idx].reshape(len(idx), -1).contiguous()


def to_dev(step):
    return tuple(x.cuda() for x in step)


def run_steps(eng, seq, lo, hi, out=None, taps=True):
    """Steps lo .. hi - 1 of seq; appends clones of actions, tokens (and the hidden / logits taps) to out[...]."""
    out = {"a": [], "tok": [], "hid": [], "logits": []} if out is None else out
    for t in range(lo, hi):
        obs, rtg, rew, mask = to_dev(seq[t])
        a, tok = eng.step(obs, rtg, rew, mask)
        out["a"].append(a.clone())
        out["tok"].append(tok.clone())
        if taps:
            _, hid, logits = eng.taps()
            out["hid"].append(hid)
            out["logits"].append(logits)
    torch.cuda.synchronize()
    return out


def feed_as(seq, t_from, src, dst):
    """A copy of seq in which, from step t_from on, env dst[i] is fed what env src[i] is fed (inputs and reset mask)."""
    out = []
    for t, step in enumerate(seq):
        step = tuple(x.clone() for x in step)
        if t >= t_from:
            for x in step:
                x[list(dst)] = x[list(src)]
        out.append(step)
    return out


def force_mask(seq, slot, steps_on=(), steps_off=()):
    """Reset `slot` at steps_on and never at steps_off (in place)."""
    for t in steps_on:
        seq[t][3][slot] = 1
    for t in steps_off:
        seq[t][3][slot] = 0
