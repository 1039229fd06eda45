"""Float64 numpy restatement of the allowed-set rule (include/lram_hip.h, lram_set_action_mask): a column works on the SUB-ROW
of its allowed entries, in vocabulary order, exactly as if the reference's function had been handed that sub-row, and the answer
is mapped back to vocabulary indices.  There is no second copy of the sampling head's row rule here: the argmax, the draw and the
log-probability under the drawn distribution cut the row, call the restatement tests/sampling_ref.py / tests/sampling_slots_ref.py
hold to the reference, and map back.  The score entries' log-probability is a plain float64 log-softmax of the cut row
(_log_softmax_at: written out here in numpy, as tests/test_gpu_score.py takes torch.log_softmax; tests/test_action_mask.py holds it
to torch's).  Plus the seeded rows the CPU and GPU tests of the masks share."""
import numpy as np

from tests import sampling_ref as sr
from tests import sampling_slots_ref as ssr

NEG_INF = float("-inf")


def _index(allow, n=None):
    """The vocabulary indices of the sub-row: allowed and below n."""
    allow = np.asarray(allow, dtype=bool)
    return np.flatnonzero(allow if n is None else allow[:n])


def masked_argmax(row, allow, n=None):
    idx = _index(allow, n)
    return int(idx[sr.argmax_rule(np.asarray(row)[idx])])


def masked_row_probs(row, allow, temperature=1.0, top_k=0, top_p=0.0):
    """sr.row_probs of the sub-row scattered back to the row's length (zeros at disallowed entries), or None where the
    sub-row takes the argmax rule."""
    row = np.asarray(row, dtype=np.float32)
    idx = _index(allow, row.shape[0])
    p = sr.row_probs(row[idx], temperature, top_k, top_p)
    if p is None:
        return None
    out = np.zeros(row.shape[0], dtype=np.float64)
    out[idx] = p
    return out


def masked_sample_row(row, u, allow, mode=1, temperature=1.0, top_k=0, top_p=0.0):
    row = np.asarray(row, dtype=np.float32)
    idx = _index(allow, row.shape[0])
    sub = row[idx]
    if int(mode) == 0:
        return int(idx[sr.argmax_rule(sub)])
    return int(idx[sr.sample_rows(sub[None], np.array([u]), float(temperature), int(top_k), float(top_p))[0]])


def masked_sample_rows(logits, uni, allow, mode, temperature, top_k, top_p):
    return np.array([masked_sample_row(logits[r], uni[r], allow[r], mode[r], temperature[r], top_k[r], top_p[r])
                     for r in range(len(uni))], dtype=np.int64)


def masked_row_logp(row, token, allow, mode=1, temperature=1.0, top_k=0, top_p=0.0):
    """ssr.row_logp of the sub-row at the token's place in it; a token outside the sub-row: -inf; token -1: the fill value 0."""
    token = int(token)
    if token == -1:
        return 0.0
    row = np.asarray(row, dtype=np.float32)
    idx = _index(allow, row.shape[0])
    at = np.flatnonzero(idx == token)
    if at.size == 0:
        return NEG_INF
    return ssr.row_logp(row[idx], int(at[0]), mode, temperature, top_k, top_p)


def masked_rows_logp(logits, tokens, allow, mode, temperature, top_k, top_p):
    return np.array([masked_row_logp(logits[r], tokens[r], allow[r], mode[r], temperature[r], top_k[r], top_p[r])
                     for r in range(len(tokens))], dtype=np.float64)


def _log_softmax_at(x, at, temperature):
    """float64 log_softmax(temperature * x)[at]; NaN where x holds one (or nothing but -inf), -inf at a -inf entry."""
    z = float(temperature) * np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = z.max() if not np.isnan(z).any() else np.nan
        return float(z[at] - m - np.log(np.exp(z - m).sum()))


def masked_score_logp(row, target, allow, n, over, temperature=1.0):
    """What the score entries return for `target` on a row of n_vocab logits whose selectable range is [0, n):
    over = "vocab": log_softmax over the whole row, the mask ignored; over = "selectable": over the sub-row, a target outside it
    -inf."""
    row, target = np.asarray(row, dtype=np.float32), int(target)
    if over == "vocab":
        return _log_softmax_at(row, target, temperature) if 0 <= target < row.shape[0] else NEG_INF
    assert over == "selectable", over
    idx = _index(allow, n)
    at = np.flatnonzero(idx == target)
    if at.size == 0:
        return NEG_INF
    return _log_softmax_at(row[idx], int(at[0]), temperature)


N_CLASSES = 8


def mask_rows_case(n, rows=160, seed=20261018):
    """ssr.rows_case(n) plus one allowed set per row ("allow": bool [R, n]).  The class of row r is r % 8:
      0  everything allowed                          4  only tokens 32 .. 63 (the whole range where n <= 32)
      1  one allowed token that is not the argmax    5  a set whose logits are all -inf
      2  everything but the argmax                   6  a NaN planted at a disallowed index
      3  every other token (the parity alternates)   7  a NaN planted at an allowed index
    The N_EDGE edge rows get sets that cut into their special entries: the NaN of row e, the first +inf of e + 1, the lowest
    maximum of e + 3 and index 0 of the all -inf row e + 5 are disallowed, e + 2 keeps every third of its equal logits, e + 4
    loses both ends.  Classes 5 - 7 change the row's logits (the case's "logits" is the changed array)."""
    c = ssr.rows_case(n, rows, seed)
    logits = c["logits"].copy()
    R = logits.shape[0]
    rng = np.random.default_rng(seed + 7919 * n)
    allow = np.ones((R, n), dtype=bool)
    i = np.arange(n)
    e = R - ssr.N_EDGE
    for r in range(e):
        k = r % N_CLASSES
        top = sr.argmax_rule(logits[r])
        if k == 1:
            allow[r] = False
            allow[r, (top + 1 + int(rng.integers(0, n - 1))) % n] = True
        elif k == 2:
            allow[r, top] = False
        elif k == 3:
            allow[r] = i % 2 == (r // N_CLASSES) % 2
        elif k == 4 and n > 32:
            allow[r] = (i >= 32) & (i < 64)
        elif k == 5:
            allow[r] = rng.random(n) < 0.25
            allow[r, int(rng.integers(0, n))] = True
            logits[r, allow[r]] = -np.inf
        elif k in (6, 7):
            allow[r] = rng.random(n) < 0.5
            allow[r, [0, n - 1]] = [True, False] if (r // N_CLASSES) % 2 else [False, True]
            pick = np.flatnonzero(allow[r] == (k == 7))
            logits[r, int(pick[int(rng.integers(0, pick.size))])] = np.nan
    allow[e, 5] = False
    allow[e + 1, 3] = False
    allow[e + 2] = i % 3 == 1
    allow[e + 3, 2] = False
    allow[e + 4, [0, n - 1]] = False
    allow[e + 5, 0] = False
    return dict(c, logits=logits, allow=allow)


def cdf_margin(case):
    """Per sampled row on the draw rule, the distance (in probability) of its uniform from the nearest step of the
    restatement's CDF; inf for the rows on the argmax rule."""
    out = np.full(len(case["uniform"]), np.inf)
    for r in range(len(out)):
        if case["mode"][r] == 0:
            continue
        p = masked_row_probs(case["logits"][r], case["allow"][r], case["temperature"][r], case["top_k"][r], case["top_p"][r])
        if p is not None:
            out[r] = np.abs(np.cumsum(p)[p > 0] - case["uniform"][r]).min()
    return out
