"""Float64 numpy restatement of what lram_score_last_sampled / lram_sample_rows compute per row -- the log-probability of a
given token under the distribution the sampling head draws from, per-row settings included -- built on the row rule of
tests/sampling_ref.py, plus the seeded rows the CPU and GPU tests of the per-slot settings share."""
import numpy as np

from tests import sampling_ref as sr

NEG_INF = float("-inf")


def row_logp(row, token, mode=1, temperature=1.0, top_k=0, top_p=0.0):
    """log P(token) under sample_from_logits' filtered distribution of `row` (float64).  mode 0 (greedy) and rows the rule has
    no answer for (a NaN, a maximum of +-inf, nothing left) are on the argmax rule: 0 at the argmax token, -inf elsewhere.
    A token outside 0 .. n - 1 or outside the support (probability 0: never drawn): -inf.  Token -1: the fill value 0."""
    token = int(token)
    if token == -1:
        return 0.0
    row = np.asarray(row, dtype=np.float32)
    n = row.shape[0]
    probs = None if int(mode) == 0 else sr.row_probs(row, temperature, top_k, top_p)
    if probs is None:
        return 0.0 if token == sr.argmax_rule(row) else NEG_INF
    if not 0 <= token < n or probs[token] == 0.0:
        return NEG_INF
    x = row.astype(np.float64) + 0.0
    z = float(temperature) * (x - x.max())
    return float(z[token] - np.log(np.exp(z[probs > 0]).sum()))


def rows_logp(logits, tokens, mode, temperature, top_k, top_p):
    """row_logp over rows with per-row settings -> float64 [R]."""
    return np.array([row_logp(logits[r], tokens[r], mode[r], temperature[r], top_k[r], top_p[r])
                     for r in range(len(tokens))], dtype=np.float64)


def sample_rows(logits, uni, mode, temperature, top_k, top_p):
    """sampling_ref.sample_rows with per-row settings; greedy rows (mode 0) take the argmax rule -> int64 [R]."""
    out = np.empty(len(uni), dtype=np.int64)
    for r in range(len(uni)):
        if int(mode[r]) == 0:
            out[r] = sr.argmax_rule(logits[r])
        else:
            out[r] = sr.sample_rows(logits[r:r + 1], uni[r:r + 1], float(temperature[r]), int(top_k[r]), float(top_p[r]))[0]
    return out


TEMPERATURES = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)
TOP_K = (1, 5, 0, 40, 10)
TOP_P = (0.0, 0.5, 1.0, 0.25, 0.9)
N_EDGE = 6


def rows_case(n, rows=160, seed=20261018):
    """Seeded rows of n logits with a different setting on every row (top_k 1 / 5 / 0 / ..., top_p 0 / 0.5 / 1 / ...,
    temperatures 0.25 .. 4, every seventh row greedy), the last N_EDGE of them the edge rows of the sampling tests: a NaN, a
    +inf maximum, all-equal logits, ties at the k-th place (k = 2), -inf entries, all -inf.  Returns a dict of numpy arrays:
    logits float32 [R, n], uniform float64 [R], mode uint8 [R], temperature / top_p float64 [R], top_k int32 [R]."""
    rng = np.random.default_rng(seed + n)
    R = rows
    logits = (rng.standard_normal((R, n)) * 2).astype(np.float32)
    r = np.arange(R)
    temperature = np.array([TEMPERATURES[i % len(TEMPERATURES)] for i in r], dtype=np.float64)
    top_k = np.minimum(np.array([TOP_K[(i // 2) % len(TOP_K)] for i in r], dtype=np.int32), n)
    top_p = np.array([TOP_P[(i // 3) % len(TOP_P)] for i in r], dtype=np.float64)
    mode = (r % 7 != 6).astype(np.uint8)
    e = R - N_EDGE
    logits[e, 5] = np.nan                                   # NaN: the argmax rule (NaN is the maximum)
    logits[e + 1, 7] = logits[e + 1, 3] = np.inf            # +inf maximum: the first index of it
    logits[e + 2, :] = 1.25                                 # all equal: the quantile is the maximum, nothing is dropped
    logits[e + 3, [2, 9, n - 1]] = 50.0                     # three equal maxima, k = 2: the two lowest indices stay
    logits[e + 4, 4:n - 4] = -np.inf                        # -inf entries: probability 0
    logits[e + 5, :] = -np.inf                              # nothing has a probability: index 0
    mode[e:] = 1
    temperature[e:] = 1.0
    top_k[e:] = [0, 3, 0, 2, 0, 0]
    top_p[e:] = [0.5, 0.0, 0.5, 0.0, 0.0, 0.0]
    return {"logits": logits, "uniform": rng.random(R), "mode": mode, "temperature": temperature, "top_k": top_k,
            "top_p": top_p}


def scored_tokens(case, drawn, seed=7):
    """The tokens a rows_case is scored at: even rows the drawn token (inside the support), odd rows uniform random over the
    row (mostly outside it where a filter is on)."""
    n = case["logits"].shape[1]
    rng = np.random.default_rng(seed + n)
    tok = np.asarray(drawn, dtype=np.int64).copy()
    odd = np.arange(len(tok)) % 2 == 1
    tok[odd] = rng.integers(0, n, size=int(odd.sum()))
    return tok.astype(np.int32)
