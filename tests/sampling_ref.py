"""Float64 numpy restatement of the sampling head's row rule (include/lram_hip.h, lram_set_sampling) and a numpy
Philox4x32-10: what the GPU tests hold the device code to on live logits.  test_sampling.py checks the restatement against
probabilities recorded from the reference's own sample_from_logits (tests/golden/sampling_reference.npz) and the generator
against the published Random123 known answers."""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (uint32, broadcastable) -> the block's four output words [..., 4] (uint32)."""
    c = np.asarray(counter, dtype=np.uint64) & _M32
    k = np.asarray(key, dtype=np.uint64) & _M32
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0      # 32 x 32 -> 64 bit products: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms(seed, slot_base, n_slots, act_dim, draw):
    """The uniforms of one draw, float64 [n_slots, act_dim]: key (seed lo, seed hi), counter (slot lo, dim, draw lo, draw hi),
    u = x0 * 2^-32."""
    seed, slot_base, draw = int(seed), int(slot_base), int(draw)
    slots = (np.arange(n_slots, dtype=np.uint64) + np.uint64(slot_base & 0xFFFFFFFFFFFFFFFF)) & _M32
    ctr = np.zeros((n_slots, act_dim, 4), dtype=np.uint64)
    ctr[..., 0] = slots[:, None]
    ctr[..., 1] = np.arange(act_dim, dtype=np.uint64)[None, :]
    ctr[..., 2] = draw & 0xFFFFFFFF
    ctr[..., 3] = (draw >> 32) & 0xFFFFFFFF
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32_10(ctr, key)[..., 0].astype(np.float64) * 2.0 ** -32


def argmax_rule(row):
    """torch.argmax: NaN is the maximum, the first index wins."""
    row = np.asarray(row)
    nan = np.isnan(row)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(row))


def row_probs(row, temperature=1.0, top_k=0, top_p=0.0):
    """Probability of every vocabulary entry (float64, zeros outside the support), or None where the rule has no answer
    (a NaN, a maximum of +-inf, nothing left) and the head takes the argmax."""
    x = np.asarray(row, dtype=np.float32).astype(np.float64) + 0.0
    n = x.shape[0]
    if np.isnan(x).any() or not np.isfinite(x.max()):
        return None
    keep = np.ones(n, dtype=bool)
    if top_p > 0.0:
        srt = np.sort(x)
        rank = float(top_p) * (n - 1)
        lo, hi = int(np.floor(rank)), int(np.ceil(rank))
        w = rank - lo
        a, b = srt[lo], srt[hi]
        with np.errstate(invalid="ignore"):
            q = a + w * (b - a) if w < 0.5 else b - (b - a) * (1.0 - w)   # at::lerp
        if q != x.max():
            keep &= x > q
    if top_k > 0 and keep.sum() > top_k:
        idx = np.flatnonzero(keep)
        order = idx[np.argsort(-x[idx], kind="stable")]   # descending, the lowest index first among equals
        keep = np.zeros(n, dtype=bool)
        keep[order[:top_k]] = True
    if not keep.any():
        return None
    z = np.where(keep, float(temperature) * (x - x.max()), -np.inf)
    p = np.exp(z)
    return p / p.sum()


def inverse_cdf(p, u):
    """First index, in vocabulary order, whose cumulative probability exceeds u (the last of the support if none does)."""
    p = np.asarray(p, dtype=np.float64)
    cdf = np.cumsum(p)
    u = np.atleast_1d(np.asarray(u, dtype=np.float64))
    tok = np.searchsorted(cdf, u, side="right")
    last = int(np.flatnonzero(p > 0)[-1])
    tok = np.minimum(tok, last)
    # a plateau of the CDF (zero-probability entries) is never an answer: searchsorted(right) already steps over them
    return tok.astype(np.int64), cdf


def sample_rows(logits, uni, temperature=1.0, top_k=0, top_p=0.0):
    """logits [R, n] float32, uni [R] -> tokens [R] (int64) by the row rule; rows without an answer take the argmax."""
    logits = np.asarray(logits, dtype=np.float32)
    out = np.empty(logits.shape[0], dtype=np.int64)
    for r in range(logits.shape[0]):
        p = row_probs(logits[r], temperature, top_k, top_p)
        out[r] = argmax_rule(logits[r]) if p is None else inverse_cdf(p, uni[r])[0][0]
    return out


def inv_tokenize(tokens, n_discrete=18, action_channels=256, tok_min=-1.0, tok_max=1.0):
    """MinMaxTokenizer.inv_tokenize as the head kernels evaluate it (fp32)."""
    t = np.maximum(np.asarray(tokens, dtype=np.int64) - n_discrete, 0).astype(np.float32)
    bw = (np.float32(tok_max) - np.float32(tok_min)) / np.float32(action_channels)
    return t * bw + np.float32(tok_min)
