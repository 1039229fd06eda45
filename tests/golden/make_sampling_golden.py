#!/usr/bin/env python3
"""Generate tests/golden/sampling_reference.npz by EXECUTING the reference's own sample_from_logits
(src/algos/models/model_utils.py:7-32; the file imports torch and numpy only).

    python tests/golden/make_sampling_golden.py <path of the reference checkout>

Run in a build container with a read-only checkout of the reference, never on the GPU box (see the security note in
make_golden_from_reference.py: this imports third-party code).  The function draws with torch's generator, which the engine
cannot reproduce; what is recorded is the DISTRIBUTION it draws from: torch.distributions.Categorical and torch.topk are
wrapped by recorders while it runs, and per case the file stores inputs and outputs only --

    logits [C, 274] float32 (row c uses its first n[c] entries), n, temperature, top_k, top_p, name,
    probs  [C, 274] float64: the probability of every vocabulary entry, zeros outside the support

-- no reference source text.  Cases: n = 274 (continuous head) and 18 (discrete head); seeded normal rows of standard
deviation 0.3 / 1 / 3 / 10; the keyword sets below ((1, 50, 0.9): fewer than k logits survive the quantile, and with n = 18
k is 18, as torch.topk refuses k > n); a flat row, a row with -inf entries, a row with ties away from the k-th place, a row
peaked by 40.  The generator asserts that no case has a tie at its k-th place (torch leaves the winner open there)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N_MAX = 274


def load_reference(root):
    path = os.path.join(root, "src", "algos", "models", "model_utils.py")
    spec = importlib.util.spec_from_file_location("ref_model_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.sample_from_logits


def reference_probs(fn, row, temperature, top_k, top_p):
    """Run the reference function on one row; return the probabilities it sampled from, per vocabulary entry."""
    rec = {}
    real_cat, real_topk = torch.distributions.Categorical, torch.topk

    class Recorder(real_cat):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            rec["probs"] = self.probs.detach().clone()

    def topk(*a, **kw):
        out = real_topk(*a, **kw)
        rec["values"], rec["indices"] = out[0].detach().clone(), out[1].detach().clone()
        return out

    torch.distributions.Categorical, torch.topk = Recorder, topk
    try:
        tok = fn(torch.from_numpy(row), temperature=temperature, top_k=top_k, top_p=top_p)
    finally:
        torch.distributions.Categorical, torch.topk = real_cat, real_topk
    p = rec["probs"].double().numpy()
    full = np.zeros(row.shape[0], dtype=np.float64)
    if top_k > 0:
        idx = rec["indices"].numpy()
        vals = rec["values"].double().numpy()
        if top_k < row.shape[0]:   # no tie at the k-th place: the k-th kept value is strictly above everything dropped
            dropped = np.ones(row.shape[0], dtype=bool)
            dropped[idx] = False
            filt = row.astype(np.float64)
            rest = filt[dropped]
            kth = vals.min()
            assert np.isneginf(kth) or rest.size == 0 or not np.any(rest == kth), "tie at the k-th place"
        full[idx] = p
    else:
        full[:] = p
    assert abs(full.sum() - 1.0) < 1e-12 and full[int(tok)] > 0
    return full


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    fn = load_reference(sys.argv[1])
    rng = np.random.default_rng(20261016)
    cases = []

    def add(name, row, t, k, p):
        cases.append((name, np.asarray(row, dtype=np.float32), float(t), int(k), float(p)))

    for n in (274, 18):
        for scale in (0.3, 1.0, 3.0, 10.0):
            keywords = [(1.0, 0, 0.0), (0.75, 0, 0.5), (1.0, 0, 0.5), (2.0, 5, 0.0), (1.0, 10, 0.9), (1.0, min(50, n), 0.9),
                        (0.5, 1, 0.0), (1.0, n, 0.0)]
            for t, k, p in keywords:
                row = (rng.standard_normal(n) * scale).astype(np.float32)
                add(f"normal_n{n}_s{scale}_t{t}_k{k}_p{p}", row, t, k, p)
    for n in (274, 18):
        for t, k, p in [(1.0, 0, 0.5), (0.75, 0, 0.5), (1.0, 0, 0.0)]:
            add(f"flat_n{n}_t{t}_k{k}_p{p}", np.full(n, 0.625, dtype=np.float32), t, k, p)
        for t, k, p in [(1.0, 0, 0.0), (1.0, 0, 0.5), (2.0, 5, 0.0), (1.0, 10, 0.9)]:
            row = rng.standard_normal(n).astype(np.float32)
            row[rng.choice(n, size=max(2, n // 40), replace=False)] = -np.inf
            add(f"neginf_n{n}_t{t}_k{k}_p{p}", row, t, k, p)
        for t, k, p in [(1.0, 0, 0.5), (2.0, 5, 0.0), (1.0, 0, 0.0)]:
            row = rng.standard_normal(n).astype(np.float32)
            order = np.argsort(-row)
            row[order[1]] = row[order[0]]            # the two largest are equal: both inside any k >= 2
            row[order[n // 2 + 2]] = row[order[n // 2 + 1]]   # and two equal ones below the median: both dropped by top_p = 0.5
            add(f"ties_n{n}_t{t}_k{k}_p{p}", row, t, k, p)
        for t, k, p in [(1.0, 0, 0.0), (0.75, 0, 0.5), (1.0, 10, 0.9)]:
            row = rng.standard_normal(n).astype(np.float32)
            row[n // 3] += 40.0
            add(f"peaked40_n{n}_t{t}_k{k}_p{p}", row, t, k, p)

    C = len(cases)
    logits = np.zeros((C, N_MAX), dtype=np.float32)
    probs = np.zeros((C, N_MAX), dtype=np.float64)
    for c, (name, row, t, k, p) in enumerate(cases):
        logits[c, :row.shape[0]] = row
        probs[c, :row.shape[0]] = reference_probs(fn, row, t, k, p)
    out = os.path.join(HERE, "sampling_reference.npz")
    np.savez_compressed(out, logits=logits, probs=probs, n=np.array([c[1].shape[0] for c in cases], dtype=np.int32),
                        temperature=np.array([c[2] for c in cases]), top_k=np.array([c[3] for c in cases], dtype=np.int32),
                        top_p=np.array([c[4] for c in cases]), name=np.array([c[0] for c in cases]))
    print(f"{C} cases -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
