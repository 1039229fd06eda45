#!/usr/bin/env python3
"""Cost of the allowed-action sets at the headline configuration (xLSTM 16M, 4096 env slots).

Step time with a set on every slot against no mask, greedy and sampled, in ONE process, interleaved blocks (none, masked, none,
masked, ...).  Slot b's set is a function of b: everything, Pong's six actions beside every other bin, tokens 32 .. 63, every
third token.  bench.py has no switch for masks, hence this script.  Prints one JSON line.

    python scripts/action_mask_cost.py [--slots 4096] [--model xlstm_16m] [--steps 48] [--blocks 4]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from lram_amd import init_state_dict, preset  # noqa: E402
from lram_amd.engine import Engine  # noqa: E402


def slot_sets(B, V, ND):
    t = torch.arange(V)
    allow = torch.ones(B, V, dtype=torch.bool)
    pong = torch.zeros(V, dtype=torch.bool)
    pong[[0, 1, 3, 4, 11, 12]] = True
    allow[1::4] = pong | ((t >= ND) & (t % 2 == 1))
    allow[2::4] = (t >= 32) & (t < 64)
    allow[3::4] = t % 3 == 0
    return allow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="xlstm_16m")
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=16)
    args = ap.parse_args()
    spec = preset(args.model)
    dev = torch.device("cuda", 0)
    B = args.slots
    eng = Engine(spec, init_state_dict(spec, seed=0), B, device=dev)
    allow = slot_sets(B, spec.n_vocab, spec.n_discrete)
    obs = torch.rand(B, spec.state_dim, device=dev) * 2 - 1
    rtg, rew = torch.full((B,), 4.5, device=dev), torch.zeros(B, device=dev)
    mask = torch.zeros(B, dtype=torch.uint8, device=dev)

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            eng.step(obs, rtg, rew, mask)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    run(args.warmup)
    out = {"model": args.model, "slots": B, "steps_per_block": args.steps, "state_mode": eng.state_mode}
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])  # noqa: E731
    for head in ("greedy", "sampled"):
        if head == "sampled":
            eng.set_sampling(0.75, 10, 0.5, seed=1)
        ms = {False: [], True: []}
        for _ in range(args.blocks):
            for on in (False, True):
                eng.set_action_mask(allow if on else None)
                run(4)
                ms[on].append(run(args.steps))
        out[head] = {"ms_per_step_no_mask": [round(x, 4) for x in ms[False]], "ms_per_step_masked": [round(x, 4) for x in ms[True]],
                     "median_no_mask_ms": round(med(ms[False]), 4), "median_masked_ms": round(med(ms[True]), 4),
                     "masked_over_no_mask": round(med(ms[True]) / med(ms[False]), 4)}
    _, tok = eng.step(obs, rtg, rew, mask)
    torch.cuda.synchronize()
    out["tokens_allowed"] = bool(allow.to(dev).gather(1, tok.long()).all())
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
