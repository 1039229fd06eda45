#!/usr/bin/env python3
"""Cost of the sampling head at the headline configuration (xLSTM 16M, 4096 env slots).

Step time armed against disarmed in ONE process, interleaved blocks (A B A B ...), and -- when run under
`rocprofv3 --kernel-trace --stats -- python scripts/sample_head_cost.py` -- the per-launch time of action_sample_kernel
beside the head's logits GEMM of the same trace (the GEMM is untouched by the sampling mode).  bench.py has no switch for
sampling, hence this script.  Prints one JSON line.

    python scripts/sample_head_cost.py [--slots 4096] [--model xlstm_16m] [--steps 48] [--blocks 4]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="xlstm_16m")
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--temperature", type=float, default=0.75)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--top-p", type=float, default=0.5)
    args = ap.parse_args()
    spec = preset(args.model)
    dev = torch.device("cuda", 0)
    eng = Engine(spec, init_state_dict(spec, seed=0), args.slots, device=dev)
    B = args.slots
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

    def arm(on):
        if on:
            eng.set_sampling(args.temperature, args.top_k, args.top_p, seed=1)
        else:
            eng.set_sampling(None)

    run(args.warmup)
    ms = {False: [], True: []}
    for _ in range(args.blocks):
        for on in (False, True):
            arm(on)
            run(4)
            ms[on].append(run(args.steps))
    off, on = sorted(ms[False]), sorted(ms[True])
    med = lambda v: v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])  # noqa: E731
    print(json.dumps({"model": args.model, "slots": B, "steps_per_block": args.steps, "sampling": [args.temperature, args.top_k, args.top_p],
                      "ms_per_step_argmax": [round(x, 4) for x in ms[False]], "ms_per_step_sampling": [round(x, 4) for x in ms[True]],
                      "median_argmax_ms": round(med(off), 4), "median_sampling_ms": round(med(on), 4),
                      "sampling_over_argmax": round(med(on) / med(off), 4), "state_mode": eng.state_mode}))
    eng.close()


if __name__ == "__main__":
    main()
