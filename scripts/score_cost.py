"""Timing instrument of lram_score: what the head at every timestep costs on top of lram_prefill.

HIP-event time of Engine.score (tokens + logp wanted, int32 targets, no logits) against Engine.prefill over the same inputs,
in one process, alternating, after warm-up: the 16M geometry at 1024 envs x 63 timesteps and the 206M geometry at 64 envs x
512 timesteps.  By arithmetic the head adds 2 * B * L * d_model * act_dim * n_vocab FLOP and the score kernel one read of the
logits; the ratio score / prefill is what this prints.
Usage: python scripts/score_cost.py [--out profiles/score_cost.txt] [--iters 5] [--only xlstm_16m|xlstm_206m]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lram_amd import init_state_dict, preset          # noqa: E402
from lram_amd import engine as E                      # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(name, B, L, iters, warm=2):
    spec = preset(name)
    sd = init_state_dict(spec, seed=1)
    g = torch.Generator().manual_seed(5)
    eng = E.Engine(spec, sd, B, device="cuda:0")
    obs = (torch.rand(B, L, spec.state_dim, generator=g) * 2 - 1).cuda()
    rtg = (torch.full((B, L), 4.5) - 0.01 * torch.arange(L)).contiguous().cuda()
    rew = torch.zeros(B, L).cuda()
    tok = torch.randint(spec.n_discrete, spec.n_vocab, (B, L, spec.act_dim), generator=g, dtype=torch.int32).cuda()
    ones = torch.ones(B, dtype=torch.uint8).cuda()
    prefill = lambda: eng.prefill(obs, rtg, rew, reset_mask=ones)
    score = lambda: eng.score(obs, rtg, rew, tokens=tok, reset_mask=ones, want=("tokens", "logp"))
    for _ in range(warm):      # (grows the workspaces, allocates the lanes and the score scratch)
        prefill()
        score()
    torch.cuda.synchronize()
    p_ms, s_ms = [], []
    for _ in range(iters):     # alternating: both see the same clocks
        p_ms.append(event_ms(prefill))
        s_ms.append(event_ms(score))
    p, s = statistics.median(p_ms), statistics.median(s_ms)
    head_gflop = 2.0 * B * L * spec.d_model * spec.act_dim * spec.n_vocab / 1e9
    row = {"model": name, "envs": B, "timesteps": L, "prefill_ms": round(p, 3), "score_ms": round(s, 3),
           "score_over_prefill": round(s / p, 4), "head_gflop": round(head_gflop, 1),
           "head_tflops_if_all_extra_time": round(head_gflop / max(s - p, 1e-6), 1),
           "prefill_ms_all": [round(x, 3) for x in p_ms], "score_ms_all": [round(x, 3) for x in s_ms]}
    eng.close()
    del eng
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default=None, help="xlstm_16m or xlstm_206m")
    a = ap.parse_args()
    rows = []
    for name, B, L in (("xlstm_16m", 1024, 63), ("xlstm_206m", 64, 512)):
        if a.only in (None, name):
            rows.append(measure(name, B, L, a.iters))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# scripts/score_cost.py: median HIP-event ms of Engine.prefill and Engine.score over the same inputs, alternating\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
