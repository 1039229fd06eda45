"""Stored contexts of per-env length: what lram_prefill_ragged costs beside the dense call and beside L lram_step calls.

    python scripts/bench_ragged.py [config] [B] [L] [repeats]      (defaults: xlstm_16m 64 252 7)

Legs, all in this one process on warm engines, interleaved (leg a, b, c, d, e, then again), median of `repeats` each:
  (a) Engine.prefill                                  the dense call
  (b) Engine.prefill(lengths = L for every env)       the ragged entry, same launches as (a)
  (c) 4 distinct lengths  (L, 3L/4, L/2, L/4, B/4 envs each)
  (d) B distinct lengths spread over 1 .. L
  (e) what callers do for (d) without the entry: L lram_step calls (every env stepped through L timesteps)
Every call ends in a device synchronise; env-timesteps/s counts the timesteps of the contexts (sum of the lengths), (e) as (d)."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lram_amd import init_state_dict, preset
from lram_amd.engine import Engine, context_plan

cfg = sys.argv[1] if len(sys.argv) > 1 else "xlstm_16m"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
L = int(sys.argv[3]) if len(sys.argv) > 3 else 252
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
spec = preset(cfg); sd = init_state_dict(spec, 0)
dev = "cuda:0"
eng = Engine(spec, sd, B, device=dev)
obs = torch.rand(B, L, spec.state_dim, device=dev) * 2 - 1
rtg = torch.full((B, L), 4.5, device=dev); rew = torch.zeros(B, L, device=dev)
ones = torch.ones(B, dtype=torch.uint8, device=dev)
obs_t = [obs[:, l].contiguous() for l in range(L)]; rtg_t = [rtg[:, l].contiguous() for l in range(L)]
rew_t = [rew[:, l].contiguous() for l in range(L)]
full = [L] * B
four = [max(1, L * (4 - (b * 4) // B) // 4) for b in range(B)]
spread = [1 + round(b * (L - 1) / max(1, B - 1)) for b in range(B)]


def steps():
    for l in range(L):
        eng.step(obs_t[l], rtg_t[l], rew_t[l], ones if l == 0 else None)


legs = (("a", "lram_prefill", lambda: eng.prefill(obs, rtg, rew, reset_mask=ones), full),
        ("b", "lram_prefill_ragged, every length L", lambda: eng.prefill(obs, rtg, rew, reset_mask=ones, lengths=full), full),
        ("c", "lram_prefill_ragged, 4 distinct lengths", lambda: eng.prefill(obs, rtg, rew, reset_mask=ones, lengths=four), four),
        ("d", f"lram_prefill_ragged, {len(set(spread))} distinct lengths", lambda: eng.prefill(obs, rtg, rew, reset_mask=ones, lengths=spread), spread),
        ("e", f"{L} lram_step calls", steps, spread))
times = {k: [] for k, *_ in legs}
for _, _, fn, _ in legs:      # warm: workspace growth, lane streams, scratch
    fn(); torch.cuda.synchronize()
for rep in range(reps):
    for k, _, fn, _ in legs:
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
print(f"{cfg}, {B} envs x {L} timesteps, median of {reps} interleaved repeats (min .. max), one process, warm")
for k, name, _, lengths in legs:
    t = times[k]
    med = statistics.median(t)
    n_chunks = "-" if k in ("a", "e") else str(len(context_plan(L, lengths, -(-L // -(-L // 21)))))
    print(f"({k}) {name:<45s} {med*1e3:8.2f} ms  ({min(t)*1e3:.2f} .. {max(t)*1e3:.2f})  chunks {n_chunks:>4s}  "
          f"{sum(lengths)/med:12,.0f} context env-timesteps/s  {B*L/med:12,.0f} call env-timesteps/s")
