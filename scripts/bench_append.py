"""Appended stored contexts: what lram_prefill_append costs beside the ragged (replace) entry, what holding slots of length 0 costs
beside saving and loading their records, and what scoring long trajectories window by window costs.

    python scripts/bench_append.py [config] [B] [L] [repeats]      (defaults: xlstm_16m 64 252 7)

Legs, all in this one process on warm engines, interleaved (leg a, b, ... then again), median of `repeats` each:
  (a) Engine.prefill(lengths = 4 distinct lengths)                 lram_prefill_ragged
  (b) the same lengths with append=True, every env restarting      lram_prefill_append
  (c) half the lengths 0, the other half L: the ragged entry       (saves and loads the records of B / 2 slots)
  (d) the same by the append entry                                 (the B / 2 slots are held)
  (e1) RecurrentAgent.score_trajectories, B distinct lengths       one lram_score_ragged call
  (e2) the same with window = L / 4                                4 lram_score_append calls
  (e3) what callers do without either: L lram_step calls
Every call ends in a device synchronise; env-timesteps/s counts the timesteps of the contexts (sum of the lengths)."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lram_amd import init_state_dict, preset
from lram_amd.agent import RecurrentAgent

cfg = sys.argv[1] if len(sys.argv) > 1 else "xlstm_16m"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
L = int(sys.argv[3]) if len(sys.argv) > 3 else 252
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
spec = preset(cfg); sd = init_state_dict(spec, 0)
dev = "cuda:0"
agent = RecurrentAgent(spec, sd, n_envs=B, device=dev)
eng = agent.engine
obs = torch.rand(B, L, spec.state_dim, device=dev) * 2 - 1
rtg = torch.full((B, L), 4.5, device=dev); rew = torch.zeros(B, L, device=dev)
rec = torch.rand(B, L, spec.act_dim, device=dev) * 2 - 1
ones = torch.ones(B, dtype=torch.uint8, device=dev)
obs_t = [obs[:, l].contiguous() for l in range(L)]; rtg_t = [rtg[:, l].contiguous() for l in range(L)]
rew_t = [rew[:, l].contiguous() for l in range(L)]
four = [max(1, L * (4 - (b * 4) // B) // 4) for b in range(B)]
half = [L if b % 2 else 0 for b in range(B)]
spread = [1 + round(b * (L - 1) / max(1, B - 1)) for b in range(B)]
W = max(1, L // 4)


def steps():
    for l in range(L):
        eng.step(obs_t[l], rtg_t[l], rew_t[l], ones if l == 0 else None)


legs = (("a", "lram_prefill_ragged, 4 distinct lengths", lambda: eng.prefill(obs, rtg, rew, reset_mask=ones, lengths=four), four),
        ("b", "lram_prefill_append, the same, all restarting", lambda: eng.prefill(obs, rtg, rew, reset_mask=ones, lengths=four, append=True), four),
        ("c", f"lram_prefill_ragged, {B // 2} lengths 0 (records saved / loaded)", lambda: eng.prefill(obs, rtg, rew, reset_mask=ones, lengths=half), half),
        ("d", f"lram_prefill_append, {B // 2} lengths 0 (held)", lambda: eng.prefill(obs, rtg, rew, reset_mask=ones, lengths=half, append=True), half),
        ("e1", f"score_trajectories, {len(set(spread))} distinct lengths, one call", lambda: agent.score_trajectories(obs, rtg, rew, actions=rec, lengths=spread), spread),
        ("e2", f"score_trajectories(window={W}): {-(-max(spread) // W)} calls", lambda: agent.score_trajectories(obs, rtg, rew, actions=rec, lengths=spread, window=W), spread),
        ("e3", f"{L} lram_step calls", steps, spread))
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
    print(f"({k:<2s}) {name:<62s} {med*1e3:8.2f} ms  ({min(t)*1e3:.2f} .. {max(t)*1e3:.2f})  "
          f"{sum(lengths)/med:12,.0f} context env-timesteps/s")
