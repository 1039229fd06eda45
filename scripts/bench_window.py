"""Context-window inference: what Engine.step_window costs beside the K-timestep Engine.prefill it rides on.

    python scripts/bench_window.py [config] [B] [K] [repeats]      (defaults: xlstm_16m 1024 50 7)

Legs, all in this one process on one warm engine, interleaved (leg a, b, c, d, then again), median of `repeats` each:
  (a) Engine.prefill over [B, K, d_model] embeddings, every env reset        the yardstick
  (b) step_window, pad="reference", every window full                         (a)'s launches behind the ring kernels
  (c) step_window, pad="none", every window full                              the same: full lengths are the dense call
  (d) step_window, pad="none", min(B, K) distinct lengths 1 .. K              one chunk boundary per distinct length
Observations are embeddings in every leg, so the state Linear is in none of them.  Every call ends in a device synchronise.
The lengths of (d) are held by the call itself: env b is reset where b % K == 0 (length 1) and pruned to b % K entries
otherwise (length b % K + 1)."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lram_amd import init_state_dict, preset
from lram_amd.engine import Engine

cfg = sys.argv[1] if len(sys.argv) > 1 else "xlstm_16m"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
K = int(sys.argv[3]) if len(sys.argv) > 3 else 50
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
spec = preset(cfg); sd = init_state_dict(spec, 0)
dev = "cuda:0"
D = spec.d_model
eng = Engine(spec, sd, B, device=dev)
eng.alloc_window(K)
eng.set_window_pad(torch.zeros(D, device=dev), is_embedding=True)
seq = torch.rand(B, K, D, device=dev) * 2 - 1
rtg_seq = torch.full((B, K), 4.5, device=dev); rew_seq = torch.zeros(B, K, device=dev)
obs = seq[:, 0].contiguous(); rtg = rtg_seq[:, 0].contiguous(); rew = rew_seq[:, 0].contiguous()
ones = torch.ones(B, dtype=torch.uint8, device=dev)
ragged_reset = [b % K == 0 for b in range(B)]
ragged_keep = [b % K for b in range(B)]


def fill():
    for _ in range(K):
        eng.step_window(obs, rtg, rew, pad="none", obs_is_embedding=True)


legs = (("a", f"Engine.prefill, {K} timesteps of embeddings", lambda: eng.prefill(seq, rtg_seq, rew_seq, reset_mask=ones, obs_is_embedding=True)),
        ("b", 'step_window pad="reference", full windows', lambda: eng.step_window(obs, rtg, rew, pad="reference", obs_is_embedding=True)),
        ("c", 'step_window pad="none", full windows', lambda: eng.step_window(obs, rtg, rew, pad="none", obs_is_embedding=True)),
        ("d", f'step_window pad="none", {len(set(ragged_keep))} distinct lengths',
         lambda: eng.step_window(obs, rtg, rew, reset=ragged_reset, keep=ragged_keep, pad="none", obs_is_embedding=True)))
times = {k: [] for k, *_ in legs}
fill()
for _, _, fn in legs:      # warm: workspace growth, lane streams, the plan's tables
    fn(); torch.cuda.synchronize()
for rep in range(reps):
    for k, _, fn in legs:
        if k == "a":
            fill()         # (leg d leaves shorter windows behind; ahead of the yardstick, so that no leg alone follows the 50 calls)
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
        if k in ("b", "c"):
            assert min(eng.window().counts) == K
print(f"{cfg}, {B} env slots, K = {K}, median of {reps} interleaved repeats (min .. max), one process, warm")
base = statistics.median(times["a"])
ring_mb = 2 * B * K * D * 4 / 2**20
for k, name, _ in legs:
    t = times[k]
    med = statistics.median(t)
    print(f"({k}) {name:<52s} {med*1e3:8.3f} ms  ({min(t)*1e3:.3f} .. {max(t)*1e3:.3f})  {(med - base)*1e3:+8.3f} ms against (a)  "
          f"{B/med:12,.0f} env-steps/s")
print(f"    the gather reads and writes {ring_mb:.0f} MiB (two passes over B x K x d_model floats)")
