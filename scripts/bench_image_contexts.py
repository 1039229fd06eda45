"""Stored contexts from uint8 frames: what lram_prefill_frames costs beside a prefill from ready embeddings, beside what a caller
had to do without it, at each frame-tile size, and with per-env lengths.

    python scripts/bench_image_contexts.py [config] [B] [L] [repeats] [legs]     (defaults: xlstm_206m 64 512 7 all)

Legs, each warm, median of `repeats`, every call ending in a device synchronise:
  (i)   Engine.prefill(embeddings, obs_is_embedding=True)                      the floor: no CNN at all
  (iii) what a caller does without the frames entries: L Engine.embed_images calls, each on a gather of one timestep's frames,
        the results assembled into [B, L, d_model], then (i)
  (ii)  Engine.prefill_frames(frames) at each LRAM_IMG_TILE candidate          one fresh engine per candidate (read at creation)
  (iv)  Engine.prefill_frames(frames, lengths = B distinct lengths)            at the default tile, beside its dense call
legs = "old": (i) and (iii) only -- every call they make exists on the commit before the frames entries, so the same script times
that commit from its own tree."""
import os, statistics, sys, time
sys.path.insert(0, os.getcwd())
import torch
from lram_amd import init_state_dict, preset
from lram_amd.engine import Engine

cfg = sys.argv[1] if len(sys.argv) > 1 else "xlstm_206m"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
L = int(sys.argv[3]) if len(sys.argv) > 3 else 512
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
which = sys.argv[5] if len(sys.argv) > 5 else "all"
TILES = (128, 256, 512, 1024, 2048)
dev = "cuda:0"
spec = preset(cfg)
sd = init_state_dict(spec, 0, with_image_encoder=True)
g = torch.Generator().manual_seed(1)
frames = torch.randint(0, 256, (B, L, *spec.image_shape), generator=g, dtype=torch.uint8).to(dev)
rtg = torch.full((B, L), 4.5, device=dev); rew = torch.zeros(B, L, device=dev)
ones = torch.ones(B, dtype=torch.uint8, device=dev)
spread = [1 + round(b * (L - 1) / max(1, B - 1)) for b in range(B)]


def timed(fn):
    fn(); torch.cuda.synchronize()          # warm: workspace growth, lane streams, scratch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def line(tag, what, t, n=B * L):
    print(f"({tag:4s}) {what:74s} {t[0]:9.2f} ms  ({t[1]:.2f} .. {t[2]:.2f})  {n / t[0] * 1e3:12,.0f} context env-timesteps/s", flush=True)


print(f"{cfg}, {B} envs x {L} timesteps, frames {spec.image_shape}, median of {reps} (min .. max), warm, legs: {which}", flush=True)
eng = Engine(spec, sd, B, device=dev)


def old_way():
    emb = torch.empty(B, L, spec.d_model, device=dev)
    for l in range(L):
        emb[:, l] = eng.embed_images(frames[:, l].contiguous())
    return eng.prefill(emb, rtg, rew, reset_mask=ones, obs_is_embedding=True)


emb = torch.empty(B, L, spec.d_model, device=dev)
for l in range(L):
    emb[:, l] = eng.embed_images(frames[:, l].contiguous())
floor = timed(lambda: eng.prefill(emb, rtg, rew, reset_mask=ones, obs_is_embedding=True))
line("i", "prefill from ready embeddings", floor)
line("iii", f"{L} embed_images calls on gathered timesteps + prefill(obs_is_embedding)", timed(old_way))
eng.close()
if which != "old":
    results = {}
    for tile in TILES:
        os.environ["LRAM_IMG_TILE"] = str(tile)
        e = Engine(spec, sd, B, device=dev)
        del os.environ["LRAM_IMG_TILE"]
        results[tile] = timed(lambda: e.prefill_frames(frames, rtg, rew, reset_mask=ones))
        line("ii", f"prefill_frames, LRAM_IMG_TILE={tile}: CNN share {results[tile][0] - floor[0]:.2f} ms", results[tile])
        e.close()
    best = min(results, key=lambda k: results[k][0])
    second = sorted(v[0] for v in results.values())[1]
    print(f"       fastest tile {best}: {results[best][0]:.2f} ms, {100 * (second / results[best][0] - 1):.2f} % ahead of the next", flush=True)
    e = Engine(spec, sd, B, device=dev)       # the default tile
    dense = timed(lambda: e.prefill_frames(frames, rtg, rew, reset_mask=ones))
    line("iv", "prefill_frames, dense, default tile", dense)
    e.image_counts(reset=True)
    ragged = timed(lambda: e.prefill_frames(frames, rtg, rew, reset_mask=ones, lengths=spread))
    counts = e.image_counts()
    line("iv", f"prefill_frames, {len(set(spread))} distinct lengths ({sum(spread)} of {B * L} frames)", ragged, sum(spread))
    emb_r = timed(lambda: e.prefill(emb, rtg, rew, reset_mask=ones, obs_is_embedding=True, lengths=spread))
    line("iv", "prefill from ready embeddings, the same lengths", emb_r, sum(spread))
    assert counts["frames"] == (reps + 1) * sum(spread), counts
    print(f"       CNN share: dense {dense[0] - floor[0]:.2f} ms for {B * L} frames, ragged {ragged[0] - emb_r[0]:.2f} ms for {sum(spread)} "
          f"frames: {(ragged[0] - emb_r[0]) / (dense[0] - floor[0]):.3f} of the dense share for {sum(spread) / (B * L):.3f} of the frames", flush=True)
    e.close()
