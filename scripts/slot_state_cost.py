"""Timing instrument of the per-slot state calls (lram_state_copy_slots / save / load, csrc/slot_state.hip).

HIP-event time of copy, save and load for 1 / 64 / 1024 slots of the 16M geometry and 1 / 64 of the 206M geometry, in both
state modes, next to `lram_stream_copy` over the same number of bytes in the same process (the yardstick: a plain float4
device copy on the same box) and one whole-batch `lram_state_export` of block 0 for scale.  Rates count bytes read plus bytes
written.  Usage: python scripts/slot_state_cost.py [--out profiles/slot_state_cost.txt] [--iters 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lram_amd import init_state_dict, preset          # noqa: E402
from lram_amd import engine as E                      # noqa: E402

LAZY_WINDOW = 48


def timed(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def lazy_extra_floats(spec):
    """Floats a copy moves per slot on top of the record in lazy mode: window rows, the live coefficients and scale, the count."""
    n_mlstm = spec.n_blocks - len(spec.slstm_at)
    return n_mlstm * (2 * spec.n_heads * LAZY_WINDOW * spec.head_dim + spec.n_heads * LAZY_WINDOW + spec.n_heads) + 1


def measure(name, batch, counts, iters, lines):
    spec = preset(name)
    sd = init_state_dict(spec, seed=1)
    g = torch.Generator().manual_seed(5)
    for mode in ("lazy", "eager"):
        eng = E.Engine(spec, sd, batch, device="cuda:0")
        eng.set_state_mode(mode)
        obs = (torch.rand(batch, spec.state_dim, generator=g) * 2 - 1).cuda()
        rtg, rew = torch.full((batch,), 4.5).cuda(), torch.zeros(batch).cuda()
        mask = torch.ones(batch, dtype=torch.uint8).cuda()
        for t in range(8):                                  # windows hold pending tokens when the calls are timed
            eng.step(obs, rtg, rew, mask if t == 0 else None)
        torch.cuda.synchronize()
        numel = eng.slot_state_numel
        rec_bytes = 4 * numel
        copy_bytes = rec_bytes + (4 * lazy_extra_floats(spec) if mode == "lazy" else 0)
        for n in counts:
            src, dst = list(range(n)), list(range(batch - n, batch))
            rec = torch.empty(n, numel, device="cuda")
            scratch_src = torch.empty(n * copy_bytes // 4 + 4, device="cuda")
            scratch_dst = torch.empty_like(scratch_src)
            for what, fn, nbytes in (("copy", lambda: eng.copy_slots(src, dst), copy_bytes),
                                     ("save", lambda: eng.save_slots(src, out=rec), rec_bytes),
                                     ("load", lambda: eng.load_slots(dst, rec), rec_bytes)):
                ms = timed(fn, iters)
                k = n * nbytes // 4 // 4 * 4
                ref = timed(lambda: E.stream_copy(scratch_dst[:k], scratch_src[:k]), iters)
                row = {"model": name, "batch": batch, "mode": eng.state_mode, "what": what, "slots": n,
                       "MB_moved": round(2 * n * nbytes / 1e6, 2), "ms": round(ms, 4), "GBps": round(2 * n * nbytes / ms / 1e6, 1),
                       "stream_copy_ms": round(ref, 4), "stream_copy_GBps": round(2 * n * nbytes / ref / 1e6, 1),
                       "fraction_of_stream_copy": round(ref / ms, 3)}
                lines.append(row)
                print(json.dumps(row), flush=True)
        # for scale: the whole-batch export of ONE tensor of ONE block (the first call folds every pending window of every env)
        for what in ("export_block0_C_whole_batch_first", "export_block0_C_whole_batch_again"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.export_state_tensor(0, 0)
            b.record()
            b.synchronize()
            row = {"model": name, "batch": batch, "mode": eng.state_mode, "what": what, "ms": round(a.elapsed_time(b), 4)}
            lines.append(row)
            print(json.dumps(row), flush=True)
        eng.close()
        del eng
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--only", default=None, help="xlstm_16m or xlstm_206m")
    a = ap.parse_args()
    lines = []
    if a.only in (None, "xlstm_16m"):
        measure("xlstm_16m", 2048, (1, 64, 1024), a.iters, lines)
    if a.only in (None, "xlstm_206m"):
        measure("xlstm_206m", 128, (1, 64), a.iters, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# scripts/slot_state_cost.py: median HIP-event ms; rates count bytes read + written; fraction = stream_copy ms / call ms\n")
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
