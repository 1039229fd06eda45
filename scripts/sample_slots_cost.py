#!/usr/bin/env python3
"""Cost of the per-slot sampling table at the headline configuration (xLSTM 16M, 4096 env slots), and whether the
engine-wide path moved when the row code was split into parts.

Three cases on ONE box, each a fresh child process, interleaved round by round (parent, this, table, parent, ...):
  parent   the engine-wide settings (lram_set_sampling alone) on the PARENT commit's library
  this     the same on this commit's library: the same kernel instantiation, so a difference beyond the parent's
           run-to-run spread means the template split leaked into it
  table    a per-slot table (lram_set_sampling_slots) that gives every slot the same settings: same rows, same support
Per case two figures:
  row_us   the row code alone on 4096 * act_dim rows of n_vocab logits (lram_sample_tokens; for `table` lram_sample_rows
           with per-row settings), HIP events around --launches back-to-back launches: the head's work without the step
  step_ms / head_ms   step time armed, and armed minus disarmed, in interleaved blocks as scripts/sample_head_cost.py
The parent's library is csrc/_variants/<--parent>.so (LRAM_LIB_VARIANT; build the parent commit and copy its liblram_hip.so
there).  Without it only `this` and `table` run.  Prints one JSON line: every run, medians, and the parent's spread
(max - min over its runs) beside |this - parent|.

    python scripts/sample_slots_cost.py [--slots 4096] [--rounds 3] [--parent parent]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("lram_set_sampling_slots", "lram_get_sampling_slots", "lram_score_last_sampled", "lram_sample_rows")


def child(args):
    if args.case == "parent":
        os.environ["LRAM_LIB_VARIANT"] = args.parent
    import torch
    from lram_amd import engine, init_state_dict, preset
    if args.case == "parent":          # the parent's library predates these entries
        for name in NEW_SYMBOLS:
            engine._SYMBOLS.pop(name, None)
    spec = preset(args.model)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)               # the same observations in every child: parent and this commit must draw the same tokens
    B, A, V = args.slots, spec.act_dim, spec.n_vocab
    kw = dict(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p)
    eng = engine.Engine(spec, init_state_dict(spec, seed=0), B, device=dev)
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
        if not on:
            eng.set_sampling(None)
            return
        eng.set_sampling(seed=1, **kw)
        if args.case == "table":
            eng.set_sampling_slots(**kw)

    run(args.warmup)
    ms = {False: [], True: []}
    for _ in range(args.blocks):
        for on in (False, True):
            arm(on)
            run(4)
            ms[on].append(run(args.steps))
    # the row code alone, on the logits the last step left
    logits = eng.taps()[2].view(B * A, V).contiguous()
    u = engine.sample_uniforms(1, 0, B, A, 0, device=dev).view(-1).contiguous()

    # (the library entries directly, on buffers made once: no host work between the launches)
    lib, ptr, sp = engine.load_library(), engine._ptr, engine._stream_ptr(dev)
    tok = torch.empty(B * A, dtype=torch.int32, device=dev)
    if args.case == "table":
        full = engine.slot_setting_arrays(B * A, **kw)
        mode = (~full["greedy"]).to(torch.uint8).to(dev)
        t, k, p = (full[name].to(dev) for name in ("temperature", "top_k", "top_p"))

    def rows():
        if args.case == "table":
            rc = lib.lram_sample_rows(ptr(logits), B * A, V, V, ptr(mode), ptr(t), ptr(k), ptr(p), ptr(u), None, ptr(tok), None, sp)
        else:
            rc = lib.lram_sample_tokens(ptr(logits), B * A, V, V, args.temperature, args.top_k, args.top_p, ptr(u), ptr(tok), sp)
        assert rc == 0, lib.lram_last_error()
        return tok

    for _ in range(8):
        tok = rows()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    row_us = []
    for _ in range(args.blocks):
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.launches):
            rows()
        stop.record()
        torch.cuda.synchronize()
        row_us.append(start.elapsed_time(stop) * 1e3 / args.launches)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print(json.dumps({"case": args.case, "step_ms": round(med(ms[True]), 4), "argmax_ms": round(med(ms[False]), 4),
                      "head_ms": round(med(ms[True]) - med(ms[False]), 4), "row_us": round(med(row_us), 3),
                      "row_us_runs": [round(x, 3) for x in row_us], "tokens_sum": int(tok.sum())}))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="xlstm_16m")
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=0.75)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--top-p", type=float, default=0.5)
    ap.add_argument("--parent", default="parent", help="csrc/_variants/<name>.so: the parent commit's library")
    ap.add_argument("--case", choices=["parent", "this", "table"], help="(internal) run one case in this process")
    args = ap.parse_args()
    if args.case:
        child(args)
        return
    have_parent = os.path.exists(os.path.join(ROOT, "lram_amd", "csrc", "_variants", args.parent + ".so"))
    cases = (["parent"] if have_parent else []) + ["this", "table"]
    runs = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c in cases:       # one fresh process at a time
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", c] + sys.argv[1:], capture_output=True,
                                 text=True, timeout=300, check=True).stdout
            runs[c].append(json.loads(out.strip().splitlines()[-1]))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    res = {"model": args.model, "slots": args.slots, "sampling": [args.temperature, args.top_k, args.top_p], "rounds": args.rounds}
    for key in ("row_us", "head_ms", "step_ms"):
        for c in cases:
            res[f"{key}_{c}"] = [r[key] for r in runs[c]]
            res[f"median_{key}_{c}"] = med(res[f"{key}_{c}"])
        if have_parent:
            res[f"parent_spread_{key}"] = round(max(res[f"{key}_parent"]) - min(res[f"{key}_parent"]), 4)
            res[f"this_minus_parent_{key}"] = round(res[f"median_{key}_this"] - res[f"median_{key}_parent"], 4)
    if have_parent:
        res["same_tokens_parent_this"] = runs["parent"][0]["tokens_sum"] == runs["this"][0]["tokens_sum"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
