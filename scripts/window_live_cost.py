"""Context-window inference with a ring position per env slot: what the all-live window step costs against the parent commit's
single-position ring, and what a step costs once slots are parked.

Cases, each a fresh child process, run in alternation for --rounds rounds (parent, this, parent, this, ...; then the live /
small cases in turn):
  parent    the parent commit's library (csrc/_variants/<--parent>.so, LRAM_LIB_VARIANT: build the parent commit and copy its
            liblram_hip.so there), every slot live -- skipped when the file is absent
  this      this tree's library, slots mode "shared", every slot live
  live<n>   this tree's library, slots mode "own", n of --slots slots live (--live, default 512 and 64)
  small<n>  this tree's library, an engine of n slots, every slot live: the row count the parked engine should come down to
A child fills every window (K steps), warms up, and times --steps window steps per pad mode, each ended by a device synchronise;
its figure is the median.  Observations are embeddings, so the state Linear is in no figure.  Prints one line per case and pad mode
-- the median over the rounds with every round's figure -- and the parent's own spread (max - min over its rounds) beside
|this - parent|.

    python scripts/window_live_cost.py [--model xlstm_16m] [--slots 1024] [--timesteps 50] [--rounds 3] [--parent parent]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("lram_window_set_slots", "lram_window_get_slots", "lram_window_copy_slots", "lram_window_swap_slots",
               "lram_window_slot_numel", "lram_window_save_slots", "lram_window_load_slots")
PADS = ("reference", "none")


def child(args):
    case = args.case
    if case == "parent":
        os.environ["LRAM_LIB_VARIANT"] = args.parent
    import torch
    from lram_amd import engine, init_state_dict, preset
    if case == "parent":               # the parent's library predates these entries
        for name in NEW_SYMBOLS:
            engine._SYMBOLS.pop(name, None)
    spec = preset(args.model)
    dev = torch.device("cuda", 0)
    n = int(case[5:]) if case.startswith("small") else int(case[4:]) if case.startswith("live") else args.slots
    B = n if case.startswith("small") else args.slots
    K, D = args.timesteps, spec.d_model
    eng = engine.Engine(spec, init_state_dict(spec, seed=0), B, device=dev)
    eng.alloc_window(K)
    eng.set_window_pad(torch.zeros(D, device=dev), is_embedding=True)
    torch.manual_seed(0)
    obs = torch.rand(B, D, device=dev) * 2 - 1
    rtg, rew = torch.full((B,), 4.5, device=dev), torch.zeros(B, device=dev)
    if case.startswith("live"):
        eng.set_window_slots("own")
    for _ in range(K):                 # every window full, of every slot
        eng.step_window(obs, rtg, rew, pad="none", obs_is_embedding=True)
    if case.startswith("live"):
        eng.set_live(n)
        obs, rtg, rew = obs[:n].contiguous(), rtg[:n].contiguous(), rew[:n].contiguous()
    out = {"case": case, "rows": n}
    for pad in PADS:
        for _ in range(args.warmup):
            eng.step_window(obs, rtg, rew, pad=pad, obs_is_embedding=True)
        ms = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.step_window(obs, rtg, rew, pad=pad, obs_is_embedding=True)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[pad] = round(statistics.median(ms), 4)
    print(json.dumps(out))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="xlstm_16m")
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--timesteps", type=int, default=50)
    ap.add_argument("--live", type=int, nargs="*", default=[512, 64])
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default="parent", help="csrc/_variants/<name>.so: the parent commit's library")
    ap.add_argument("--case", help="(internal) run one case in this process")
    args = ap.parse_args()
    if args.case:
        child(args)
        return
    have_parent = os.path.exists(os.path.join(ROOT, "lram_amd", "csrc", "_variants", args.parent + ".so"))
    groups = [(["parent"] if have_parent else []) + ["this"], [f"{k}{n}" for n in args.live for k in ("live", "small")]]
    runs = {}
    for cases in groups:
        for _ in range(args.rounds):
            for c in cases:            # one fresh process at a time; the first that does not exit cleanly ends the run
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", c] + sys.argv[1:], capture_output=True,
                                   text=True, timeout=240)
                if p.returncode != 0:
                    sys.exit(f"case {c} ended with status {p.returncode}:\n{p.stderr[-2000:]}")
                runs.setdefault(c, []).append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(f"{args.model}, {args.slots} env slots, K = {args.timesteps}: window step, ms, median of {args.steps} calls per process, "
          f"{args.rounds} alternating rounds")
    med = {}
    for c, rs in runs.items():
        for pad in PADS:
            v = [r[pad] for r in rs]
            med[c, pad] = statistics.median(v)
            print(f"  {c:<9s} rows {rs[0]['rows']:>5d}  pad={pad:<9s}  {med[c, pad]:9.3f} ms   rounds {v}")
    for pad in PADS:
        if have_parent:
            v = [r[pad] for r in runs["parent"]]
            print(f"  pad={pad}: |this - parent| = {abs(med['this', pad] - med['parent', pad]):.3f} ms, the parent's own spread "
                  f"(max - min over its rounds) {max(v) - min(v):.3f} ms")
        for n in args.live:
            print(f"  pad={pad}: {n} of {args.slots} live / every slot live = {med[f'live{n}', pad] / med['this', pad]:.3f}; "
                  f"/ an engine of {n} slots = {med[f'live{n}', pad] / med[f'small{n}', pad]:.3f}")


if __name__ == "__main__":
    main()
