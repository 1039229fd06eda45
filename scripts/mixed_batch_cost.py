#!/usr/bin/env python3
"""Cost of mixed-domain batches (slot table, lram_step_slots) at the headline size (xLSTM 16M, 4096 env slots).

  --what mixed   one engine over all slots with a table of two domains (--image-slots image-discrete slots, the rest
                 vector-continuous) against the per-domain engines it replaces: lram_step_images at --image-slots slots
                 plus lram_step at the rest, each stepped on its own.  The variants alternate inside this one process
                 (A B C A B C ...); HIP events around synchronised blocks of steps.
  --what head    steps with the plain head (discrete = 0) or, with --per-slot, the per-slot head over an all-continuous
                 table -- disarmed, then armed with sampling.  Meant to run under
                 `rocprofv3 --kernel-trace --stats -- python scripts/mixed_batch_cost.py --what head [--per-slot]`, once per
                 variant (the kernels of the two variants carry the same names): the per-launch time of
                 action_argmax_kernel / action_sample_kernel is read from the trace's statistics.

Prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from lram_amd import init_state_dict, preset  # noqa: E402
from lram_amd.engine import Engine  # noqa: E402


def timed(fn, n):
    """ms per call over n calls, HIP events around the synchronised block."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def inputs(spec, B, dev, image):
    g = torch.Generator(device=dev).manual_seed(B)
    if image:
        obs = torch.randint(0, 256, (B, *spec.image_shape), generator=g, device=dev, dtype=torch.uint8)
    else:
        obs = torch.rand(B, spec.state_dim, generator=g, device=dev) * 2 - 1
    return obs, torch.full((B,), 4.5, device=dev), torch.zeros(B, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["mixed", "head"], default="mixed")
    ap.add_argument("--model", default="xlstm_16m")
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--image-slots", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--per-slot", action="store_true")
    args = ap.parse_args()
    spec = preset(args.model)
    dev = torch.device("cuda", 0)
    B, n_img = args.slots, args.image_slots
    out = {"what": args.what, "model": args.model, "slots": B, "steps_per_block": args.steps,
           "library": os.environ.get("LRAM_LIB_VARIANT", "tree")}
    if args.what == "head":
        eng = Engine(spec, init_state_dict(spec, seed=0), B, device=dev)
        obs, rtg, rew, mask = inputs(spec, B, dev, False)
        head = False
        if args.per_slot:
            eng.set_slot_table([False] * B, [spec.act_dim] * B, None)
            head = "per_slot"
        step = lambda: eng.step(obs, rtg, rew, mask, discrete=head)  # noqa: E731
        timed(step, args.warmup)
        res = {}
        for name, arm in (("argmax", None), ("sampling", 0.75)):
            eng.set_sampling(arm, 10, 0.5, seed=1) if arm else eng.set_sampling(None)
            timed(step, 4)
            res[name] = [round(timed(step, args.steps), 4) for _ in range(args.blocks)]
        out.update(head="per_slot" if args.per_slot else "plain", ms_per_step=res,
                   median_ms={k: round(median(v), 4) for k, v in res.items()})
        print(json.dumps(out))
        eng.close()
        return
    sd = init_state_dict(spec, seed=0, with_image_encoder=True)
    mixed, e_img, e_vec = Engine(spec, sd, B, device=dev), Engine(spec, sd, n_img, device=dev), Engine(spec, sd, B - n_img, device=dev)
    mixed.set_slot_table([True] * n_img + [False] * (B - n_img), [1] * n_img + [spec.act_dim] * (B - n_img),
                         [True] * n_img + [False] * (B - n_img))
    vo, vr, vw, vm = inputs(spec, B, dev, False)
    io, ir, iw, im = inputs(spec, n_img, dev, True)
    so, sr, sw, sm = inputs(spec, B - n_img, dev, False)
    runs = {
        "mixed_step_slots": lambda: mixed.step_slots(vo, io, vr, vw, vm),
        "image_engine_step_images": lambda: e_img.step_images(io, ir, iw, im, discrete=True),
        "vector_engine_step": lambda: e_vec.step(so, sr, sw, sm, discrete=False),
    }
    for fn in runs.values():
        timed(fn, args.warmup)
    ms = {k: [] for k in runs}
    for _ in range(args.blocks):
        for k, fn in runs.items():
            timed(fn, 2)
            ms[k].append(round(timed(fn, args.steps), 4))
    med = {k: median(v) for k, v in ms.items()}
    parts = med["image_engine_step_images"] + med["vector_engine_step"]
    out.update(image_slots=n_img, ms_per_step=ms, median_ms={k: round(v, 4) for k, v in med.items()},
               per_domain_sum_ms=round(parts, 4), mixed_over_per_domain_sum=round(med["mixed_step_slots"] / parts, 4),
               env_steps_per_s={"mixed": round(B / med["mixed_step_slots"] * 1e3), "per_domain_engines": round(B / parts * 1e3)},
               state_modes=[e.state_mode for e in (mixed, e_img, e_vec)])
    print(json.dumps(out))
    for e in (mixed, e_img, e_vec):
        e.close()


if __name__ == "__main__":
    main()
