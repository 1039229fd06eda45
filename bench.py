#!/usr/bin/env python3
"""bench.py -- env-steps/sec (action-inference) of the recurrent rollout hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Both forms run N ranks.  Started WITHOUT a torchrun environment (no WORLD_SIZE) and with --gpus N > 1, this process
never touches the GPU: it starts N fresh child processes of itself (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set,
rendezvous on 127.0.0.1), relays rank 0's JSON line and exits non-zero if any rank does (`launch_ranks`).  Started
WITH WORLD_SIZE set, WORLD_SIZE must equal --gpus; a mismatch is refused, not papered over.  The line carries
`ranks_seen` = an all-reduce of one 1 per rank, so a mislabelled single-rank run cannot pass for N GPUs.

A "step" is one pass of the hot path over one batch of synthetic env inputs: B env slots per GPU each advance one
timestep (embed (s, rtg, r) -> 3 recurrent token steps through the block stack -> action head -> argmax ->
de-tokenise), plus, for N > 1, the all-gather of the action tensor (RCCL).  Workload = BASELINE.json's metric
configuration: xLSTM[7:1] 16M, batch 4096 env slots per GPU (weak scaling).

`value`: inputs (observations, returns-to-go, reset masks for every step) are resident in HBM before the timed region
starts; K steps are enqueued back to back between barrier + synchronize on both sides; max over ranks.

A plain run does only what `value` needs: set up, prime and warm up, time the K steps, write `--dump-outputs`, print the
line.  The line also carries what the timed region measures anyway (the sampled state-pass events behind `roofline`, the
GEMM dispatch counters).  `--full` adds every measurement that takes time of its own, after the timed region: `host_io`,
`roofline.standalone`, the STREAM-like ceilings, `configs` (BASELINE configurations 2-5), `cpu_baseline` and, where the
steps all-gather (N > 1 or LRAM_DIST_SINGLE_RANK=1), `collective`.  `--no-cpu-baseline`, `--no-configs`,
`--no-stream-ceilings` and `--host-io-steps 0` leave single ones out of a --full run.
`host_io` (--full; extra object, rank 0's GPU): SURVEY.md 8d's host-inclusive variant of the same step, measured in the
same run -- observations / returns-to-go / masks in pinned host memory, H2D copies, lram_step, D2H of the actions, host
synchronisation EVERY step (so launch ramp and PCIe are inside the time).  It is reported beside `value`, never as it.

`roofline` (dominant kernel = the mLSTM state pass, HIP-event timed on the stream it is launched on, inside the timed
region): `achieved` = the bytes that kernel's algorithm has to move per launch / its average
launch time, so `frac` <= 1 is HBM utilisation.  In the lazy matrix-memory mode the algorithm moves fewer bytes than
SURVEY 8d's materialised read+write figure; the 8d-equivalent rate is reported apart as `effective_8d_GBps`.
`traffic` = HBM bytes per launch from a separate rocprofv3 --pmc pass (profiles/, `traffic_source`), never measured
in this process.  `cpu_baseline` (--full): the CPU oracle timed on the host cores on a bounded sample (rank 0, N = 1 only).

`--dump-outputs DIR`: right after the timed region, rank 0 writes what the last timed step handed its caller -- the actions
[global batch, act_dim] and their token ids -- to DIR/actions.npy and DIR/tokens.npy.  Every input is seeded, so two builds
run with the same arguments can be compared file for file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

# image observations: lram_step_images (one call) unless LRAM_BENCH_TWO_CALL_IMAGES=1 (lram_embed_images + lram_step: A/B of the two)
TWO_CALL_IMAGES = os.environ.get("LRAM_BENCH_TWO_CALL_IMAGES", "0") == "1"

HBM_PEAK_GBPS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s float4 copy measured)
LAZY_PERIOD = 13        # engine default fold period (lram_set_state_mode)


GEMM_KINDS = {   # LRAM_GEMM (engine.hip::finalize); every kind is fp32-accurate, checked against fp64 in tests/
    "f16x2": "as fp32-accurate 2-way f16-split products on the f16 matrix cores (f16x2: rows scaled by a power of two, "
             "3 MFMA products per fp32 product)",
    "bf16x3": "as fp32-accurate 3-way bf16-split products on the bf16 matrix cores (bf16x3: 6 MFMA products per fp32 product)",
    "f32": "on the exact fp32 MFMA (k-ordered fma chain)",
}
MFMA_PEAK_PFLOPS = 2.5   # dense f16 / bf16 matrix-core peak of MI355X (MI355X_MICROARCH.md; the 2:1-sparsity figure is not used)


def projection_label(ran, env_kind):
    """Which projection kernels served the timed region, from the engine's own dispatch counters (lram_gemm_counts) --
    the dispatcher takes f16x2 only from 1024 operand rows (512 for wide weights), bf16x3 for the batched per-head
    GEMMs of the sLSTM block and for fewer rows, the fp32 few-row / GEMV kernels below 385 rows -- not from LRAM_GEMM."""
    if not ran:
        return GEMM_KINDS[env_kind]
    tot = sum(v["flop"] for v in ran.values()) or 1.0
    main = max(ran, key=lambda k: ran[k]["flop"])
    desc = {"f16x2": GEMM_KINDS["f16x2"], "bf16x3": GEMM_KINDS["bf16x3"], "f32": GEMM_KINDS["f32"],
            "few_row_f32": "on the exact fp32 MFMA (few-row kernel: one 32 x 32 tile per workgroup, operands in registers)"}[main]
    rest = ", ".join(f"{k} {100.0 * v['flop'] / tot:.0f} %" for k, v in ran.items() if v["flop"] > 0 and k != main)
    return desc + f" ({100.0 * ran[main]['flop'] / tot:.0f} % of the projection FLOPs" + (f"; {rest}" if rest else "") + ")"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# ---- algorithmic bytes of the dominant kernel (per env slot, per launch = one block, T tokens) ------------------
def cell_bytes_materialised(spec, T):
    """mlstm_cell_kernel: matrix memory C read once + written once, q/k/v read, h written, gate scalars read.
    This is SURVEY.md 8d's per-block state term."""
    return 2 * spec.n_heads * spec.head_dim ** 2 * 4 + T * 4 * spec.inner * 4 + T * spec.n_heads * 16


def cell_bytes_lazy(spec, T, period=LAZY_PERIOD, r2_model=False):
    """Lazy state pass = mlstm_lazy_cell_kernel + its share of mlstm_lazy_fold_kernel:
    C_base read once; the pending window (steady-state mean T (period - 1) / 2 tokens): its V rows for the window
    attention and -- head dims whose read pass computes the window scores itself (128 / 256: one column slice per head) --
    its khat rows for q . khat_j; q, v read, h written, the step's khat / v rows appended; plus 1/period of a fold (C_base
    read + written, the whole window's khat and v rows read).
    r2_model: the figure rounds 1-2 reported, which left the khat rows out (it dated from the separate score kernel and
    counted that kernel's 3 KB of score rows instead); kept beside the corrected one for continuity."""
    nh, dh, inner = spec.n_heads, spec.head_dim, spec.inner
    c = nh * dh * dh * 4
    mean_pending = T * (period - 1) / 2.0
    fused_scores = dh in (128, 256) and not r2_model
    window = mean_pending * inner * 4 * (2 if fused_scores else 1)
    read_pass = c + window + 3 * T * inner * 4 + 2 * T * inner * 4 + (0 if fused_scores else T * nh * 64 * 4)
    fold = 2 * c + 2 * T * period * inner * 4
    return read_pass + fold / period


def ssm_bytes(spec, T):
    return 2 * spec.d_inner * spec.d_state * 4 + T * (4 * spec.d_inner + 2 * spec.d_state) * 4


# ---- CPU baseline ------------------------------------------------------------------------------------------
def cpu_baseline(spec, sd, seconds_budget=22.0):
    """The oracle (oracle/dt_ref.py, the parity checker) timed on the host cores: `kind: port`.  SURVEY 8d asks for the
    config batch with 8 + 32 steps; at the oracle's rate that is most of an hour for 4096 envs, so the sample is bounded
    (task statement: 10-30 s of CPU work): throughput at B = 256 over as many timesteps as fit the budget, plus the
    B = 1 per-step latency (the reference's real operating point, src/callbacks/evaluation.py:80)."""
    from oracle.dt_ref import OraclePolicy
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1

    def inputs(B):
        g = torch.Generator().manual_seed(1234)
        return torch.rand(B, spec.state_dim, generator=g) * 2 - 1, torch.full((B,), 4.5), torch.zeros(B)

    def timed_steps(B, nthreads, max_s, max_n, warm=1):
        torch.set_num_threads(nthreads)
        obs, rtg, rew = inputs(B)
        ora = OraclePolicy(spec, sd)
        for _ in range(warm):
            ora.step(obs, rtg, rew)
        t0, n = time.time(), 0
        while n < max_n and (n == 0 or time.time() - t0 < max_s):
            ora.step(obs, rtg, rew)
            n += 1
        return n, time.time() - t0

    # PyTorch-eager on many small ops does not scale to every core of a big host: calibrate the thread count on one
    # timestep each (smallest first, stop when it gets slower), then time with the best.
    cal = []
    for thr in sorted({min(avail, c) for c in (8, 16, 32, 64, 128)}):
        n, w = timed_steps(64, thr, 60.0, 2)    # two timesteps after one warm-up: one alone flipped between 8 and 32 threads
        w /= max(n, 1)                          # from box to box (round 3)
        cal.append((w, thr))
        if w > 1.5 * min(c[0] for c in cal):
            break
    # the best thread count at B = 64 is not always the best at the sample's B = 256 (round 5: 16 vs 32 threads): the two
    # fastest candidates each get half of the budget at the sample's batch, the faster one is reported
    B = 256
    tried = []
    for _, thr in sorted(cal)[:2]:
        n, wall = timed_steps(B, thr, (seconds_budget - 6.0) / 2, 16)
        tried.append((B * n / wall, thr, n, wall))
    _, best_thr, n, wall = max(tried)
    n1, wall1 = timed_steps(1, min(best_thr, 8), 3.0, 32, warm=3)
    return {"value": B * n / wall, "unit": "env-steps/s", "cores": best_thr, "kind": "port",
            "sample": f"CPU oracle (PyTorch-eager fp32 restatement of the same path), same model and weights, "
                      f"B={B} envs x {n} timesteps after 1 warm-up, {wall:.1f} s wall, {best_thr} torch threads "
                      f"(8/16/32/64/128 threads calibrated at B=64, the two fastest timed at this batch, the faster reported; host exposes {avail} cores); SURVEY 8d's 8+32 steps "
                      f"at the config batch would take ~{(8 + 32) * 4096 / max(B * n / wall, 1e-9) / 60:.0f} min, hence "
                      f"the bounded sample",
            "b1_latency_ms": wall1 / n1 * 1e3,
            "b1_sample": f"B=1, {n1} timesteps after 3 warm-up, {min(best_thr, 8)} threads"}



# ---- the other BASELINE configurations, timed in the same run ---------------------------------
PER_PRODUCT = {"f16x2": 3, "bf16x3": 6, "f32": 1, "few_row_f32": 1}   # matrix-core products issued per fp32 product


def state_pass_roofline(spec, T, lazy, main_ms, n_main, aux_ms, n_aux, steps, envs_total):
    """Roofline block of one configuration's dominant kernel from its live HIP-event timing (lram_profile_end_split): the
    bytes one launch has to move over its mean duration; the lazy mode's fold launches are shared
    out over the state-pass launches."""
    if spec.backbone == "xlstm":
        n_rec = spec.n_blocks - len(spec.slstm_at)
        per_env = cell_bytes_lazy(spec, T) if lazy else cell_bytes_materialised(spec, T)
        kname = "mlstm_lazy_cell_kernel + its share of mlstm_lazy_fold_kernel" if lazy else "mlstm_cell_kernel"
    else:
        n_rec, per_env, kname = spec.n_blocks, ssm_bytes(spec, T), "mamba_ssm_lane_kernel (selective state update)"
    r = {"bound": "hbm", "kernel": kname, "achieved": None, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": None,
         "traffic": None, "algorithmic_bytes_per_env_per_launch": per_env}
    if n_main > 0:
        launches_per_step = n_main / steps
        envs_per_launch = envs_total * n_rec / launches_per_step
        avg = main_ms / n_main + (aux_ms / n_main if n_aux else 0.0)
        ab = per_env * envs_per_launch
        r.update(algorithmic_bytes_per_launch=ab, envs_per_launch=envs_per_launch, launches_per_step=launches_per_step,
                 avg_launch_ms=avg, launches_timed=n_main, achieved=ab / (avg * 1e-3) / 1e9)
        r["frac"] = r["achieved"] / HBM_PEAK_GBPS
    return r


def mfma_block(gemm_ran, seconds):
    """Matrix-core work of the projections (engine dispatch counters) over a measured interval."""
    flops = sum(v["flop"] for v in gemm_ran.values())
    issued = sum(v["flop"] * PER_PRODUCT[k] for k, v in gemm_ran.items())
    return {"bound": "mfma", "fp32_equiv_flop": flops, "issued_flop": issued, "achieved": issued / seconds / 1e15,
            "peak": MFMA_PEAK_PFLOPS, "unit": "PFLOP/s", "frac": issued / seconds / 1e15 / MFMA_PEAK_PFLOPS,
            "note": "issued matrix-core FLOPs of the projections (3 f16 products per fp32 product on the f16x2 kernels) over the "
                    "WHOLE measured interval, every other kernel's time included"}


def _leg_inputs(spec, B, n_steps, ep_len, rtg0, drtg, native, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    ring = torch.zeros(4, B, spec.state_dim, device=dev)
    ring[:, :, :native] = torch.rand(4, B, native, generator=g, device=dev) * 2 - 1
    age = (torch.arange(B, device=dev).view(1, -1) % ep_len + torch.arange(n_steps, device=dev).view(-1, 1)) % ep_len
    masks = (age == 0).to(torch.uint8).contiguous()
    masks[0] = 1
    return ring, (rtg0 - age.float() * drtg).contiguous(), masks, g


def step_leg(tag, cfg, B, K, W, dev, ep_len, rtg0, drtg, native, image=False, compat_act_dim=0, what=""):
    """One BASELINE configuration as K timed lram_step calls on a fresh engine (inputs resident in HBM, the state pass
    HIP-event timed on every 2nd step), engine destroyed afterwards."""
    from lram_amd import init_state_dict, preset
    from lram_amd.engine import Engine
    spec = preset(cfg)
    sd = init_state_dict(spec, seed=0, with_image_encoder=image)
    eng = Engine(spec, sd, B, device=dev)
    try:
        return _step_leg_run(eng, spec, tag, cfg, B, K, W, dev, ep_len, rtg0, drtg, native, image, compat_act_dim, what)
    finally:   # (a leg that fails must not leave its state -- up to 57 GB at 206M / 512 slots -- behind for the next one)
        eng.close()
        del eng, sd
        torch.cuda.empty_cache()


def _step_leg_run(eng, spec, tag, cfg, B, K, W, dev, ep_len, rtg0, drtg, native, image, compat_act_dim, what):
    T = spec.tokens_per_step
    prime = 16 if eng.state_mode == "lazy" else 2
    ring, rtgs, masks, g = _leg_inputs(spec, B, prime + W + K, ep_len, rtg0, drtg, native, dev, 4321)
    zero = torch.zeros(B, device=dev)
    if image:
        frames = torch.randint(0, 256, (2, B, 3, 64, 64), generator=g, device=dev, dtype=torch.uint8)
        emb = torch.empty(B, spec.d_model, device=dev)
    if compat_act_dim:
        eng.set_compat_mode(compat_act_dim, True)

    def one(t):
        if image and TWO_CALL_IMAGES:
            eng.embed_images(frames[t % 2], emb)
            eng.step(emb, rtgs[t], zero, masks[t], discrete=True, obs_is_embedding=True)
        elif image:
            eng.step_images(frames[t % 2], rtgs[t], zero, masks[t], discrete=True)
        else:
            eng.step(ring[t % 4], rtgs[t], zero, masks[t])

    for t in range(prime + W):
        one(t)
    torch.cuda.synchronize()
    eng.profile_begin_sampled(2)
    eng.gemm_counts(reset=True)
    t0 = time.perf_counter()
    for t in range(prime + W, prime + W + K):
        one(t)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ran = eng.gemm_counts()
    main_ms, n_main, aux_ms, n_aux = eng.profile_end_split()
    lazy = eng.state_mode == "lazy"
    leg = {"id": tag, "workload": what or f"{cfg}, {B} env slots", "preset": cfg, "batch": B, "steps": K, "warmup": W + prime,
           "value": B * K / wall, "unit": "env-steps/s", "ms_per_step": wall / K * 1e3,
           "state_mode": eng.state_mode if spec.backbone == "xlstm" else None,
           "projections": projection_label(ran, "f16x2"),
           # (the reference Mamba trajectory runs `compat_act_dim` forwards per env-step: that many state passes over every env)
           "roofline": state_pass_roofline(spec, T, lazy, main_ms, n_main, aux_ms, n_aux, len(range(0, K, 2)),
                                           B * max(1, compat_act_dim)),
           "mfma": mfma_block(ran, wall)}
    if spec.backbone == "xlstm":
        leg["whole_step_8d_GBps"] = (2 * spec.state_bytes_per_env() + 4 * spec.state_dim + 4 * spec.act_dim) * leg["value"] / 1e9
    return leg


def prefill_leg(tag, cfg, B, L, n_decode, dev, what=""):
    """BASELINE config 5: lram_prefill of L stored timesteps (3 L tokens; chunkwise-parallel kernels) on B envs, then n_decode
    single steps from the prefilled state.  `value` = env-timesteps/s of the prefill; the decode steps are reported beside it."""
    from lram_amd import init_state_dict, preset
    from lram_amd.engine import Engine
    spec = preset(cfg)
    sd = init_state_dict(spec, seed=0)
    eng = Engine(spec, sd, B, device=dev)
    try:
        leg = _prefill_leg_run(eng, spec, tag, cfg, B, L, n_decode, dev, what)
    finally:
        eng.close()
        del eng
        torch.cuda.empty_cache()
    # the same state pass with the chip to itself: one chunk at a time (LRAM_PREFILL_CHUNK=3), one un-timed prefill under events
    if leg.get("roofline"):
        old = os.environ.get("LRAM_PREFILL_CHUNK")
        os.environ["LRAM_PREFILL_CHUNK"] = "3"
        try:
            solo = Engine(spec, sd, B, device=dev)
        finally:
            if old is None:
                del os.environ["LRAM_PREFILL_CHUNK"]
            else:
                os.environ["LRAM_PREFILL_CHUNK"] = old
        try:
            obs, rtg, rew, ones = _prefill_inputs(spec, B, L, dev)
            solo.prefill(obs, rtg, rew, ones)
            solo.profile_begin()
            solo.prefill(obs, rtg, rew, ones)
            torch.cuda.synchronize()
            ms, n, _, _ = solo.profile_end_split()
            if n > 0:
                r = leg["roofline"]
                ach = r["algorithmic_bytes_per_launch"] / (ms / n * 1e-3) / 1e9
                r["standalone"] = {"avg_launch_ms": ms / n, "achieved": ach, "frac": ach / HBM_PEAK_GBPS, "launches_timed": n,
                                   "note": "one chunk at a time: the launch has the chip to itself"}
        finally:
            solo.close()
            del solo
            torch.cuda.empty_cache()
    return leg


def _prefill_inputs(spec, B, L, dev):
    g = torch.Generator(device=dev).manual_seed(77)
    obs = torch.zeros(B, L, spec.state_dim, device=dev)
    obs[:, :, :168] = torch.rand(B, L, 168, generator=g, device=dev) * 2 - 1          # Mimicgen: 168-dim full state space
    rtg = (6.0 - 0.01 * torch.arange(L, device=dev).float()).repeat(B, 1).contiguous()
    rew = torch.zeros(B, L, device=dev)
    ones = torch.ones(B, dtype=torch.uint8, device=dev)
    return obs, rtg, rew, ones


def _prefill_leg_run(eng, spec, tag, cfg, B, L, n_decode, dev, what):
    obs, rtg, rew, ones = _prefill_inputs(spec, B, L, dev)
    eng.prefill(obs, rtg, rew, ones)                                                   # warm-up pass (allocations, first launches)
    torch.cuda.synchronize()
    eng.gemm_counts(reset=True)
    t0 = time.perf_counter()
    eng.prefill(obs, rtg, rew, ones)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ran = eng.gemm_counts()
    o1, r1, z1 = obs[:, 0].contiguous(), rtg[:, -1].contiguous(), torch.zeros(B, device=dev)
    for _ in range(2):
        eng.step(o1, r1, z1, None)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(n_decode):
        eng.step(o1, r1, z1, None)
    torch.cuda.synchronize()
    wall_d = time.perf_counter() - t1
    # the chunkwise state pass (mlstm_cell_chunk3_kernel: C of every (env, head) read once and written once per chunk) timed by
    # live HIP events in a THIRD, un-timed prefill (the events sit on the chunk lanes' streams): its own roofline
    roof = None
    if spec.backbone == "xlstm":
        eng.profile_begin()
        eng.prefill(obs, rtg, rew, ones)
        torch.cuda.synchronize()
        ms, n, _, _ = eng.profile_end_split()
        if n > 0:
            n_rec = spec.n_blocks - len(spec.slstm_at)
            chunks = n / n_rec                                     # state passes per block
            tok = 3.0 * L / chunks                                 # tokens per pass (mean)
            per_env = 2 * spec.n_heads * spec.head_dim ** 2 * 4 + tok * 4 * spec.inner * 4 + spec.n_heads * 64 * 64 * 4
            ab, avg = per_env * B, ms / n
            roof = {"bound": "hbm", "kernel": "mlstm_cell_chunk3_kernel (chunkwise state pass, bf16x3)", "achieved": ab / (avg * 1e-3) / 1e9,
                    "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": ab / (avg * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": None,
                    "algorithmic_bytes_per_launch": ab, "avg_launch_ms": avg, "launches_timed": n, "state_passes_per_block": chunks,
                    "note": "C read + written once per pass, q / k / v read and h written for its tokens, the 64 x 64 intra-chunk "
                            "matrix; three chunks are in flight, so a launch shares the chip with the other lanes' kernels"}
    leg = {"id": tag, "workload": what or f"{cfg} prefill", "preset": cfg, "batch": B, "context_timesteps": L,
           "steps": 1, "warmup": 1, "value": B * L / wall, "unit": "env-timesteps/s", "ms_per_step": wall * 1e3,
           "roofline": roof,
           "projections": projection_label(ran, "f16x2"), "mfma": mfma_block(ran, wall),
           "decode": {"steps": n_decode, "ms_per_step": wall_d / n_decode * 1e3, "value": B * n_decode / wall_d,
                      "unit": "env-steps/s", "state_mode": eng.state_mode}}
    return leg


def config_legs(dev):
    """BASELINE.json `configs` 2-5 at their per-GPU sizes, one fresh engine each (the headline's is closed first)."""
    legs = []
    plan = [
        lambda: step_leg("C2", "xlstm_16m", 1024, 48, 4, dev, 1000, 4.51274, 0.01, 17,
                         what="xLSTM[7:1] 16M, DMControl cheetah-run-shaped obs, continuous head, 1024 env slots"),
        lambda: step_leg("C3", "mamba_48m", 2048, 32, 4, dev, 200, 6.50346, 0.005, 39,
                         what="Mamba 48M, Meta-World-shaped obs (39 dims), 2048 env slots, one state advance per env-step"),
        lambda: step_leg("C3-reference-trajectory", "mamba_48m", 2048, 12, 2, dev, 200, 6.50346, 0.005, 39, compat_act_dim=4,
                         what="Mamba 48M, 2048 env slots, the reference Mamba agent's trajectory (src/algos/decision_mamba.py:"
                              "107-122: one forward per action dim = 4 per env-step on Meta-World, layer-0-only resets)"),
        lambda: step_leg("C4-per-gpu-shard", "xlstm_206m", 512, 12, 2, dev, 1000, 3.0, 0.001, 0, image=True,
                         what="xLSTM[7:1] 206M, Atari-shaped uint8 [3,64,64] frames -> IMPALA-CNN -> 18-way discrete head, "
                              "512 env slots = one GPU's shard of BASELINE's 4096 over 8"),
        lambda: prefill_leg("C5", "xlstm_206m", 64, 512, 16, dev,
                            what="xLSTM 206M, Mimicgen-shaped obs: lram_prefill of 512 timesteps (1536 tokens, chunkwise-parallel) "
                                 "on 64 envs, then 16 single-step decodes"),
    ]
    for fn in plan:
        t0 = time.time()
        try:
            leg = fn()
        except Exception as ex:   # a leg that cannot run says so on the line instead of taking the headline down with it
            leg = {"id": "?", "error": f"{type(ex).__name__}: {ex}"}
        leg["leg_wall_s"] = time.time() - t0
        log("[bench] config leg:", json.dumps({k: leg.get(k) for k in ("id", "value", "unit", "ms_per_step", "leg_wall_s", "error")}))
        legs.append(leg)
    return legs


# ---- the run ------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4096, help="env slots per GPU")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="strong scaling: total env slots, split over the ranks with lram_amd.dist.shard_bounds "
                         "(overrides --batch; BASELINE C4: 4096 over 8 GPUs)")
    ap.add_argument("--config", default="xlstm_16m", help="preset name (lram_amd.config.preset)")
    ap.add_argument("--obs", choices=("state", "image"), default="state",
                    help="image: uint8 [3,64,64] frames through the IMPALA-CNN front end + 18-way discrete head "
                         "(BASELINE C4, Atari-shaped)")
    ap.add_argument("--state", choices=("auto", "lazy", "eager"), default="auto",
                    help="mLSTM matrix-memory representation (lram_set_state_mode); auto = lazy where the state pass dominates")
    ap.add_argument("--graph", action="store_true", help="replay the step as a hipGraph")
    ap.add_argument("--micro", type=int, default=0, help="env slices pipelined on separate streams (0 = auto, 1 = off)")
    ap.add_argument("--side-stream", action="store_true", help="issue the steps on a non-default HIP stream")
    ap.add_argument("--mamba-compat", action="store_true",
                    help="Mamba: the reference agent's trajectory (one forward per action dim, layer-0-only resets; "
                         "lram_set_compat_mode) instead of one state advance per env-step")
    ap.add_argument("--env-act-dim", type=int, default=0, help="action dims the env uses (compat forwards per step)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also take every measurement that needs time of its own: the host-inclusive "
                         "leg, the state pass with the chip to itself, the STREAM-like ceilings, the `configs` legs, the CPU "
                         "baseline and the collective report.  Without it the run times the headline and nothing else")
    ap.add_argument("--host-io-steps", type=int, default=48, help="--full: steps of the host-inclusive leg (0 = skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline (and the `configs` legs)")
    ap.add_argument("--no-configs", action="store_true",
                    help="--full: skip the `configs` legs (BASELINE configs 2-5 at their per-GPU sizes; they run on default-workload "
                         "N = 1 runs that also take the CPU baseline)")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--timing-every", type=int, default=4,
                    help="live HIP-event timing of the dominant kernel on every n-th step of the timed region (1 = every step)")
    ap.add_argument("--kernel-timing", action="store_true", help="keep the live state-pass timing below 256 env slots")
    ap.add_argument("--no-stream-ceilings", action="store_true", help="--full: skip the STREAM-like ceilings")
    ap.add_argument("--engine-factory", default="",
                    help="test hook: 'file.py:attr' or 'module:attr' of a stand-in engine factory(spec, batch, device); the "
                         "run then stays on the CPU over gloo (tests/test_dist_rollout.py).  Never used on the product path")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy "
                         "(actions, tokens; see dump_outputs), so that two builds can be compared output for output")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy, floating point as float32, integers as float64 (token ids stay
    exact).  All arrays share their first (env slot) axis.  Above DUMP_LIMIT_BYTES in all, every array keeps the same fixed
    sample of rows (seed 0, ascending) and out_dir/rows.npy holds their indices; the files never exceed the limit."""
    import numpy as np
    host = {k: v.detach().cpu() for k, v in arrays.items() if v is not None}
    host = {k: v.to(torch.float32 if v.is_floating_point() else torch.float64) for k, v in host.items()}
    n = next(iter(host.values())).shape[0]
    row_bytes = sum(v[0].numel() * v.element_size() for v in host.values())
    rows = None
    if n * row_bytes > DUMP_LIMIT_BYTES:
        keep = DUMP_LIMIT_BYTES // (row_bytes + 8)          # (+ 8: the row's index in rows.npy)
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:keep].sort().values
        host = {k: v[rows] for k, v in host.items()}
        host["rows"] = rows.to(torch.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, v in host.items():
        np.save(os.path.join(out_dir, name + ".npy"), v.numpy())
    log(f"[bench] wrote {', '.join(sorted(host))} to {out_dir}")


def _resolve_factory(ref):
    mod, _, attr = ref.rpartition(":")
    if mod.endswith(".py"):
        import importlib.util
        sp = importlib.util.spec_from_file_location("_bench_engine_factory", mod)
        m = importlib.util.module_from_spec(sp)
        sp.loader.exec_module(m)
    else:
        import importlib
        m = importlib.import_module(mod)
    return getattr(m, attr)


def launch_ranks(args, argv, timeout_s=3600.0):
    """--gpus N > 1 from a plain process: start N ranks of this script, one per GPU, and relay rank 0's line.

    The parent does not call into torch.cuda / HIP at all (the children are fork+exec'd from it; a process that has
    initialised the GPU must not exec).  Children get the torchrun variables; stdout of rank 0 is captured and
    re-printed, every other stream is inherited.  The first rank that exits non-zero ends the job: the remaining
    children are terminated by PID and the parent exits with that code.  Returns rank 0's parsed JSON line."""
    import socket
    import subprocess
    import threading
    n = args.gpus
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    script = os.path.abspath(__file__)
    cmd = [sys.executable, script] + list(argv)
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this pool (RCCL needs it)
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0)))
    log(f"[bench] launcher: started {n} ranks (pids {[p.pid for p in procs]}), rendezvous 127.0.0.1:{port}")
    captured = []
    reader = threading.Thread(target=lambda: captured.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    t0, failed = time.time(), None
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            failed = bad[0]
            break
        if all(c == 0 for c in codes):
            break
        if time.time() - t0 > timeout_s:
            failed = (-1, 124)
            break
        time.sleep(0.1)
    if failed is not None:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(10)
            except subprocess.TimeoutExpired:
                p.kill()
        raise SystemExit(f"[bench] rank {failed[0]} exited with code {failed[1]}; job aborted")
    reader.join(10)
    text = captured[0] if captured else ""
    line = None
    for ln in text.splitlines():
        if ln.startswith("{"):
            line = ln
    if line is None:
        raise SystemExit("[bench] rank 0 printed no JSON line")
    out = json.loads(line)
    if out.get("n_gpus") != n or out.get("ranks_seen") != n:
        raise SystemExit(f"[bench] asked for {n} ranks, line says n_gpus={out.get('n_gpus')} ranks_seen={out.get('ranks_seen')}")
    print(line, flush=True)
    return out


def timed_region(step_fn, first, K, sync, ldist, dev):
    """EXACTLY K steps bracketed by barrier + device synchronize on both sides; max over ranks.  Returns
    (wall seconds, last step's output)."""
    ldist.barrier()
    sync()
    t0 = time.perf_counter()
    last = None
    for t in range(first, first + K):
        last = step_fn(t)
    sync()
    ldist.barrier()
    wall = time.perf_counter() - t0
    return ldist.max_over_ranks(wall, dev), last


def main(argv=None, engine_factory=None, device=None):
    """engine_factory / device: test hooks (tests/test_dist_rollout.py drives this function on CPU over gloo with a
    stand-in engine so that the N > 1 code path -- shard, step, all-gather, max over ranks -- is executed without GPUs)."""
    args = parse_args(argv)
    cli_stub = engine_factory is None and bool(args.engine_factory)
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            if engine_factory is not None:
                raise SystemExit("bench.main: a callable engine_factory cannot cross into child ranks; pass --engine-factory")
            return launch_ranks(args, sys.argv[1:] if argv is None else argv)
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"[bench] --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}: refusing to run a "
                         "mislabelled job (launch with --nproc-per-node equal to --gpus)")
    if cli_stub:
        engine_factory = _resolve_factory(args.engine_factory)
    from lram_amd import dist as ldist, init_state_dict, preset
    stub = engine_factory is not None
    if not stub:
        _, _, lr = ldist.dist_env()
        if torch.cuda.device_count() <= lr:      # before any rendezvous: a missing GPU must not leave the others waiting
            raise SystemExit(f"bench.py: rank with LOCAL_RANK={lr} has no HIP device ({torch.cuda.device_count()} visible); "
                             "the engine has no CPU fallback")
    if not stub and not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device; the engine has no CPU fallback")
    rank, world, local_rank = ldist.init_distributed("gloo" if stub else None)
    assert world == args.gpus
    if stub:
        dev = torch.device("cpu") if device is None else torch.device(device)
    else:
        from lram_amd import build
        from lram_amd.engine import Engine
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        if rank == 0:
            build.build(force=False, verbose=False)
    ldist.barrier()
    on_gpu = dev.type == "cuda"
    # the N > 1 code path (all-gather per step, collective report) -- also with ONE rank under LRAM_DIST_SINGLE_RANK=1, which is
    # how a one-GPU box puts RCCL through it (tests/test_gpu_dist_single_rank.py)
    dist_on = world > 1 or ldist._single_rank_collectives()

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    gemm_kind = os.environ.get("LRAM_GEMM", "f16x2")
    gemm_kind = gemm_kind if gemm_kind in GEMM_KINDS else "f16x2"
    spec = preset(args.config)
    sd = init_state_dict(spec, seed=0, with_image_encoder=args.obs == "image") if not stub else None
    B, T, K, W = args.batch, spec.tokens_per_step, args.steps, args.warmup
    if args.global_batch > 0:
        lo, hi = ldist.shard_bounds(args.global_batch, rank, world)
        B = hi - lo
    global_batch = args.global_batch if args.global_batch > 0 else B * world
    eng = engine_factory(spec, B, dev) if stub else Engine(spec, sd, B, device=dev)
    if not stub and spec.backbone == "xlstm" and (args.state != "auto" or "LRAM_STATE" not in os.environ):
        try:
            eng.set_state_mode(args.state)
        except Exception:
            if args.state == "lazy":
                raise
    if args.graph:
        eng.set_graph_mode(True)
    eng.set_micro_batches(args.micro)
    state_mode = eng.state_mode
    compat = {"mamba_repeat": 1, "stale_state": False}
    if args.mamba_compat:
        eng.set_compat_mode(args.env_act_dim if args.env_act_dim > 0 else spec.act_dim, True)
        compat = eng.compat_mode

    # ---- synthetic inputs, all resident in HBM before timing (DummyEnv-style) ----------
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    n_ring = 8
    obs_ring = torch.zeros(n_ring, B, spec.state_dim, device=dev)
    from lram_amd.rollout import CHEETAH_RUN_OBS_INDEX
    idx = torch.tensor([i for i in CHEETAH_RUN_OBS_INDEX if i < spec.state_dim], device=dev)
    obs_ring[:, :, idx] = torch.rand(n_ring, B, idx.numel(), generator=g, device=dev) * 2 - 1
    ep_len, rtg0, scale = 1000, 451.274 / 100.0, 100.0  # cheetah-run target / reward_scale
    phase = torch.arange(B, device=dev) % ep_len
    n_prime = 16  # untimed priming steps in lazy state mode (see below); the schedule covers them either way
    steps_total = n_prime + K + W + 16 + args.host_io_steps + 8
    tt = torch.arange(steps_total, device=dev).view(-1, 1)
    age = (phase.view(1, -1) + tt) % ep_len                       # steps since that env's last reset
    masks = (age == 0).to(torch.uint8).contiguous()
    masks[0] = 1                                                  # every env starts an episode
    rtgs = (rtg0 - age.float() * (1.0 / scale)).contiguous()     # env reward 1 per step
    reward_tok = torch.zeros(B, device=dev)                       # reward token is 0 in the reference loop (Q3)
    sync()

    img_ring = None
    if args.obs == "image":
        img_ring = torch.randint(0, 256, (n_ring, B, 3, 64, 64), generator=g, device=dev, dtype=torch.uint8)
        emb = torch.empty(B, spec.d_model, device=dev)

    clock = [0]  # global timestep: the episode schedule (resets, returns-to-go) runs on without repeating step 0
    last_tokens = [None]  # the token ids the latest step wrote beside its actions (--dump-outputs)

    def next_t():
        t = clock[0] if clock[0] < steps_total else 1 + (clock[0] - 1) % (steps_total - 1)
        clock[0] += 1
        return t

    def one_step(_t=None):
        t = next_t()
        if img_ring is not None and TWO_CALL_IMAGES:
            eng.embed_images(img_ring[t % n_ring], emb)
            a, tok = eng.step(emb, rtgs[t], reward_tok, masks[t], discrete=True, obs_is_embedding=True)
        elif img_ring is not None:
            a, tok = eng.step_images(img_ring[t % n_ring], rtgs[t], reward_tok, masks[t], discrete=True)
        else:
            a, tok = eng.step(obs_ring[t % n_ring], rtgs[t], reward_tok, masks[t])
        last_tokens[0] = tok
        if dist_on:
            a = ldist.all_gather_actions(a, args.global_batch if args.global_batch > 0 else None)
        return a

    if args.side_stream and on_gpu:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        torch.cuda.set_stream(side)
    if state_mode == "lazy":
        # Untimed priming, not part of the W warm-up steps: every env starts with an empty matrix memory, and until an
        # env's first fold (at most one fold period, 13 steps) the read pass has nothing to read.  The timed region
        # must see the steady state, whatever W the caller picks.
        for t in range(n_prime):
            one_step(t)
    for t in range(W):
        one_step(t)
    # live kernel timing = HIP events around every state-pass launch: free beside 0.5 ms kernels, 12 % of a launch-bound
    # single-env step (0.422 vs 0.377 ms), so small batches run without it unless asked (--kernel-timing)
    timing = not args.no_kernel_timing and not args.graph and not stub and (B >= 256 or args.kernel_timing)
    # ... and at 21 state-pass launches per step two event packets per launch cost the 4096-slot step 1.3-1.8 % when every step
    # carries them (profiles/r05_ab_kernel_timing.txt): every `--timing-every`-th step of the timed region is timed (default 4:
    # 16 of 64 steps, 336 launches), the rest run as a caller's steps do
    every = max(1, args.timing_every)
    steps_timed = len(range(0, K, every))
    if timing:
        sync()
        eng.profile_begin_sampled(every)
    if not stub:
        eng.gemm_counts(reset=True)
    wall, last = timed_region(one_step, W, K, sync, ldist, dev)
    gemm_ran = None if stub else eng.gemm_counts()
    if timing:
        kern_ms, kern_n, fold_ms, fold_n = eng.profile_end_split()
    else:
        kern_ms, kern_n, fold_ms, fold_n = 0.0, 0, 0.0, 0
    if args.dump_outputs:
        # now, before any later step overwrites the engine's output buffers; the tokens are gathered like the actions
        tokens = last_tokens[0]
        if dist_on and tokens is not None:
            tokens = ldist.all_gather_actions(tokens, args.global_batch if args.global_batch > 0 else None)
        if rank == 0:
            dump_outputs(args.dump_outputs, {"actions": last, "tokens": tokens})
    value = global_batch * K / wall
    ranks_seen = ldist.count_ranks(dev)

    out = {
        "metric": "env-steps/sec (action-inference)", "value": value, "unit": "env-steps/s",
        "n_gpus": world, "ranks_seen": ranks_seen, "steps": K, "warmup": W, "ms_per_step": wall / K * 1e3, "higher_is_better": True,
        "scaling": "strong" if args.global_batch > 0 else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": (f"{args.config}: xLSTM[7:1] 16M rollout, {B} env slots per GPU, 3 tokens/timestep, "
                                "cheetah-run-shaped obs (17 of 204 dims), continuous 8x274 head; fp32 state and "
                                f"accumulation, dense projections {projection_label(gemm_ran, gemm_kind)}"
                                if args.config == "xlstm_16m" and args.obs == "state"
                                else f"{args.config}, {B} env slots per GPU, {args.obs} observations; fp32 state, "
                                     f"projections {projection_label(gemm_ran, gemm_kind)}"),
                   "batch_per_gpu": B, "global_batch": global_batch, "tokens_per_step": T,
                   "state_bytes_per_env": spec.state_bytes_per_env(), "parallelism": f"env-shard x{world}",
                   "graph": bool(args.graph), "micro_batches": args.micro, "state_mode": state_mode,
                   "trajectory_mode": ("reference Mamba agent: %d forwards per env-step, layer-0-only resets"
                                       % compat["mamba_repeat"]) if args.mamba_compat else
                                      "one state advance per env-step, full reset"},
        "inputs": "resident in HBM before the timed region (obs ring, per-step rtg and reset masks)",
    }
    if not stub:   # which library ran: sha256 over its sources + headers + flags, compiled in (lram_amd/build.py)
        from lram_amd import build as _build
        from lram_amd.engine import load_library
        out["build_id"] = load_library().lram_build_id().decode()
        out["build_id_matches_sources"] = out["build_id"] == _build.source_hash()
    if dist_on and args.full:   # (every rank takes part; rank 0 logs it and carries it on the line)
        out["collective"] = ldist.collective_report(torch.zeros(B, last.shape[-1], dtype=last.dtype, device=last.device),
                                                    args.global_batch if args.global_batch > 0 else None)
        if rank == 0:
            log("[bench] collective:", json.dumps(out["collective"]))
    if gemm_ran:
        out["gemm_dispatch_per_step"] = {k: {"launches": v["launches"] / K, "gflop": v["flop"] / K / 1e9}
                                         for k, v in gemm_ran.items() if v["launches"]}
    if stub:
        if cli_stub and rank == 0:
            print(json.dumps(dict(out, last_actions=last.tolist())), flush=True)
        out["last_actions"] = last
        if dist_on:
            torch.distributed.destroy_process_group()
        return out

    # ---- host-inclusive leg: pinned host -> H2D -> step -> D2H -> host sync, every step ------
    if args.full and args.host_io_steps > 0 and img_ring is None:
        n_h = args.host_io_steps
        h_obs = obs_ring.cpu().pin_memory()
        t_base = clock[0]
        h_rtg = rtgs.cpu().pin_memory()
        h_mask = masks.cpu().pin_memory()
        d_obs, d_rtg = torch.empty(B, spec.state_dim, device=dev), torch.empty(B, device=dev)
        d_mask = torch.empty(B, dtype=torch.uint8, device=dev)
        h_act = torch.empty(global_batch, spec.act_dim).pin_memory()   # every rank receives the gathered actions

        def host_step(_t=None):
            t = next_t()
            d_obs.copy_(h_obs[t % n_ring], non_blocking=True)
            d_rtg.copy_(h_rtg[t], non_blocking=True)
            d_mask.copy_(h_mask[t], non_blocking=True)
            a, _ = eng.step(d_obs, d_rtg, reward_tok, d_mask)
            if dist_on:
                a = ldist.all_gather_actions(a, args.global_batch if args.global_batch > 0 else None)
            h_act.copy_(a, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()   # the caller needs the actions before it can step its envs
            return h_act

        for _ in range(4):
            host_step()
        wall_h, _ = timed_region(host_step, 0, n_h, sync, ldist, dev)
        out["host_io"] = {"value": global_batch * n_h / wall_h, "unit": "env-steps/s", "ms_per_step": wall_h / n_h * 1e3,
                          "steps": n_h,
                          "bytes_h2d_per_step": B * (spec.state_dim * 4 + 4 + 1), "bytes_d2h_per_step": B * spec.act_dim * 4,
                          "note": "SURVEY 8d's host-inclusive step: obs / rtg / reset mask in pinned host memory -> H2D -> "
                                  "lram_step -> D2H of the actions -> host synchronisation after every step; measured after "
                                  "the timed region of `value`, same engine and schedule (started at step %d)" % t_base}
        # SURVEY 8d defines the metric host-inclusive; the bench contract defines `value` with inputs resident in HBM (a
        # PCIe-inclusive rate is never `value`).  Both are on the line, side by side, under names that say which is which.
        out["value_host_inclusive"] = out["host_io"]["value"]
        out["value_inputs_in_hbm"] = value

    # ---- roofline of the dominant kernel -----------------------------------------------------------
    n_rec_blocks = (spec.n_blocks - len(spec.slstm_at)) if spec.backbone == "xlstm" else spec.n_blocks
    lazy = state_mode == "lazy"
    if spec.backbone == "xlstm":
        kname = "mlstm_lazy_cell_kernel + its share of mlstm_lazy_fold_kernel" if lazy else "mlstm_cell_kernel"
        per_env = cell_bytes_lazy(spec, T) if lazy else cell_bytes_materialised(spec, T)
        per_env_8d = cell_bytes_materialised(spec, T)
    else:
        # (lane = channel form for env-steps of the d_state-16 / dt_rank-48 geometry from 64 envs, else the 4-lanes-per-channel kernel)
        kname, per_env = "mamba_ssm_lane_kernel | mamba_ssm_kernel (selective state update)", ssm_bytes(spec, T)
        per_env_8d = per_env
    roofline = {"bound": "hbm", "kernel": kname, "achieved": None, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": None, "traffic": None, "traffic_source": None,
                "algorithmic_bytes_per_env_per_launch": per_env}

    def fill(r, main_ms, n_main, aux_ms, n_aux, steps, envs_total):
        """One state pass = one launch of the dominant kernel over `envs_per_launch` env slots (one block); the lazy
        mode's fold launches (own stream, one per block over all slots) are shared out over the state-pass launches."""
        launches_per_step = n_main / steps
        envs_per_launch = envs_total * n_rec_blocks / launches_per_step
        avg_main = main_ms / n_main
        avg = avg_main + (aux_ms / n_main if n_aux else 0.0)
        ab = per_env * envs_per_launch
        r.update(algorithmic_bytes_per_launch=ab, envs_per_launch=envs_per_launch, launches_per_step=launches_per_step,
                 avg_launch_ms=avg, launches_timed=n_main, achieved=ab / (avg * 1e-3) / 1e9)
        r["frac"] = r["achieved"] / HBM_PEAK_GBPS
        if n_aux:
            r["state_pass_avg_ms"] = avg_main
            r["fold_avg_ms"] = aux_ms / n_aux
            r["fold_launches_timed"] = n_aux
        if lazy:
            r["effective_8d_GBps"] = per_env_8d * envs_per_launch / (avg * 1e-3) / 1e9
        return r

    if kern_n > 0:
        fill(roofline, kern_ms, kern_n, fold_ms, fold_n, steps_timed, B)
        roofline["steps_timed"] = steps_timed
        roofline["timing"] = ("HIP events around every launch of the dominant kernel on the stream it runs on, on every %s step "
                              "of the timed region (%d of %d steps)" % ("" if every == 1 else "%d-th" % every, steps_timed, K))
        roofline["kernel_share_of_step"] = (kern_ms + fold_ms) / steps_timed / (wall / K * 1e3)
    if lazy and roofline.get("avg_launch_ms"):
        r2 = cell_bytes_lazy(spec, T, r2_model=True)
        roofline["frac_round2_byte_model"] = r2 * roofline["envs_per_launch"] / (roofline["avg_launch_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS
        roofline["byte_model_note"] = ("round 3 counts the pending window's khat rows the fused read pass loads for the scores "
                                       "(mean %d B per env and launch) and no longer the separate score kernel's 3 KB of score "
                                       "rows; `frac_round2_byte_model` is the same measurement priced with rounds 1-2's bytes"
                                       % int(T * (LAZY_PERIOD - 1) / 2.0 * spec.inner * 4))
    if lazy:
        roofline["note"] = ("lazy matrix memory: `achieved` / `frac` price the bytes the lazy state pass has to move (C_base "
                            "read once, window rows, q / v / h, 1/13 of a fold's read + write of C_base) against the measured "
                            "time of one read pass plus its share of the fold launches; `effective_8d_GBps` prices SURVEY 8d's "
                            "materialised read + write of C against the same time and is not a bandwidth")
    if args.full and timing and spec.backbone == "xlstm" and args.micro != 1:
        # the same kernel with the chip to itself (no overlapping slice): 8 extra, untimed-for-`value` steps
        eng.set_micro_batches(1)
        one_step()
        sync()
        eng.profile_begin()
        for _ in range(8):
            one_step()
        sync()
        roofline["standalone"] = fill({"note": "micro-batch pipeline off: one launch per block over all env slots"},
                                      *eng.profile_end_split(), 8, B)
        eng.set_micro_batches(args.micro)
    # HBM bytes per launch come from a separate rocprofv3 --pmc pass (scripts/pmc_pass.sh -> profiles/): a constant
    # read from a committed file, labelled as such
    for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):
        tag = "" if args.config == "xlstm_16m" else "_" + args.config   # (scripts/parse_pmc.py names the other configs' files)
        pmc_file = os.path.join(ROOT, "profiles", "%s_cell_kernel_hbm_traffic%s%s.json" % (rnd, tag, "_lazy" if lazy else ""))
        if not os.path.exists(pmc_file):
            continue
        try:
            with open(pmc_file) as fh:
                pm = json.load(fh)
            if pm.get("config") == args.config and pm.get("batch") == B and "hbm_bytes_per_env_per_launch" in pm \
                    and roofline.get("envs_per_launch"):
                roofline["traffic"] = pm["hbm_bytes_per_env_per_launch"] * roofline["envs_per_launch"]
                roofline["traffic_source"] = ("%s (separate rocprofv3 --pmc pass of the same command, FETCH_SIZE x2 + "
                                              "WRITE_SIZE per MI355X_MICROARCH.md; not measured in this process)"
                                              % os.path.relpath(pmc_file, ROOT))
                roofline["traffic_over_algorithmic"] = roofline["traffic"] / roofline["algorithmic_bytes_per_launch"]
                if roofline.get("avg_launch_ms"):
                    roofline["traffic_GBps"] = roofline["traffic"] / (roofline["avg_launch_ms"] * 1e-3) / 1e9
                break
        except Exception:
            pass
    out["roofline"] = roofline
    out["_copy_ceiling_pending"] = True
    if spec.backbone == "mamba":
        # C3 is projection-bound (report the matrix cores beside the HBM state term).  Issued MFMA work of one
        # env-step = 2 M N K per projection x the piece products of the split scheme, over the measured step time: a
        # whole-step average (the projections occupy ~58 % of the device time, profiles/r03_kernel_stats_mamba48m_*), so
        # the in-kernel rate is higher; the matrix-pipe busy share of the projection kernels themselves comes from a
        # separate rocprofv3 --pmc pass (SQ_VALU_MFMA_BUSY_CYCLES), a constant read from profiles/.
        # (what ran, from the dispatch counters: dt_proj inside the state-update kernel runs on the vector ALUs and is not
        # counted; each family issues its own number of matrix-core products per fp32 product)
        per_product = {"f16x2": 3, "bf16x3": 6, "f32": 1, "few_row_f32": 1}
        flops = sum(v["flop"] for v in gemm_ran.values()) / K
        issued = sum(v["flop"] * per_product[k] for k, v in gemm_ran.items()) / K
        products = issued / max(flops, 1.0)
        m = {"bound": "mfma", "fp32_equiv_flop_per_step": flops, "mfma_products_per_fp32_product": products,
             "issued_flop_per_step": issued, "issued_PFLOPs_over_step": issued / (wall / K) / 1e15,
             "peak": MFMA_PEAK_PFLOPS, "unit": "PFLOP/s", "frac_over_step": issued / (wall / K) / 1e15 / MFMA_PEAK_PFLOPS,
             "note": "matrix-core work of the projections averaged over the WHOLE env-step (state update, conv, norms "
                     "included in the time); f32 kind: peak is 0.157 PFLOP/s, frac not comparable"}
        for rnd in ("r06", "r05", "r04", "r03"):
            pmc = os.path.join(ROOT, "profiles", "%s_gemm_mfma_busy.json" % rnd)
            if not os.path.exists(pmc):
                continue
            try:
                with open(pmc) as fh:
                    pj = json.load(fh)
                main = max(gemm_ran, key=lambda k: gemm_ran[k]["flop"])
                m["mfma_busy_in_projection_kernels"] = pj.get(main)
                m["mfma_busy_source"] = ("profiles/%s_gemm_mfma_busy.json (separate rocprofv3 --pmc pass over "
                                         "scripts/bench_gemm.py)" % rnd)
                break
            except Exception:
                pass
        out["mfma"] = m

    # STREAM-like ceilings on this box, for context (not the roofline peak)
    if args.full and not args.no_stream_ceilings:
        from lram_amd.engine import stream_copy, stream_read, stream_rmw
        n_copy = 256 * 1024 * 1024
        src = torch.empty(n_copy, device=dev)
        dst = torch.empty(n_copy, device=dev)

        def rate(fn):
            fn()
            sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                fn()
            e1.record()
            sync()
            return 5 * 2 * n_copy * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9

        out["hbm_copy_measured_GBps"] = rate(lambda: stream_copy(dst, src))
        if roofline.get("achieved"):   # the same achieved rate against what a copy kernel moves on THIS box (not the roofline peak)
            roofline["frac_of_measured_copy"] = roofline["achieved"] / out["hbm_copy_measured_GBps"]
        # the same bytes as an in-place read-modify-write with the cell kernel's access pattern (no arithmetic)
        out["hbm_rmw_measured_GBps"] = rate(lambda: stream_rmw(src))
        # half those bytes as a read-only stream with the lazy read pass's access shape (no arithmetic)
        sink = torch.zeros(1024, device=dev)
        out["hbm_read_measured_GBps"] = rate(lambda: stream_read(src, sink)) / 2
        del src, dst
        # the same read over 4 GiB per launch: launches of 1 GiB (~0.15 ms) lose ~10 % to ramp-up, tail and the gaps between them
        # (scripts/read_shape.cpp: 7.0-7.2 TB/s for 1.6-6.4 GB per launch on the boxes that report 6.1-6.4 above)
        try:
            big = torch.empty(4 * n_copy, device=dev)
            n_keep, n_copy = n_copy, 2 * n_copy            # rate() prices 2 x n_copy floats per call
            out["hbm_read_4GiB_launch_GBps"] = rate(lambda: stream_read(big, sink))
            n_copy = n_keep
            del big
        except RuntimeError:
            pass
    out.pop("_copy_ceiling_pending", None)
    out["algorithmic_bytes_per_env_step"] = 2 * spec.state_bytes_per_env() + 4 * spec.state_dim + 4 * spec.act_dim
    out["whole_step_8d_GBps"] = out["algorithmic_bytes_per_env_step"] * value / world / 1e9
    default_workload = (args.config == "xlstm_16m" and args.obs == "state" and args.batch == 4096 and args.global_batch == 0
                        and not args.mamba_compat and not args.graph)
    # (measurement scripts pass --no-cpu-baseline: profiler / counter / A-B runs of the headline must not drag five other engines along)
    if args.full and rank == 0 and world == 1 and not dist_on and default_workload and not args.no_configs \
            and not args.no_cpu_baseline:
        # BASELINE.json's other configurations, each on a fresh engine after the headline's is gone
        eng.close()
        eng = None
        torch.cuda.empty_cache()
        out["configs"] = config_legs(dev)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        if eng is not None:
            eng.close()
        torch.cuda.empty_cache()
        out["cpu_baseline"] = cpu_baseline(spec, sd)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist_on:
        torch.distributed.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
