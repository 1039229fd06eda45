#!/usr/bin/env python3
"""Byte identity of two builds of the library on the recurrent paths: for refactors of the xLSTM kernels that must not move a bit.

A fixed list of small cases (CASES: one per kernel path of xlstm_kernels.hip, mlstm_chunk.hip, mlstm_front.hip, slstm_seq.hip and
mlstm_lazy.hip -- every mlstm_pre_kernel head count, lean and not, the multi-env front end, the token-sequential and the chunkwise
prefill in both cell forms, the four forms of the sLSTM recurrence; the lazy matrix memory's read pass in its three score forms (head
dim 256, head dim 128, scores from the score kernel at head dims 384 / 512 / 640 / 1024), windows of more than 36 pending rows (fold
period 14), period 1, encoder calls of 1 / 2 / 4 tokens up to a window overflow, the group norm in the read pass, parked slots with
the tail fold, an export in the middle of a window) runs once on the PARENT commit's library (csrc/_variants/<--parent>.so,
LRAM_LIB_VARIANT: build the parent commit and copy its liblram_hip.so there) and once on this tree's.  Every case is a fresh child
process under its own time limit; the first child that does not exit cleanly ends the run.  A child prints one sha256 over the
actions and tokens of every step (the hidden rows of an encoder call) and one per exported state tensor of block 0, of the last
block and of the first sLSTM block: C, n, m, conv, the four sLSTM planes.  Env counts are ragged against every kernel's envs per
workgroup (7, 19, 37); slot 2 restarts in the middle of every run.  Geometries: tests/geometry_cases.py, tests/layout_cases.py and
the published presets (the only 4-head geometries with an inner dim beyond 1024 or an sLSTM head dim of 320).

    python scripts/ab_state_digests.py [--parent parent] [--out report.txt]

The GEMM kernels outside the engine's default paths have cases of their own: GEMM_CASES runs a standalone entry (lram_gemm_*,
engine.gemm_f32(kernel=...)) on seeded operands of every shape the parity tests use (tests/test_gpu_parity.py), with bias and as
an accumulating call, one digest per shape and form; the "tiles_*" cases are the engine runs of
test_tile_kernels_carry_few_row_projections_within_the_parity_bars (the few-row kernel off: split-K and its reduce, gated operand,
SiLU columns, batched and table-addressed GEMMs on the tile kernels).  --cases takes shell patterns: --cases 'gemm_*' 'tiles_*' 'chunk3_*'.

The stored-context entries have cases of their own as well: CTX_CASES ("ctx_*") runs Engine.prefill / Engine.score with per-env
lengths after 5 env-steps (no state is empty), every variant on a fresh engine in the case's child: the replace entry with an
all-ones mask and without a mask, the append entry with the mask 1, 0, 1, 0, 1, 0.  Digests per variant: the returned actions
and tokens (every ScoreResult tensor of a score), the state tensors above, and the save_slots record of every slot of length 0.

Prints one line per case and a JSON summary; exit status 1 when a digest differs (or a child failed)."""
import argparse
import fnmatch
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRONT = {"LRAM_FRONT_MULTI": "1", "LRAM_FRONT_MIN_ENVS": "1", "LRAM_FRONT_EPW": "3"}
GEMM, STEP = {"LRAM_SLSTM_SEQ": "0", "LRAM_SLSTM_FUSED_ROWS": "0"}, {"LRAM_SLSTM_FUSED_ROWS": "0"}
# name: (geometry, env slots, run, state mode, environment[, lazy options]); run = ("steps", n) | ("encoder", tokens per call, ...) |
# ("prefill", L, L, ...); lazy options: period = fold period, micro = env slices, live = live slots during the middle third of the
# steps (the others are parked), export_at = step before which block 0's C is exported (digest "mid.C")
CASES = {
    # mlstm_pre_kernel<3, NH>: every head count, eager (q / k / v rows written) and lazy (lean: phase 3 rebuilds q and k from xa --
    # the branch runs where the read pass fuses the scores, head dim 128 / 256, so never in the 4-head kernel beyond one channel
    # group per thread); 4 heads beyond and inside one channel group per thread
    "pre_nh1": ("geo:nh1_dh128", 7, ("steps", 6), "eager", {}),
    "pre_nh2": ("geo:nh2_dh128", 7, ("steps", 6), "eager", {}),
    "pre_nh8": ("geo:nh8_dh128", 19, ("steps", 6), "eager", {}),
    "pre_nh1_lean": ("geo:nh1_dh128", 7, ("steps", 8), "lazy", {}),
    "pre_nh2_lean": ("geo:nh2_dh128", 7, ("steps", 8), "lazy", {}),
    "pre_nh8_lean": ("geo:nh8_dh128", 19, ("steps", 8), "lazy", {}),
    "pre_nh4_wide": ("preset:xlstm_48m", 7, ("steps", 4), "eager", {}),
    "pre_nh4_single": ("preset:xlstm_16m", 19, ("steps", 6), "eager", {}),
    "pre_nh4_single_lean": ("preset:xlstm_16m", 19, ("steps", 8), "lazy", {"LRAM_FRONT_MULTI": "0"}),
    "pre_t4": ("preset:xlstm_16m", 7, ("encoder", 4), "eager", {}),
    # mlstm_front_kernel<3>: 19 envs, 3 per workgroup (the last workgroup holds one)
    "front_epw3": ("preset:xlstm_16m", 19, ("steps", 8), "lazy", FRONT),
    # mlstm_pre_seq_kernel: a 7-timestep context = launches of 12 and 9 tokens
    "prefill_seq_nh4": ("lay:s_last", 7, ("prefill", 7, 7), "eager", {"LRAM_PREFILL_CHUNK": "0"}),
    "prefill_seq_nh2": ("geo:nh2_dh128", 7, ("prefill", 7, 7), "eager", {"LRAM_PREFILL_CHUNK": "0"}),
    # chunkwise prefill, both cell kernels: a full 63-token pass (two token tiles), then 24 tokens (one tile)
    "chunk3_nh4": ("lay:s_last", 7, ("prefill", 21, 8), "eager", {"LRAM_PREFILL_CHUNK": "1"}),
    "chunk3_nh2": ("geo:nh2_dh128", 7, ("prefill", 21, 8), "eager", {"LRAM_PREFILL_CHUNK": "1"}),
    "chunk32_nh4": ("lay:s_last", 7, ("prefill", 21, 8), "eager", {"LRAM_PREFILL_CHUNK": "2"}),
    "chunk32_nh2": ("geo:nh2_dh128", 7, ("prefill", 21, 8), "eager", {"LRAM_PREFILL_CHUNK": "2"}),
    # sLSTM: recurrent GEMM + slstm_pointwise_kernel, slstm_token_kernel, slstm_seq16_kernel, slstm_seq_kernel
    "slstm_gemm_b37": ("preset:xlstm_16m", 37, ("steps", 4), None, GEMM),
    "slstm_gemm_b7": ("preset:xlstm_16m", 7, ("steps", 4), None, GEMM),
    "slstm_token_b7": ("preset:xlstm_16m", 7, ("steps", 4), None, {}),
    "slstm_token_b37": ("preset:xlstm_16m", 37, ("steps", 4), None, {}),
    "slstm_seq16_b37": ("preset:xlstm_16m", 37, ("steps", 4), None, {**STEP, "LRAM_SLSTM_SEQ": "1"}),
    "slstm_seq16_b7": ("preset:xlstm_16m", 7, ("steps", 4), None, {**STEP, "LRAM_SLSTM_SEQ": "1"}),
    "slstm_seq32_b37": ("preset:xlstm_16m", 37, ("steps", 4), None, {**STEP, "LRAM_SLSTM_SEQ": "2"}),
    "slstm_seq32_b7": ("preset:xlstm_16m", 7, ("steps", 4), None, {**STEP, "LRAM_SLSTM_SEQ": "2"}),
    "slstm_seq32_dh320": ("preset:xlstm_206m", 37, ("steps", 3), None, {**STEP, "LRAM_SLSTM_SEQ": "2"}),   # (the instances that spill)
    # mlstm_lazy.hip: fold, score and read-pass kernels.  Scores from the score kernel: LPR = 64 (head dim 512), staging and dot loops
    # beyond 768 columns (1024), LPR = 32 (384); fused scores at 256-wide heads with 8 heads
    "lazy_dh512": ("geo:nh2_dh512", 7, ("steps", 8), "lazy", {}),
    "lazy_dh1024": ("geo:nh1_dh1024", 7, ("steps", 8), "lazy", {}),
    "lazy_dh384": ("preset:xlstm_48m", 7, ("steps", 6), "lazy", {}),
    "lazy_nh8_dh256": ("geo:nh8_dh256", 19, ("steps", 8), "lazy", {}),
    # fold period 14 (the longest lram_set_state_mode accepts): 39 rows pending at the last read pass before an env's fold -- the
    # late-row paths beyond the 36-row prefetch
    "lazy_p14_dh256": ("preset:xlstm_16m", 7, ("steps", 22), "lazy", {}, {"period": 14}),
    "lazy_p14_dh512": ("geo:nh2_dh512", 7, ("steps", 22), "lazy", {}, {"period": 14}),
    "lazy_p14_dh128": ("geo:nh2_dh128", 7, ("steps", 22), "lazy", {}, {"period": 14}),
    "lazy_p1_dh128": ("geo:nh2_dh128", 7, ("steps", 8), "lazy", {}, {"period": 1}),
    # encoder calls in lazy mode: T = 1, 2, 4 instances; twelve 4-token calls fill the window to 44 / 48 rows and overflow it ahead of
    # the fold phase (full grid)
    "lazy_enc_t124": ("preset:xlstm_16m", 7, ("encoder", 1, 2, 4, 2, 1, 4), "lazy", {}),
    "lazy_enc_t124_dh512": ("geo:nh2_dh512", 7, ("encoder", 1, 2, 4, 2, 1, 4), "lazy", {}),
    "lazy_enc_overflow": ("preset:xlstm_16m", 7, ("encoder",) + (4,) * 14, "lazy", {}, {"period": 14}),
    "lazy_enc_overflow_dh512": ("geo:nh2_dh512", 7, ("encoder",) + (4,) * 14, "lazy", {}, {"period": 14}),
    "lazy_gn_fuse": ("preset:xlstm_16m", 19, ("steps", 8), "lazy", {"LRAM_GN_FUSE": "1"}),
    # parked slots (mlstm_lazy_parked_kernel, the parked fold) under two env slices (the tail fold), period 3; an export mid-window
    "lazy_parked": ("preset:xlstm_16m", 19, ("steps", 18), "lazy", {}, {"period": 3, "micro": 2, "live": 11}),
    "lazy_parked_dh512": ("geo:nh2_dh512", 19, ("steps", 18), "lazy", {}, {"period": 3, "micro": 2, "live": 11}),
    "lazy_export_mid": ("preset:xlstm_16m", 7, ("steps", 10), "lazy", {}, {"export_at": 5}),
    # the 36- / 18-row projections on the 128 x 128 tile kernels (few-row kernel off), sLSTM recurrence as batched GEMMs
    **{f"tiles_{kind}_{model[:5]}": (f"preset:{model}", B, ("steps", 4), None,
                                     {"LRAM_GEMM": kind, "LRAM_GEMM_SKINNY_ROWS": "0", **GEMM})
       for kind in ("bf16x3", "f32") for model, B in (("xlstm_16m", 12), ("mamba_48m", 6))},
}
# standalone GEMM entries: name -> (kernel of engine.gemm_f32, shapes (m, n, k)): the parameter lists of tests/test_gpu_parity.py
_TILE = [(128, 128, 32), (96, 2192, 512), (300, 80, 1536), (1000, 1408, 512), (4096, 512, 1024), (1100, 1024, 40), (1030, 650, 40)]
_NARROW = [(3072, 80, 1536), (300, 80, 1536), (257, 33, 256), (1000, 96, 320), (17, 5, 256), (4100, 80, 2560), (64, 16, 576),
           (40, 48, 320), (40, 20, 256), (40, 60, 320)]
GEMM_CASES = {
    "gemm_f32": ("f32", _TILE + [(37, 204, 204), (9, 80, 1536)]),
    "gemm_gemv": ("f32", [(5, 8, 4), (3, 2048, 512), (6, 513, 1024), (8, 80, 1536)]),
    "gemm_bf16x3": ("bf16x3", _TILE + [(5, 8, 8), (257, 129, 48)]),
    "gemm_few_row": ("skinny", [(9, 80, 1536), (96, 2192, 512), (36, 2048, 512), (96, 512, 1024), (192, 2816, 512), (33, 130, 36),
                                (100, 513, 1344), (24, 1280, 2560), (63, 5120, 1280), (17, 32, 32)]),
    "gemm_narrow": ("narrow", _NARROW),
    "gemm_narrow16": ("narrow16", _NARROW),
}
# stored contexts of per-env length: name -> (geometry, env slots, timesteps, lengths (None: the dense entry), "prefill" | "score",
# environment[, options]); options: mode = state mode, micro = env slices.  The smallest shapes that reach each path: the 16M plan
# [0, 9, 17, 28, 38, 46] on the chunkwise kernels over the three lanes, on the token-sequential kernels and one chunk at a time;
# slots of length 0 in both state modes; two env slices; the geometries without a chunkwise form; the sLSTM instances that spill
_LEN16 = [47, 47, 30, 30, 9, 1]
CTX_CASES = {
    "ctx_16m": ("preset:xlstm_16m", 6, 47, _LEN16, "prefill", {}),
    "ctx_16m_seq": ("preset:xlstm_16m", 6, 47, _LEN16, "prefill", {"LRAM_PREFILL_CHUNK": "0"}),
    "ctx_16m_one": ("preset:xlstm_16m", 6, 47, _LEN16, "prefill", {"LRAM_PREFILL_CHUNK": "3"}),
    "ctx_zero": ("preset:xlstm_16m", 4, 12, [0, 12, 0, 5], "prefill", {}, {"mode": "eager"}),
    "ctx_zero_lazy": ("preset:xlstm_16m", 4, 12, [0, 12, 0, 5], "prefill", {}, {"mode": "lazy"}),
    "ctx_micro2": ("preset:xlstm_16m", 6, 13, [13, 13, 8, 8, 3, 1], "prefill", {}, {"micro": 2}),
    "ctx_xlstm_tiny": ("preset:xlstm_tiny", 4, 9, [9, 6, 2, 0], "prefill", {}),
    "ctx_mamba_tiny": ("preset:mamba_tiny", 4, 9, [9, 6, 2, 0], "prefill", {}),
    "ctx_206m": ("preset:xlstm_206m", 3, 6, [6, 3, 0], "prefill", {}),
    "ctx_score_16m": ("preset:xlstm_16m", 6, 47, _LEN16, "score", {}),
    "ctx_score_dense": ("preset:xlstm_16m", 6, 21, None, "score", {}),
}
CTX_PRE, CTX_APPEND_MASK = 5, [1, 0, 1, 0, 1, 0]
RESTART_SLOT = 2


def case_spec(geometry):
    kind, name = geometry.split(":")
    if kind == "preset":
        from lram_amd import preset
        return preset(name)
    if kind == "geo":
        from tests.geometry_cases import case_spec as geo
        return geo(name)
    from tests.layout_cases import case_spec as lay
    return lay(name)


def child_gemm(name):
    import torch
    from lram_amd.engine import gemm_f32
    kernel, shapes = GEMM_CASES[name]
    digests = {}
    for m, n, k in shapes:
        g = torch.Generator().manual_seed(m * 7 + n + k)
        a = (torch.randn(m, k, generator=g) * torch.exp(torch.randn(m, 1, generator=g))).cuda()   # rows of varied scale
        w, bias, base = torch.randn(n, k, generator=g).cuda(), torch.randn(n, generator=g).cuda(), torch.randn(m, n, generator=g).cuda()
        outs = [gemm_f32(a, w, bias, kernel=kernel)]
        if not kernel.startswith("narrow"):   # (the narrow-output kernels take no residual)
            outs.append(gemm_f32(a, w, None, out=base.clone(), accumulate=True, kernel=kernel))
        torch.cuda.synchronize()
        for form, t in zip(("bias", "accumulate"), outs):
            digests[f"{m}x{n}x{k}.{form}"] = hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
    print(json.dumps({"case": name, "digests": digests, "slstm": {}, "mode": kernel}))


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def state_digests(eng, spec, prefix=""):
    """One digest per exported state tensor of block 0, of the last block and of the first sLSTM block (Mamba: conv and SSM state of
    the first and the last block)."""
    digests = {}
    if spec.backbone == "mamba":
        pkv = eng.export_past_key_values()
        for blk in (0, spec.n_blocks - 1):
            for which, what in ((0, "conv"), (1, "ssm")):
                digests[f"{prefix}block{blk}.{what}"] = _sha(pkv[blk][which])
    blocks = [] if spec.backbone == "mamba" else sorted({0, spec.n_blocks - 1} | set(list(spec.slstm_at)[:1]))
    for blk in blocks:
        for which, what in ((0, "planes"), (3, "conv")) if blk in spec.slstm_at else ((0, "C"), (1, "n"), (2, "m"), (3, "conv")):
            digests[f"{prefix}block{blk}.{what}"] = _sha(eng.export_state_tensor(blk, which))
    return digests


def child_ctx(name):
    import torch
    from lram_amd import engine, init_state_dict
    from tests.helpers import make_inputs
    geometry, B, L, lengths, kind, _, *opt = CTX_CASES[name]
    opt = opt[0] if opt else {}
    spec = case_spec(geometry)
    dev = torch.device("cuda", 0)
    sd = init_state_dict(spec, seed=5)
    seq = make_inputs(spec, B, L + CTX_PRE, seed=41, reset_prob=0.0)
    obs, rtg, rew = (torch.stack([x[i] for x in seq[:L]], 1).contiguous() for i in range(3))
    for b, n in enumerate(lengths or []):   # NaN in every padded position
        obs[b, n:], rtg[b, n:], rew[b, n:] = float("nan"), float("nan"), float("nan")
    obs, rtg, rew = obs.to(dev), rtg.to(dev), rew.to(dev)
    target = (torch.rand(B, L, spec.act_dim, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    ones, alternate = torch.ones(B, dtype=torch.uint8, device=dev), torch.tensor(CTX_APPEND_MASK[:B], dtype=torch.uint8, device=dev)
    variants = [("dense", False, None)] if lengths is None else \
        [("replace.ones", False, ones), ("replace.nomask", False, None), ("append", True, alternate)]
    digests, ran = {}, None
    for variant, append, mask in variants:
        eng = engine.Engine(spec, sd, B, device=dev)
        if "mode" in opt:
            eng.set_state_mode(opt["mode"])
        if "micro" in opt:
            eng.set_micro_batches(opt["micro"])
        for t in range(L, L + CTX_PRE):   # no state is empty
            eng.step(*(x.to(dev) for x in seq[t][:3]), None)
        if kind == "score":
            res = eng.score(obs, rtg, rew, actions=target, reset_mask=mask, want=("actions", "tokens", "logp"), logits=True,
                            lengths=lengths, append=append)
            out = {k: getattr(res, k) for k in ("actions", "tokens", "logp", "logits")}
        else:
            out = dict(zip(("actions", "tokens"), eng.prefill(obs, rtg, rew, reset_mask=mask, lengths=lengths, append=append)))
        torch.cuda.synchronize()
        for k, t in out.items():
            digests[f"{variant}.{k}"] = _sha(t)
        digests.update(state_digests(eng, spec, variant + "."))
        for b, n in enumerate(lengths or []):
            if n == 0:
                digests[f"{variant}.record{b}"] = _sha(eng.save_slots([b]))
        ran = eng.state_mode
        eng.close()
    print(json.dumps({"case": name, "digests": digests, "slstm": {}, "mode": ran}))


def child(name):
    if name in GEMM_CASES:
        return child_gemm(name)
    if name in CTX_CASES:
        return child_ctx(name)
    import torch
    from lram_amd import engine, init_state_dict
    from tests.helpers import make_inputs
    geometry, B, run, mode, _, *opt = CASES[name]
    opt = opt[0] if opt else {}
    spec = case_spec(geometry)
    dev = torch.device("cuda", 0)
    eng = engine.Engine(spec, init_state_dict(spec, seed=5), B, device=dev)
    if mode is not None:
        eng.set_state_mode(mode, opt.get("period", 0))
    if "micro" in opt:
        eng.set_micro_batches(opt["micro"])
    h, digests = hashlib.sha256(), {}

    def take(t):
        h.update(t.detach().cpu().contiguous().numpy().tobytes())

    if run[0] == "encoder":
        g = torch.Generator().manual_seed(3)
        calls = run[1:] if len(run) > 2 else run[1:] * 2
        for call, T in enumerate(calls):   # each call reads the state the one before left; slot RESTART_SLOT restarts in the middle one
            mask = torch.zeros(B, dtype=torch.uint8)
            mask[RESTART_SLOT] = call == len(calls) // 2
            take(eng.encoder_step(torch.randn(B, T, spec.d_model, generator=g).to(dev), mask.to(dev)))
    else:
        seq = make_inputs(spec, B, sum(run[1:]), seed=41, reset_prob=0.0)   # (every slot starts at timestep 0)
        seq[len(seq) // 2 if run[0] == "steps" else sum(run[1:-1])][3][RESTART_SLOT] = 1   # prefill: at the last context's start
        if run[0] == "steps":
            for t, (obs, rtg, rew, mask) in enumerate(seq):
                if "live" in opt and t in (len(seq) // 3, 2 * len(seq) // 3):   # parked during the middle third of the steps
                    eng.set_live(opt["live"] if t == len(seq) // 3 else B)
                if t == opt.get("export_at"):   # (in the middle of a window: the export folds)
                    digests["mid.C"] = hashlib.sha256(eng.export_state_tensor(0, 0).cpu().contiguous().numpy().tobytes()).hexdigest()
                n = eng.live
                a, tok = eng.step(obs[:n].to(dev), rtg[:n].to(dev), rew[:n].to(dev), mask[:n].to(dev))
                take(a), take(tok)
        else:
            t0 = 0
            for L in run[1:]:   # one prefill call per context, on the state the one before left
                part = seq[t0:t0 + L]
                obs, rtg, rew = (torch.stack([x[i] for x in part], 1).contiguous().to(dev) for i in range(3))
                a, tok = eng.prefill(obs, rtg, rew, part[0][3].to(dev))
                take(a), take(tok)
                t0 += L
    torch.cuda.synchronize()
    digests["outputs"] = h.hexdigest()
    digests.update(state_digests(eng, spec))
    counts = eng.slstm_counts() if spec.backbone != "mamba" and spec.slstm_at else {}
    if name.startswith("tiles_"):   # which projection families ran (launch counts per family)
        counts = {**counts, **{k: v["launches"] for k, v in eng.gemm_counts().items()}}
    ran = eng.state_mode   # (what lram_get_state_mode reports: a "lazy" run took the lean front end where the head dim is 128 / 256)
    eng.close()
    print(json.dumps({"case": name, "digests": digests, "slstm": counts, "mode": ran}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="parent", help="csrc/_variants/<name>.so: the parent commit's library")
    ap.add_argument("--out", help="write the report here as well")
    ap.add_argument("--timeout", type=int, default=150, help="time limit of one child, seconds")
    ap.add_argument("--case", choices=list(CASES) + list(GEMM_CASES) + list(CTX_CASES), help="(internal) run one case in this process")
    ap.add_argument("--cases", nargs="+", default=["*"], help="shell patterns: the cases to run (default: all)")
    args = ap.parse_args()
    if args.case:
        return child(args.case)
    if not os.path.exists(os.path.join(ROOT, "lram_amd", "csrc", "_variants", args.parent + ".so")):
        sys.exit(f"csrc/_variants/{args.parent}.so is missing: build the parent commit and copy its liblram_hip.so there")
    lines, results = [], {}
    every = {**CASES, **{n: (f"entry:{k}", len(s), ("shapes",), None, {}) for n, (k, s) in GEMM_CASES.items()},
             **{n: (g, B, (kind, L, "full" if ls is None else ",".join(map(str, ls))), None, env, *opt)
                for n, (g, B, L, ls, kind, env, *opt) in CTX_CASES.items()}}
    cases = {n: c for n, c in every.items() if any(fnmatch.fnmatch(n, pat) for pat in args.cases)}

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for lib in (args.parent, None):
        for name, case in cases.items():
            env = {**os.environ, **case[4]}
            env.pop("LRAM_LIB_VARIANT", None)
            if lib:
                env["LRAM_LIB_VARIANT"] = lib
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], capture_output=True, text=True,
                                   timeout=args.timeout, env=env, cwd=ROOT)
                rc, out, err = p.returncode, p.stdout, p.stderr
            except subprocess.TimeoutExpired as e:
                rc, out, err = 124, "", f"time limit of {args.timeout} s: {e}"
            if rc != 0:   # nothing more runs on the device after a child that did not exit cleanly
                say(f"{name} on {lib or 'tree'}: exit status {rc}\n{err[-2000:]}")
                sys.exit(1)
            results[(lib or "tree", name)] = json.loads(out.strip().splitlines()[-1])
            print(f"[{lib or 'tree'}] {name}: done", file=sys.stderr, flush=True)
    differ = []
    for name, (geometry, B, run, mode, env, *opt) in cases.items():
        env = {**env, **(opt[0] if opt else {})}
        a, b = results[(args.parent, name)], results[("tree", name)]
        bad = sorted(k for k in a["digests"] if a["digests"][k] != b["digests"].get(k))
        differ += [f"{name}:{k}" for k in bad]
        forms = " ".join(f"{k}={v}" for k, v in b["slstm"].items() if v)
        say(f"{name:22s} {geometry:18s} B={B:<3d} {' '.join(map(str, run)):14s} {(mode or 'auto') + '>' + b['mode'][:5]:11s} "
            f"{' '.join(f'{k}={v}' for k, v in env.items()) or '-':58s} {len(a['digests'])} digests "
            f"{'EQUAL' if not bad else 'DIFFER: ' + ', '.join(bad)}  outputs {b['digests'].get('outputs', '-')[:12]}  sLSTM launches: {forms or '-'}")
    n = sum(len(results[("tree", c)]["digests"]) for c in cases)
    say(json.dumps({"cases": len(cases), "digests": n, "differ": differ}))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
