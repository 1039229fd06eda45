"""GPU: env isolation and reset recovery with non-finite inputs.

A diverged simulation (DMControl / Meta-World do return NaN, Inf or huge observations) must cost its own env slot alone, and a
reset must give that slot exactly the state of a fresh one (`past_key_values = None`, src/callbacks/evaluation.py:238-251).

Every case drives two engines, one after the other, over the same seeded trajectory.  The poisoned run differs from the clean
one only in a set S of slots over a few steps; both reset S at the same step t0 (through the step's reset mask, Engine.reset
between steps, or prefill's reset_mask).  Asserted per case:

  isolation  every step, every slot outside S: actions and tokens bit-identical; at the end, the taps, lazy_peek (lazy mode)
             and every exported state tensor of every block bit-identical outside S (per-row digests: sum of the int32 bit
             patterns times odd random int64 weights, which any single changed element alters)
  token rule every step, every slot: tokens == torch.argmax (NaN = maximum, first index wins) of the engine's own logits tap,
             actions == inv_tokenize(tokens) exactly; tokens in range
  recovery   from t0 on, every slot, S included, bit-identical to the clean run, final state included (Mamba compat stale mode:
             S keeps the poison, as the reference's InferenceParams.reset() does)
  regime     the state mode, f16x2 launches and env-slice count the case's name claims (tests/test_gpu_published_models.py)

Few-env cases also run the fp32 oracle on the poisoned inputs: actions of a poisoned slot whose oracle logits hold a NaN equal
the oracle's exactly (all-NaN logits: token 0), every other action within assert_actions_match with no ties, and hidden states
from t0 on within 2e-4 or the float64 rule."""
from dataclasses import dataclass

import pytest
import torch

from lram_amd import init_state_dict, preset
from oracle.dt_ref import OraclePolicy, minmax_inv_tokenize
from tests.helpers import Fp64Oracle, assert_actions_match, assert_close_or_as_close_as_fp32_oracle

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
STEPS = 16


def _poison(kind, obs, rtg, rew, rows):
    """Apply one poison to the rows of one step's (device) inputs."""
    if kind == "nan_row":
        obs[rows] = NAN
    elif kind in ("nan", "+inf", "-inf"):
        obs[rows, 5] = {"nan": NAN, "+inf": INF, "-inf": -INF}[kind]
    elif kind == "3e38":
        obs[rows, 1:12:3] = 3e38
        obs[rows, 2] = -3e38
    elif kind == "nan_rtg":
        rtg[rows] = NAN
    elif kind == "inf_rtg":
        rtg[rows] = INF
    elif kind == "inf_reward":
        rew[rows] = INF
    else:
        raise KeyError(kind)


def _nan_argmax(lg):
    """torch.argmax over the last dim with its NaN rule (first NaN, else first index of the maximum), computed without relying
    on a tie order: min over the indices that qualify."""
    n = lg.shape[-1]
    nan = torch.isnan(lg)
    mx = torch.where(nan, torch.full_like(lg, -INF), lg).amax(-1, keepdim=True)
    hit = torch.where(nan.any(-1, keepdim=True), nan, lg == mx)
    ar = torch.arange(n, device=lg.device).expand_as(lg)
    return torch.where(hit, ar, torch.full_like(ar, n)).amin(-1)


_W = {}


def _row_digest(t, rows_dim=0):
    """[rows] int64: sum over each row of the int32 bit patterns times odd random int64 weights (wrapping)."""
    t = t.transpose(0, rows_dim) if rows_dim else t
    t = t.contiguous().view(t.shape[0], -1)
    n = t.shape[1]
    if n not in _W:
        g = torch.Generator(device="cuda").manual_seed(n)
        _W[n] = torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g, device="cuda", dtype=torch.int64) | 1
    out = []
    for r0 in range(0, t.shape[0], 128):
        out.append((t[r0:r0 + 128].view(torch.int32).to(torch.int64) * _W[n]).sum(1))
    return torch.cat(out).cpu()


def _state_digests(eng):
    spec = eng.spec
    out = {}
    for i in range(spec.n_blocks):
        if spec.backbone == "mamba":
            kinds = (0, 3)
        else:
            kinds = (0, 3) if i in spec.slstm_at else (0, 1, 2, 3)
        for w in kinds:
            t = eng.export_state_tensor(i, w)
            out[(i, w)] = _row_digest(t, 1 if (spec.backbone == "xlstm" and i in spec.slstm_at and w == 0) else 0)
            del t
    return out


@dataclass
class Case:
    name: str
    model: str
    slots: int
    S: list                 # the poisoned slots
    plan: list              # (step, slots, poison kind)
    t0: int                 # the step at which S resets
    route: str = "mask"     # "mask": the step's reset mask; "reset": Engine.reset(mask) just before step t0
    mode: str = None        # set_state_mode (None: automatic)
    slices: int = 1         # env slices the automatic choice takes
    f16: bool = False       # f16x2 projections expected
    env: dict = None        # engine knobs read at creation
    graph: bool = False
    compat: tuple = None    # Mamba (mamba_repeat, stale_state)
    discrete: bool = False
    oracle: bool = False
    image: bool = False


def _regime_mib(spec, slots):
    """One mLSTM block's matrix memory over the batch, MiB (the engine's lazy / side-fold / slice thresholds)."""
    return slots * spec.n_heads * spec.head_dim ** 2 * 4 / 2 ** 20


def _inputs(spec, slots, t, g, image):
    if image:
        obs = torch.randint(0, 256, (slots, *spec.image_shape), generator=g, device="cuda", dtype=torch.uint8)
    else:
        obs = torch.zeros(slots, spec.state_dim, device="cuda")
        obs[:, : spec.state_dim * 3 // 4] = torch.rand(slots, spec.state_dim * 3 // 4, generator=g, device="cuda") * 2 - 1
    mask = (torch.rand(slots, generator=g, device="cuda") < 0.03).to(torch.uint8) if t > 0 else \
        torch.ones(slots, dtype=torch.uint8, device="cuda")
    return obs, mask


def _drive(case, spec, sd, poisoned, monkeypatch):
    """One engine over the case's trajectory.  Returns per-step actions / tokens (host), the inputs fed (few-env cases), the
    final taps and state digests, lazy_peek and regime facts."""
    from lram_amd.engine import Engine
    for k, v in (case.env or {}).items():
        monkeypatch.setenv(k, v)
    eng = Engine(spec, sd, case.slots, device="cuda:0")
    for k in (case.env or {}):
        monkeypatch.delenv(k)
    if case.mode is not None:
        eng.set_state_mode(case.mode)
    if case.compat is not None:
        eng.set_compat_mode(*case.compat)
    if poisoned and case.slices > 1:
        eng.set_micro_batches(case.slices)   # the automatic slice count (clean run) == the claimed one (poisoned run), bit for bit
    if case.graph:
        eng.set_graph_mode(True)
    eng.gemm_counts(reset=True)
    B, A = case.slots, spec.act_dim
    S = torch.as_tensor(case.S, device="cuda")
    s_mask = torch.zeros(B, dtype=torch.uint8, device="cuda")
    s_mask[S] = 1
    g = torch.Generator(device="cuda").manual_seed(1000 + B)
    d_obs = torch.zeros(B, *(spec.image_shape if case.image else (spec.state_dim,)), device="cuda",
                        dtype=torch.uint8 if case.image else torch.float32)
    d_rtg, d_rew = torch.full((B,), 4.5, device="cuda"), torch.zeros(B, device="cuda")
    d_mask = torch.ones(B, dtype=torch.uint8, device="cuda")
    rtg = torch.full((B,), 4.5, device="cuda")
    ncol = 1 if case.discrete else A
    out = {"acts": [], "toks": [], "fed": [], "hidden": [], "logits": []}
    for t in range(STEPS):
        obs, mask = _inputs(spec, B, t, g, case.image)
        if t > 0:
            mask[S] = 0                      # S resets at t0 only
        if t == case.t0 and case.route == "mask":
            mask[S] = 1
        d_obs.copy_(obs), d_mask.copy_(mask)
        restart = mask.bool() | ((s_mask > 0) & (t == case.t0))
        rtg = torch.where(restart, torch.full_like(rtg, 4.5), rtg - 0.01)   # the clean return-to-go (a poison lasts one step)
        d_rtg.copy_(rtg)
        d_rew.zero_()
        if poisoned:
            for (tp, rows, kind) in case.plan:
                if tp == t:
                    _poison(kind, d_obs, d_rtg, d_rew, torch.as_tensor(rows, device="cuda"))
        if t == case.t0 and case.route == "reset":
            eng.reset(s_mask)
        if case.oracle:
            fed_mask = d_mask.clone()
            if t == case.t0 and case.route == "reset":
                fed_mask[S] = 1
            out["fed"].append((d_obs.cpu(), d_rtg.cpu(), d_rew.cpu(), fed_mask.cpu()))
        if case.image:
            a, tok = eng.step_images(d_obs, d_rtg, d_rew, d_mask, discrete=case.discrete)
        else:
            a, tok = eng.step(d_obs, d_rtg, d_rew, d_mask, discrete=case.discrete)
        torch.cuda.synchronize()
        _, hidden, logits = eng.taps()
        _check_token_rule(spec, case, a, tok, logits, t)
        out["acts"].append(a[:, :ncol].cpu().clone())
        out["toks"].append(tok[:, :ncol].cpu().clone())
        if case.oracle:
            out["hidden"].append(hidden.cpu())
            out["logits"].append(logits.cpu())
    _, hidden, logits = eng.taps()
    out["taps"] = (_row_digest(hidden), _row_digest(logits))
    out["mode"] = eng.state_mode
    out["gemm"] = eng.gemm_counts()
    if eng.state_mode == "lazy":   # looked at before the exports, which fold
        out["peek"] = {(i, w): eng.lazy_peek(i, w).cpu() for i in range(spec.n_blocks) if i not in spec.slstm_at
                       for w in ("g", "m", "pending")}
    out["state"] = _state_digests(eng)
    eng.close()
    torch.cuda.empty_cache()
    return out


def _check_token_rule(spec, case, a, tok, logits, t):
    B, A = case.slots, spec.act_dim
    lg = logits.view(B, A, spec.n_vocab)
    if case.discrete:
        want = _nan_argmax(lg[:, 0, : spec.n_discrete])
        got = tok[:, 0].long()
        assert torch.equal(got, want), f"{case.name} step {t}: discrete tokens vs argmax of the logits tap"
        assert torch.equal(a[:, 0], want.float()), f"{case.name} step {t}: discrete actions"
        return
    cols = slice(A - 1, A) if (case.compat and case.compat[0] > 1) else slice(0, A)   # repeat mode: the tap is the last forward
    want = _nan_argmax(lg[:, cols])
    got = tok[:, cols].long()
    assert bool(((tok >= 0) & (tok < spec.n_vocab)).all()), f"{case.name} step {t}: token out of range"
    assert torch.equal(got, want), f"{case.name} step {t}: tokens vs argmax of the logits tap"
    inv = minmax_inv_tokenize(tok.long(), spec.action_channels, spec.n_discrete)
    assert torch.equal(a, inv), f"{case.name} step {t}: actions vs inv_tokenize(tokens)"


def _compare(case, spec, clean, bad):
    B = case.slots
    outside = torch.ones(B, dtype=torch.bool)
    outside[torch.as_tensor(case.S)] = False
    stale = bool(case.compat and case.compat[1])
    for t in range(STEPS):
        rows = outside if (t < case.t0 or stale) else torch.ones(B, dtype=torch.bool)
        for k in ("acts", "toks"):
            x, y = clean[k][t][rows], bad[k][t][rows]
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{case.name} step {t}: {k} differ in clean slots" \
                + ("" if t < case.t0 else " (or after the reset)")
    rows = outside if stale else torch.ones(B, dtype=torch.bool)
    what = "outside S" if stale else "after the reset"
    for i, (x, y) in enumerate(zip(clean["taps"], bad["taps"])):
        assert torch.equal(x[rows], y[rows]), f"{case.name}: tap {('hidden', 'logits')[i]} {what}"
    for k in clean["state"]:
        assert torch.equal(clean["state"][k][rows], bad["state"][k][rows]), f"{case.name}: state {k} {what}"
    if "peek" in clean:
        for k in clean["peek"]:
            x, y = clean["peek"][k], bad["peek"][k]
            assert torch.equal(x[rows].view(torch.int32), y[rows].view(torch.int32)), f"{case.name}: lazy_peek {k} {what}"
    if stale:   # the reference keeps layers >= 1's cache over a reset: the poison stays in S
        assert any(not torch.equal(clean["state"][k][~outside], bad["state"][k][~outside]) for k in clean["state"] if k[0] >= 1)


def _check_oracle(case, spec, sd, run):
    kw = {}
    if case.compat is not None:
        kw = dict(mamba_repeat=case.compat[0], stale_state=case.compat[1])
    o32, o64 = OraclePolicy(spec, sd, **kw), Fp64Oracle(spec, sd, **kw)
    in_s = torch.isin(torch.arange(case.slots), torch.as_tensor(case.S))
    stale = bool(case.compat and case.compat[1])
    ties = 0
    for t, (obs, rtg, rew, mask) in enumerate(run["fed"]):
        a_ref, d = o32.step(obs, rtg, rew, mask, discrete=case.discrete, return_debug=True)
        _, d64 = o64.step(obs, rtg, rew, mask, discrete=case.discrete, return_debug=True)
        a = run["acts"][t]
        lg = d["logits"]
        nan = torch.isnan(lg[:, :1, : spec.n_discrete] if case.discrete else lg).any(-1)
        exact = nan & in_s.view(-1, 1)   # a NaN in the oracle's logits of a poisoned slot: the NaN rule decides, bit for bit
        assert torch.equal(a[exact], a_ref.float()[exact]), f"{case.name} step {t}: poisoned actions vs the oracle"
        ties += assert_actions_match(torch.where(exact, a_ref.float(), a), a_ref, lg, spec, discrete=case.discrete,
                                     what=f"{case.name} step {t}")
        rows = ~in_s if (t < case.t0 or stale) else torch.ones(case.slots, dtype=torch.bool)
        assert_close_or_as_close_as_fp32_oracle(run["hidden"][t][rows], d["hidden"][rows], d64["hidden"][rows],
                                                what=f"{case.name} step {t}: hidden")
    assert ties == 0, f"{case.name}: {ties} action ties"


X = "xlstm_16m"
CASES = [
    # xLSTM-16M, few envs, lazy: slot 3 folds at step 10 (window with the poison of step 2) before its reset at 12; slot 0's
    # fold would be due at 13 -- it is reset at 12 with the poison still in its window
    Case("x16_few_lazy", X, 4, [0, 3], [(2, [0], "nan"), (2, [3], "nan_row"), (3, [0], "-inf")], t0=12, mode="lazy",
         oracle=True),
    Case("x16_few_materialised_engine_reset", X, 4, [0, 3], [(2, [0], "+inf"), (3, [3], "3e38"), (4, [3], "inf_reward")],
         t0=7, route="reset", mode="eager", oracle=True),
    Case("x16_few_materialised_discrete", X, 4, [1], [(2, [1], "nan_row")], t0=6, mode="eager", oracle=True, discrete=True),
    Case("x16_graph", X, 8, [0, 7], [(2, [0], "nan_row"), (3, [7], "nan_rtg")], t0=6, graph=True),
    # f16x2 projections, materialised (48M: proj_up from 32 rows); head dim 384
    Case("x48_f16x2_materialised", "xlstm_48m", 32, [0, 15, 16, 31], [(2, [0, 31], "nan_row"), (3, [15, 16], "3e38")],
         t0=6, mode="eager", f16=True),
    Case("x48_few_lazy_separate_score_kernel", "xlstm_48m", 4, [0, 2], [(2, [0], "nan"), (2, [2], "+inf")], t0=6,
         mode="lazy", oracle=True),
    Case("x110_few_lazy_separate_score_kernel", "xlstm_110m", 4, [1, 3], [(2, [1], "nan_row"), (3, [3], "3e38")], t0=6,
         mode="lazy", route="reset", oracle=True),
    # lazy, one slice, side-stream folds (256 .. 512 MiB); slot 1 shares every multi-row workgroup with clean neighbours
    Case("x16_lazy_one_slice_side_stream_folds", X, 256, [0, 1, 130, 255],
         [(2, [0], "nan_row"), (2, [1], "nan_rtg"), (3, [130], "inf_reward"), (4, [255], "-inf")], t0=9),
    # lazy, two slices (2051 slots: 1026 + 1025, ragged GEMM tiles), multi-env front end (4 envs per workgroup at these slices),
    # fused group norm, the f16x2 sLSTM step kernel; slot 5 shares its front-end workgroup with clean slots
    Case("x16_lazy_two_slices_front_end", X, 2051, [0, 5, 1025, 1026, 2050],
         [(2, [0, 1026], "nan_row"), (2, [5], "3e38"), (3, [1025], "+inf"), (3, [2050], "nan_rtg")], t0=8, route="reset",
         slices=2),
    # the sLSTM step kernel's fp32 form and the per-token path, forced at a small slice
    Case("x16_slstm_seq_fp32", X, 64, [0, 63], [(2, [0], "nan_row"), (3, [63], "+inf")], t0=6, mode="eager",
         env={"LRAM_SLSTM_FUSED_ROWS": "0", "LRAM_SLSTM_SEQ": "2"}),
    Case("x16_slstm_per_token", X, 64, [0, 63], [(2, [0], "nan_row"), (3, [63], "+inf")], t0=6, mode="eager",
         env={"LRAM_SLSTM_FUSED_ROWS": "0", "LRAM_SLSTM_SEQ": "0"}),
    Case("x16_images_nan_inf_rtg", X, 6, [0, 5], [(2, [0], "nan_rtg"), (3, [5], "inf_rtg")], t0=6, mode="eager",
         image=True, oracle=True),
    # Mamba-48M: few envs; 2048 slots = two slices, the 8-phase in_proj, the narrow x_proj (16-row blocks: slot 17 among clean
    # ones), the dt_rank-48 lane kernel (slot 2 shares its state-update workgroup with clean slots)
    Case("m48_few", "mamba_48m", 6, [0, 4], [(2, [0], "nan_row"), (3, [4], "3e38"), (3, [0], "inf_reward")], t0=7,
         oracle=True),
    Case("m48_two_slices", "mamba_48m", 2048, [0, 2, 17, 1023, 1024, 2047],
         [(2, [0, 1024], "nan_row"), (2, [2], "nan"), (3, [17], "3e38"), (3, [1023], "-inf"), (4, [2047], "nan_rtg")],
         t0=8, route="reset", slices=2),
    Case("m16_generic_state_update", "mamba_16m", 130, [0, 1, 129], [(2, [0], "nan_row"), (3, [1], "+inf"),
                                                                     (3, [129], "3e38")], t0=6),
    Case("m16_compat_repeat", "mamba_16m", 6, [2], [(2, [2], "nan_row")], t0=5, compat=(8, False), oracle=True),
    Case("m16_compat_stale", "mamba_16m", 6, [2, 5], [(2, [2], "nan_row"), (3, [5], "nan")], t0=5, compat=(1, True),
         oracle=True),
]


def _check_regime(case, spec, run):
    if spec.backbone == "xlstm":
        mib = _regime_mib(spec, case.slots)
        want_mode = {"lazy": "lazy", "eager": "materialised"}.get(case.mode, "lazy" if mib >= 128 and not case.graph
                                                                  else "materialised")
        assert run["mode"] == want_mode, f"{case.name}: state mode {run['mode']}"
        assert (mib >= 512) == (case.slices == 2), f"{case.name}: {mib:.0f} MiB per block is not {case.slices} slice(s)"
        if case.name == "x16_lazy_one_slice_side_stream_folds":
            assert 256 <= mib < 512
    else:
        assert (case.slots >= 1024) == (case.slices == 2), case.name
        if case.name.startswith("m48"):
            assert spec.dt_rank == 48
        else:
            assert spec.dt_rank != 48
    if case.f16:
        assert run["gemm"]["f16x2"]["launches"] > 0, f"{case.name}: no f16x2 projection"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_poisoned_slots_stay_isolated_and_recover(hip_lib, monkeypatch, case):
    spec = preset(case.model)
    sd = init_state_dict(spec, seed=0, with_image_encoder=case.image)
    clean = _drive(case, spec, sd, False, monkeypatch)
    bad = _drive(case, spec, sd, True, monkeypatch)
    _check_regime(case, spec, clean)
    assert bad["mode"] == clean["mode"]
    _compare(case, spec, clean, bad)
    if case.oracle:
        _check_oracle(case, spec, sd, bad)


# ---- stored contexts: prefill ----------------------------------------------------------------------------------------------
L1, L2, DECODE, B_CTX, S_CTX = 43, 41, 4, 16, [0, 7, 15]


def _prefill_run(spec, sd, chunk_env, poisoned, monkeypatch):
    """16 envs: a 43-timestep context (three chunks of 15 / 15 / 13 in flight, the poison in the middle one), then S restarts
    through prefill's reset_mask into a 41-timestep lazy context (a one-timestep last chunk), then lazy decode steps."""
    from lram_amd.engine import Engine
    if chunk_env is not None:
        monkeypatch.setenv("LRAM_PREFILL_CHUNK", chunk_env)
    eng = Engine(spec, sd, B_CTX, device="cuda:0")
    if chunk_env is not None:
        monkeypatch.delenv("LRAM_PREFILL_CHUNK")
    eng.set_state_mode("lazy")
    g = torch.Generator(device="cuda").manual_seed(5)
    seqs = []
    for L in (L1, L2, DECODE):
        obs = torch.rand(B_CTX, L, spec.state_dim, generator=g, device="cuda") * 2 - 1
        rtg = 4.5 - 0.01 * torch.arange(L, device="cuda", dtype=torch.float32).expand(B_CTX, L).contiguous()
        seqs.append([obs, rtg, torch.zeros(B_CTX, L, device="cuda")])
    if poisoned:
        obs, rtg, rew = seqs[0]
        obs[0, 17] = NAN
        obs[7, 20, 3] = INF
        rtg[15, 18] = NAN
        rew[7, 16] = INF
    case = Case("prefill", "xlstm_16m", B_CTX, S_CTX, [], 0)
    ones = torch.ones(B_CTX, dtype=torch.uint8, device="cuda")
    s_mask = torch.zeros(B_CTX, dtype=torch.uint8, device="cuda")
    s_mask[torch.as_tensor(S_CTX, device="cuda")] = 1
    out = {"acts": [], "toks": []}
    for k, (L, mask) in enumerate(((L1, ones), (L2, s_mask))):
        a, tok = eng.prefill(*seqs[k], reset_mask=mask)
        torch.cuda.synchronize()
        _, _, logits = eng.taps()
        _check_token_rule(spec, case, a, tok, logits, f"prefill {k}")
        out["acts"].append(a.cpu().clone()), out["toks"].append(tok.cpu().clone())
    for t in range(DECODE):
        a, tok = eng.step(*(x[:, t].contiguous() for x in seqs[2]), None)
        torch.cuda.synchronize()
        _, _, logits = eng.taps()
        _check_token_rule(spec, case, a, tok, logits, f"decode {t}")
        out["acts"].append(a.cpu().clone()), out["toks"].append(tok.cpu().clone())
    out["mode"] = eng.state_mode
    out["peek"] = {(i, w): eng.lazy_peek(i, w).cpu() for i in range(spec.n_blocks) if i not in spec.slstm_at
                   for w in ("g", "m", "pending")}
    out["state"] = _state_digests(eng)
    eng.close()
    return out


@pytest.mark.parametrize("chunk_env", [None, "0"], ids=["chunk_lanes", "token_sequential"])
def test_prefill_poison_in_a_middle_chunk_then_reset_through_prefill(hip_lib, monkeypatch, chunk_env):
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=0)
    clean = _prefill_run(spec, sd, chunk_env, False, monkeypatch)
    bad = _prefill_run(spec, sd, chunk_env, True, monkeypatch)
    assert clean["mode"] == bad["mode"] == "lazy"
    outside = torch.ones(B_CTX, dtype=torch.bool)
    outside[torch.as_tensor(S_CTX)] = False
    for k in range(len(clean["acts"])):
        rows = outside if k == 0 else torch.ones(B_CTX, dtype=torch.bool)
        for key in ("acts", "toks"):
            assert torch.equal(clean[key][k][rows].view(torch.int32), bad[key][k][rows].view(torch.int32)), (key, k)
    assert not torch.equal(clean["acts"][0][~outside], bad["acts"][0][~outside])   # the poison reached the actions
    for key in clean["peek"]:
        assert torch.equal(clean["peek"][key].view(torch.int32), bad["peek"][key].view(torch.int32)), key
    for key in clean["state"]:
        assert torch.equal(clean["state"][key], bad["state"][key]), key


# ---- the argmax rule from the head weights --------------------------------------------------------------------------------
def _poisoned_bias(spec, sd, discrete):
    """action_net.0.bias with NaN at two positions p < q of one action dim, a NaN at index n_discrete, +Inf at two positions
    and -Inf everywhere but one: tokens {dim: expected token}."""
    V, nd = spec.n_vocab, spec.n_discrete
    b = sd["action_net.0.bias"].clone().view(spec.act_dim, V)
    if discrete:
        b[0, 5], b[0, 12], b[0, nd] = NAN, NAN, NAN
        want = {0: 5}
    else:
        b[0, nd], b[0, 200] = NAN, NAN
        b[1, 7], b[1, 150] = NAN, NAN
        b[2, 30], b[2, 60] = INF, INF
        b[3, :] = -INF
        b[3, 123] = 0.0
        want = {0: nd, 1: 7, 2: 30, 3: 123}
    return {**sd, "action_net.0.bias": b.view(-1).contiguous()}, want


ARGMAX_CASES = [("xlstm_16m", 4, False, False), ("xlstm_16m", 4, False, True), ("xlstm_16m", 4, True, False),
                ("xlstm_16m", 4, True, True), ("mamba_48m", 6, False, True), ("mamba_48m", 2048, False, False),
                ("xlstm_16m", 2051, False, True)]


@pytest.mark.parametrize("model,slots,graph,discrete", ARGMAX_CASES,
                         ids=[f"{m}-{b}-{'graph' if g else 'eager'}-{'discrete' if d else 'continuous'}"
                              for m, b, g, d in ARGMAX_CASES])
def test_action_argmax_follows_torch_nan_rule_from_the_head_weights(hip_lib, model, slots, graph, discrete):
    from lram_amd.engine import Engine
    spec = preset(model)
    sd, want = _poisoned_bias(spec, init_state_dict(spec, seed=0), discrete)
    eng = Engine(spec, sd, slots, device="cuda:0")
    if graph:
        eng.set_graph_mode(True)
    case = Case("argmax", model, slots, [], [], 0, graph=graph, discrete=discrete)
    ora = OraclePolicy(spec, sd) if slots <= 8 else None
    g = torch.Generator(device="cuda").manual_seed(9)
    d_obs, d_rtg = torch.zeros(slots, spec.state_dim, device="cuda"), torch.full((slots,), 4.5, device="cuda")
    d_rew, d_mask = torch.zeros(slots, device="cuda"), torch.ones(slots, dtype=torch.uint8, device="cuda")
    ties = 0
    for t in range(4):
        obs, mask = _inputs(spec, slots, t, g, False)
        d_obs.copy_(obs), d_mask.copy_(mask)
        d_rtg.sub_(0.01)
        a, tok = eng.step(d_obs, d_rtg, d_rew, d_mask, discrete=discrete)
        torch.cuda.synchronize()
        _, _, logits = eng.taps()
        _check_token_rule(spec, case, a, tok, logits, t)
        for j, w in want.items():
            assert bool((tok[:, j] == w).all()), f"{model} {slots} step {t}: action dim {j} tokens {tok[:, j].unique().tolist()}"
        if ora is not None:
            a_ref, d = ora.step(d_obs.cpu(), d_rtg.cpu(), d_rew.cpu(), d_mask.cpu(), discrete=discrete, return_debug=True)
            cols = list(want)
            assert torch.equal(a[:, cols].cpu(), a_ref[:, cols].float()), f"step {t}: NaN-rule actions vs the oracle"
            keep = [j for j in range(a_ref.shape[1]) if j not in want]
            if keep:
                ties += assert_actions_match(a[:, keep], a_ref[:, keep], d["logits"][:, keep], spec, what=f"step {t}")
    assert ties == 0
    eng.close()
