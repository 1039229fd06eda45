"""GPU: what bench.py times, held to the oracle call for call.

bench.main and bench.config_legs run exactly as `bench.py --full` runs them (a plain run makes the same steps up to the end
of its timed region), with every engine they build under the recorder of tests/bench_replay.py; each engine's record is then
replayed through the CPU oracle on a sample of rows (rows 0 and B - 1, both ends of every env slice, rows the bench's reset
schedule restarts inside the run, a row that never restarts):

  headline    16M x 4096 with the lazy priming steps, the sampled state-pass events, the standalone sub-leg (one env slice in
              the middle of the run) and the host-inclusive leg; the --dump-outputs arrays are the recorder's last timed step,
  options     --graph, --side-stream, --micro 2 (an odd batch: uneven slices), --state eager, --obs image, Mamba-48M and its
              reference trajectory (--mamba-compat --env-act-dim 4),
  configs     C2, C3, C3-reference-trajectory and C4 (206M image frames through lram_step_images) replayed; C5's timed prefill
              and 16 + 2 decode steps against a fresh engine stepping the same inputs one lram_step at a time (that path is
              held to the oracle at this geometry by test_gpu_configs.py), and the LRAM_PREFILL_CHUNK=3 engine's prefill bit for
              bit equal to the chunk lanes'.

Every engine replays with 0 action ties on the bench's fixed seeds.  LRAM_TEST_REPORT=1 prints calls, ties and float64-rule
rows per engine."""
import os

import numpy as np
import pytest
import torch

from tests.bench_replay import Session, bench_rows, recording_engine, replay
from tests.helpers import assert_actions_match, rel_err

pytestmark = pytest.mark.gpu

# --full: the host-inclusive leg and the standalone sub-leg run after the timed steps and are replayed with them
COMMON = ["--gpus", "1", "--full", "--no-cpu-baseline", "--no-stream-ceilings", "--no-configs"]


def _report(line):
    if os.environ.get("LRAM_TEST_REPORT"):
        print("[report] " + line)


def _resets_inside(rec):
    """Sampled rows whose reset mask is set on some step after the first."""
    steps = [c for c in rec.calls if c["kind"] in ("step", "step_images")]
    hit = torch.zeros(len(rec.rows), dtype=torch.bool)
    for c in steps[1:]:
        if c["args"]["mask"] is not None:
            hit |= c["args"]["mask"].cpu().bool()
    return [r for r, h in zip(rec.rows, hit.tolist()) if h]


def _run(monkeypatch, argv, rows_for):
    import bench
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LRAM_DIST_SINGLE_RANK"):
        monkeypatch.delenv(k, raising=False)
    session = Session(rows_for)
    monkeypatch.setattr("lram_amd.engine.Engine", recording_engine(session))
    out = bench.main(COMMON + argv)
    session.close_all()
    torch.cuda.empty_cache()
    assert len(session.records) == 1, [r.label for r in session.records]
    return out, session.records[0]


def _replay(rec, name):
    res = replay(rec, report=lambda line: _report(f"{name}: {line}"))
    assert res["ties"] == 0, f"{name}: {res['ties']} action ties"
    return res


def test_headline_run_matches_the_oracle(hip_lib, monkeypatch, tmp_path):
    W, K, H = 2, 8, 8
    argv = ["--config", "xlstm_16m", "--batch", "4096", "--steps", str(K), "--warmup", str(W), "--host-io-steps", str(H),
            "--dump-outputs", str(tmp_path)]
    out, rec = _run(monkeypatch, argv, lambda spec, b: bench_rows(spec, b, 1000, 16 + W + K + 9 + 4 + H))
    lazy = out["config"]["state_mode"] == "lazy"
    assert lazy and out["roofline"].get("launches_timed", 0) > 0 and "standalone" in out["roofline"], out["roofline"]
    kinds = [c["kind"] for c in rec.calls]
    n_steps = 16 + W + K + 9 + 4 + H     # priming, warm-up, timed, the standalone sub-leg (1 + 8), host-inclusive (4 + H)
    assert kinds.count("step") == n_steps, kinds
    micro = [c["args"]["n"] for c in rec.calls if c["kind"] == "set_micro_batches"]
    assert micro == [0, 1, 0], micro
    assert len(_resets_inside(rec)) >= 2, rec.rows
    # --dump-outputs holds the last timed step (call number 16 + W + K among the steps)
    last = [c for c in rec.calls if c["kind"] == "step"][16 + W + K - 1]["out"]
    dumped = {n: np.load(str(tmp_path / (n + ".npy"))) for n in ("actions", "tokens")}
    rows = np.asarray(rec.rows)
    assert np.array_equal(dumped["actions"][rows], last["actions"].cpu().numpy())
    assert np.array_equal(dumped["tokens"][rows], last["tokens"].cpu().numpy().astype(np.float64))
    assert rec.calls[-1]["kind"] == "set_micro_batches"   # (the standalone sub-leg's last call: the tap is still compared)
    assert _replay(rec, "headline xlstm_16m x 4096")["relaxed"] is not None


# (name, bench arguments, preset): batches of 1000 slots and more, so that the bench's schedule restarts sampled rows inside the run
OPTIONS = [
    ("graph", ["--graph", "--batch", "1000"], "xlstm_16m"),
    ("side_stream", ["--side-stream", "--batch", "1024"], "xlstm_16m"),
    ("micro_2", ["--micro", "2", "--batch", "1001"], "xlstm_16m"),
    ("state_eager", ["--state", "eager", "--batch", "1024"], "xlstm_16m"),
    ("obs_image", ["--obs", "image", "--batch", "1024"], "xlstm_16m"),
    ("mamba_48m", ["--batch", "1024"], "mamba_48m"),
    ("mamba_48m_compat", ["--mamba-compat", "--env-act-dim", "4", "--batch", "1024"], "mamba_48m"),
]


@pytest.mark.parametrize("name,argv,config", OPTIONS, ids=[o[0] for o in OPTIONS])
def test_optional_path_matches_the_oracle(hip_lib, monkeypatch, name, argv, config):
    graph = "--graph" in argv
    micro = (int(argv[argv.index("--micro") + 1]) if "--micro" in argv else 0, 1)
    window = 12 if config.startswith("mamba") else 20
    argv = ["--config", config, "--steps", "4", "--warmup", "2", "--host-io-steps", "4"] + argv
    out, rec = _run(monkeypatch, argv, lambda spec, b: bench_rows(spec, b, 1000, window, micro=micro, graph=graph))
    assert out["config"]["graph"] == graph
    if name == "state_eager":
        assert out["config"]["state_mode"] == "materialised"
    if name == "obs_image":
        assert {c["kind"] for c in rec.calls} >= {"step_images"} and rec.image
    if name == "mamba_48m_compat":
        assert [c["args"] for c in rec.calls if c["kind"] == "set_compat_mode"] == [{"mamba_repeat": 4, "stale_state": True}]
    assert len(_resets_inside(rec)) >= 2, rec.rows
    assert _replay(rec, f"{name} {config}")["relaxed"] is not None, f"{name}: no hidden tap compared"


# ---- the config legs ------------------------------------------------------------------------------------------------------
# leg -> (preset, env slots, episode length, steps the engine makes, rows that restart inside them) as bench.config_legs runs it:
# step_leg makes 16 lazy priming steps (2 otherwise) + W + K; C5's engines keep every row (its decode comparison re-steps the
# whole batch).  An engine whose geometry is not in this table fails its leg; the records map to the legs in construction
# order, and each one's geometry is checked against its leg's.
LEG_GEOMETRY = {
    "C2": ("xlstm_16m", 1024, 1000, 16 + 4 + 48, True),
    "C3": ("mamba_48m", 2048, 200, 2 + 4 + 32, True),
    "C3-reference-trajectory": ("mamba_48m", 2048, 200, 2 + 2 + 12, True),
    "C4-per-gpu-shard": ("xlstm_206m", 512, 1000, 16 + 2 + 12, False),   # phases < 512: none restarts within 30 steps of 1000
    "C5": ("xlstm_206m", 64, None, None, False),
    "C5 LRAM_PREFILL_CHUNK=3": ("xlstm_206m", 64, None, None, False),
}
LEGS = list(LEG_GEOMETRY)


def _leg_rows(spec, b):
    from lram_amd import preset
    geo = [g for g in LEG_GEOMETRY.values() if preset(g[0]) == spec and g[1] == b]
    assert geo, f"no config leg of {spec.backbone} d_model {spec.d_model} x {b} envs in LEG_GEOMETRY"
    ep_len = geo[0][2]
    if ep_len is None:
        return list(range(b))
    window = min(g[3] for g in geo)   # (C3 and its reference trajectory share a geometry: the shorter run's window)
    return bench_rows(spec, b, ep_len, window, micro=(0,))


@pytest.fixture(scope="module")
def config_run(hip_lib):
    import bench
    session = Session(_leg_rows)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr("lram_amd.engine.Engine", recording_engine(session))
        legs = bench.config_legs("cuda:0")
        session.close_all()
    torch.cuda.empty_cache()
    return legs, dict(zip(LEGS, session.records)), len(session.records)


def test_config_legs_ran_clean(config_run):
    from lram_amd import preset
    legs, recs, n = config_run
    assert [l.get("id") for l in legs] == LEGS[:5]
    for l in legs:
        assert "error" not in l, l
    assert n == len(LEGS)
    for leg, rec in recs.items():
        assert (preset(LEG_GEOMETRY[leg][0]), LEG_GEOMETRY[leg][1]) == (rec.spec, rec.batch), leg


@pytest.mark.parametrize("leg", LEGS[:4])
def test_config_leg_matches_the_oracle(config_run, leg):
    _, recs, _ = config_run
    rec = recs[leg]
    _, _, ep_len, n_steps, restarts = LEG_GEOMETRY[leg]
    kinds = [c["kind"] for c in rec.calls]
    assert ("step_images" in kinds) == leg.startswith("C4"), kinds
    assert kinds.count("step_images" if leg.startswith("C4") else "step") == n_steps, kinds
    if restarts:
        assert len(_resets_inside(rec)) >= 2, rec.rows
    else:   # the schedule restarts no env slot inside the run (phase = slot % ep_len)
        assert rec.batch <= ep_len - n_steps and _resets_inside(rec) == [], rec.rows
    res = _replay(rec, leg)
    assert res["relaxed"] is not None, f"{leg}: no hidden tap compared"


def test_c5_prefill_and_decode_match_the_step_path(config_run):
    from lram_amd import init_state_dict
    from lram_amd.engine import Engine
    _, recs, _ = config_run
    rec, solo = recs["C5"], recs["C5 LRAM_PREFILL_CHUNK=3"]
    spec, B = rec.spec, rec.batch
    kinds = [c["kind"] for c in rec.calls]
    assert kinds == ["prefill", "prefill"] + ["step"] * 18 + ["prefill"], kinds
    assert [c["kind"] for c in solo.calls] == ["prefill", "prefill"]
    pre = rec.calls[1]
    for other in (rec.calls[0], rec.calls[-1], *solo.calls):   # every prefill of the leg saw the same inputs
        for k in ("obs", "rtg", "reward", "mask"):
            assert torch.equal(other["args"][k], pre["args"][k]), k
    # the chunk lanes vs one chunk at a time: bit for bit (actions, token ids, final state after a prefill of the same inputs)
    for c in solo.calls:
        assert torch.equal(c["out"]["actions"], pre["out"]["actions"]) and torch.equal(c["out"]["tokens"], pre["out"]["tokens"])
    for k in rec.final_state:
        assert torch.equal(solo.final_state[k], rec.final_state[k]), f"C5 lanes vs LRAM_PREFILL_CHUNK=3: state {k}"
    # the same inputs one lram_step at a time on a fresh engine
    sd = init_state_dict(spec, seed=0)
    eng = Engine(spec, sd, B, device="cuda:0")
    obs, rtg, rew, ones = (pre["args"][k] for k in ("obs", "rtg", "reward", "mask"))
    ties = 0

    def check(got, a_step, what):   # the step path's own logits decide what is a rounding-level tie
        torch.cuda.synchronize()
        logits = eng.taps()[2].view(B, spec.act_dim, spec.n_vocab).cpu()
        return assert_actions_match(got, a_step.cpu(), logits, spec, what=what)

    for t in range(obs.shape[1]):
        a_s, _ = eng.step(obs[:, t].contiguous(), rtg[:, t].contiguous(), rew[:, t].contiguous(), ones if t == 0 else None)
    ties += check(pre["out"]["actions"], a_s, f"C5 prefill of {obs.shape[1]} timesteps vs as many lram_step calls")
    # rec.final_state is the state after the leg's third (event-timed) prefill, which restarts every row and sees the same
    # inputs as the timed one (asserted above): so it is the timed prefill's state.  The state after the 18 decode steps is
    # not exported by the leg (the third prefill overwrites it); the decode steps are held to the step path by their actions.
    for (blk, w), t in rec.final_state.items():
        assert rel_err(t, eng.export_state_tensor(blk, w)) < 1e-4, f"C5 prefill vs step path: block {blk} state {w}"
    for i, c in enumerate(rec.calls[2:-1]):
        a = c["args"]
        a_s, _ = eng.step(a["obs"], a["rtg"], a["reward"], a["mask"])
        ties += check(c["out"]["actions"], a_s, f"C5 decode step {i}")
    eng.close()
    _report(f"C5: prefill + {len(rec.calls) - 3} decode steps vs the step path over {B} envs, ties {ties}")
    assert ties == 0, ties
