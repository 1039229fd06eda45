"""CPU: the bench recorder / replayer (tests/bench_replay.py) itself.  bench.main drives an oracle-backed stand-in engine
(tests/oracle_engine.py) through the headline's sequence; its replay is green, and each planted defect turns it red with a
message that names the call and the row."""
import re

import pytest
import torch

import bench
from lram_amd import preset
from tests.bench_replay import ReplayError, Session, bench_rows, replay, slice_bounds
from tests.oracle_engine import recording_factory

# 1000 env slots: the bench's schedule (phase = slot % 1000, episode length 1000) resets rows 993 ... 999 inside these 8 steps
B, W, K = 1000, 2, 6
ARGV = ["--gpus", "1", "--config", "xlstm_tiny", "--batch", str(B), "--warmup", str(W), "--steps", str(K)]


def _rows(spec, batch):
    return bench_rows(spec, batch, ep_len=1000, window=W + K)


def _bench(monkeypatch, **defect):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LRAM_DIST_SINGLE_RANK"):
        monkeypatch.delenv(k, raising=False)
    session = Session(_rows)
    bench.main(ARGV, engine_factory=recording_factory(session, **defect))
    session.close_all()
    assert len(session.records) == 1
    return session.records[0]


def test_row_sample_follows_the_bench_schedule():
    spec = preset("xlstm_tiny")
    rows = _rows(spec, B)
    assert rows[0] == 0 and rows[-1] == B - 1
    resets = [r for r in rows if 0 < 1000 - r % 1000 < W + K]
    assert len(resets) >= 2, rows
    assert any(r % 1000 <= 1000 - (W + K) and r != 0 for r in rows), rows   # a row that does not reset
    # make_slices: B / n rows per slice, the first B % n slices one more; graph mode and auto at small batches: one slice
    assert slice_bounds(spec, 1001, 2, False) == [(0, 501), (501, 1001)]
    assert slice_bounds(spec, 10, 3, False) == [(0, 4), (4, 7), (7, 10)]
    assert slice_bounds(spec, 4096, 0, True) == [(0, 4096)]
    assert slice_bounds(spec, 5, 16, False) == [(i, i + 1) for i in range(5)]
    big = preset("xlstm_16m")   # 4 heads x 256^2 x 4 bytes = 1 MiB per env: two slices from 512 envs
    assert slice_bounds(big, 511, 0, False) == [(0, 511)] and slice_bounds(big, 512, 0, False) == [(0, 256), (256, 512)]
    mamba = preset("mamba_48m")
    assert len(slice_bounds(mamba, 1023, 0, False)) == 1 and len(slice_bounds(mamba, 1024, 0, False)) == 2


def test_oracle_backed_stand_in_replays_green(monkeypatch):
    rec = _bench(monkeypatch)
    assert [c["kind"] for c in rec.calls] == ["set_micro_batches"] + ["step"] * (W + K)
    res = replay(rec)
    assert res == {"calls": 1 + W + K, "ties": 0, "relaxed": 0.0}


def _red(monkeypatch, **defect):
    rec = _bench(monkeypatch, **defect)
    with pytest.raises(AssertionError) as ex:
        replay(rec)
    msg = str(ex.value)
    m = re.search(r"call (\d+) \(step\) row (\d+)", msg)
    assert m, msg
    return int(m.group(1)), int(m.group(2)), msg


def test_ignored_reset_is_caught(monkeypatch):
    spec = preset("xlstm_tiny")
    row = max(r for r in _rows(spec, B) if r < B - 1)                  # phase 998: resets at step 2 (call 3)
    call, got_row, msg = _red(monkeypatch, defect="ignore_reset_row", defect_row=row)
    assert got_row == row and call > 1000 - row, msg


def test_stale_rtg_is_caught(monkeypatch):
    call, _, msg = _red(monkeypatch, defect="stale_rtg")
    assert call >= 2, msg


def test_previous_ring_slot_is_caught(monkeypatch):
    call, _, msg = _red(monkeypatch, defect="previous_ring_slot")
    assert call >= 2, msg


def test_one_action_off_by_one_bin_is_caught(monkeypatch):
    spec = preset("xlstm_tiny")
    row = _rows(spec, B)[2]
    call, got_row, msg = _red(monkeypatch, defect="action_off_by_one_bin", defect_row=row, defect_call=4)
    assert (call, got_row) == (5, row), msg   # (call 0 is set_micro_batches)


def test_a_call_the_replayer_does_not_model_fails_the_run(monkeypatch):
    rec = _bench(monkeypatch)
    eng = rec._engine
    rec.closed = False
    eng.import_state_tensor(0, 3, eng.export_state_tensor(0, 3))    # a state import: unknown to the replayer
    eng.close()
    with pytest.raises(ReplayError, match=r"call 9 \(import_state_tensor\)"):
        replay(rec)


def test_recorder_keeps_clones_not_references(monkeypatch):
    """The host-IO leg refills one device buffer before every step: the record must hold what each call saw."""
    from tests.oracle_engine import RecordingOracleEngine
    spec = preset("xlstm_tiny")
    session = Session(lambda s, b: [0, 2, 3])
    eng = type("R", (RecordingOracleEngine,), {"session": session})(spec, 4, "cpu")
    obs, rtg, zero = torch.zeros(4, spec.state_dim), torch.full((4,), 4.5), torch.zeros(4)
    for t in range(3):
        obs.fill_(0.1 * t)
        rtg.fill_(4.5 - 0.01 * t)
        eng.step(obs, rtg, zero, torch.ones(4, dtype=torch.uint8) if t == 0 else None)
    eng.close()
    rec = session.records[0]
    assert [float(c["args"]["obs"][1, 0]) for c in rec.calls] == pytest.approx([0.0, 0.1, 0.2])
    assert rec.calls[0]["args"]["obs"].shape == (3, spec.state_dim)
    assert replay(rec)["ties"] == 0


def _stand_in(rows=(0, 2, 3)):
    from tests.oracle_engine import RecordingOracleEngine
    spec = preset("xlstm_tiny")
    session = Session(lambda s, b: list(rows))
    eng = type("R", (RecordingOracleEngine,), {"session": session})(spec, 4, "cpu")
    g = torch.Generator().manual_seed(3)
    for t in range(3):
        eng.step(torch.rand(4, spec.state_dim, generator=g) * 2 - 1, torch.full((4,), 4.5 - 0.01 * t), torch.zeros(4),
                 torch.ones(4, dtype=torch.uint8) if t == 0 else None)
    return eng, session.records[0]


def test_hidden_tap_is_compared_after_a_trailing_setter():
    """bench.main's standalone sub-leg ends with set_micro_batches after its last step: the hidden tap is still that step's,
    it is kept and compared, and a record that ends with a step cannot skip the comparison."""
    eng, rec = _stand_in()
    eng.set_micro_batches(1)
    eng.close()
    assert rec.calls[-1]["kind"] == "set_micro_batches" and rec.hidden is not None
    lines = []
    assert replay(rec, report=lines.append)["relaxed"] == 0.0 and "float64-rule rows 0.00%" in lines[0]
    good = rec.hidden
    rec.hidden = good.clone()
    rec.hidden[1, 1, 0] += 1e-2 * float(good.abs().max())     # one element of row 2's rtg-token hidden state off
    with pytest.raises(AssertionError, match="final hidden tap"):
        replay(rec)
    rec.hidden = None
    with pytest.raises(AssertionError, match="ends with a step but holds no hidden tap"):
        replay(rec)


def test_report_says_when_no_hidden_tap_was_compared():
    eng, rec = _stand_in()
    eng.reset(torch.tensor([0, 1, 0, 0], dtype=torch.uint8))
    eng.close()
    assert rec.hidden is None
    lines = []
    res = replay(rec, report=lines.append)
    assert res["relaxed"] is None and "float64-rule rows n/a" in lines[0], lines
