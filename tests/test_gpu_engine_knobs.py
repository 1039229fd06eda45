"""GPU: an engine's launch knobs are its own -- read at lram_create, untouched by engines created
later, and never reached by editing the environment from Python."""
import os

import pytest
import torch

from lram_amd import init_state_dict, preset
from tests.helpers import make_inputs

pytestmark = pytest.mark.gpu

LATE_BLOCK = 7   # the last mLSTM block of xlstm_16m: its state has seen every projection of the stack


def _engine(spec, sd, B):
    from lram_amd.engine import Engine
    eng = Engine(spec, sd, B, device="cuda:0")
    eng.set_micro_batches(1)
    return eng


def _run(eng, seq):
    acts = []
    for obs, rtg, rew, mask in seq:
        a, _ = eng.step(obs.cuda(), rtg.cuda(), rew.cuda(), mask.cuda())
        acts.append(a.clone())
    torch.cuda.synchronize()
    return torch.stack(acts).cpu(), [eng.export_state_tensor(LATE_BLOCK, which).cpu() for which in range(4)]   # C, n, m, conv


def test_a_second_engine_does_not_change_the_first(hip_lib, monkeypatch):
    """Engine A is created under LRAM_SPLITK_TILES=0 (no projection is split along K), engine B afterwards with the variable
    unset, and only then both step: A must run as engine C does, which is created and stepped alone under the same setting
    (bit for bit), and not as B does.  160 envs = 480 rows: beyond the few-row kernel's 384, and proj_down (480 x 512 x 1024)
    is 16 tiles of 128 x 128 -- fewer than the default threshold of 56, so B splits it along K and sums in another order.
    The last assertion holds the test to that: were no projection split by default at this batch, A and B would agree and
    the test would say nothing."""
    spec = preset("xlstm_16m")
    sd = init_state_dict(spec, seed=73)
    B = 160
    seq = make_inputs(spec, B, 4, seed=33, reset_prob=0.1)
    monkeypatch.setenv("LRAM_SPLITK_TILES", "0")
    a = _engine(spec, sd, B)
    monkeypatch.delenv("LRAM_SPLITK_TILES")
    b = _engine(spec, sd, B)
    act_a, st_a = _run(a, seq)
    act_b, st_b = _run(b, seq)
    a.close(), b.close()
    monkeypatch.setenv("LRAM_SPLITK_TILES", "0")
    c = _engine(spec, sd, B)
    monkeypatch.delenv("LRAM_SPLITK_TILES")
    act_c, st_c = _run(c, seq)
    c.close()
    assert torch.equal(act_a, act_c)
    for which in range(4):
        assert torch.equal(st_a[which], st_c[which]), which
    assert any(not torch.equal(x, y) for x, y in zip(st_a, st_b))


@pytest.mark.parametrize("m,n,k", [(300, 300, 2560), (513, 300, 64)])
def test_the_8_phase_entry_needs_no_environment_edit(hip_lib, monkeypatch, m, n, k):
    """kernel="f16x2p8" is an entry of its own: it reaches the 8-phase kernel (bit-identical to the f16x2 kernel) whatever
    LRAM_GEMM_TILE says, and leaves the variable alone."""
    from lram_amd.engine import gemm_f32
    g = torch.Generator().manual_seed(m + n + k)
    a, w, bias = torch.randn(m, k, generator=g).cuda(), torch.randn(n, k, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    monkeypatch.setenv("LRAM_GEMM_TILE", "64")
    got = gemm_f32(a, w, bias, kernel="f16x2p8")
    ref = gemm_f32(a, w, bias, kernel="f16x2")
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert os.environ["LRAM_GEMM_TILE"] == "64"
