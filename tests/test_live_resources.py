"""CPU (hipcc cross-compiles): the two kernels behind parked env slots -- slot_swap_kernel (csrc/slot_state.hip: pure streaming,
2 x 4 16-byte pieces in flight per lane) and mlstm_lazy_parked_kernel (csrc/mlstm_lazy.hip: one wave per (head, env) carrying the
lazy bookkeeping over to the step's ping-pong side) -- need no scratch memory, spill no register and stay within 64 VGPRs, like
their siblings (tests/test_slot_state_resources.py)."""
import pytest

from tests.test_slot_state_resources import _one, _resources


@pytest.mark.parametrize("src,kernel", [("slot_state.hip", "slot_swap_kernel"), ("mlstm_lazy.hip", "mlstm_lazy_parked_kernel")])
def test_no_scratch_no_spills(src, kernel):
    r = _one(_resources(src), kernel)
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] <= 64 and r["AGPRs"] == 0, r           # eight waves per SIMD: both live on loads in flight
    assert r["LDS Size [bytes/block]"] == 0, r
