"""CPU (hipcc cross-compiles): the allowed-set rule is a compile-time split of the head kernels (csrc/action_head.h,
sample_kernels.hip, score_kernels.hip).  The masked instances need no scratch memory and spill no register; the unmasked
instances -- what every launch without a mask runs, bench.py's step among them -- keep the VGPR count, the LDS bytes and the
(zero) scratch they had before the masks.  Those numbers were read from a build of the commit before this rule and are written
down here, as tests/test_kernel_resources.py does for the shared GEMM pieces."""
import functools

import pytest

from tests.test_slot_state_resources import _one, _resources


@functools.lru_cache(maxsize=None)
def _res(src):
    return _resources(src)


MASKED = [("sample_kernels.hip", "action_argmax_masked_kernelE")] + \
    [("sample_kernels.hip", f"{k}ILi{per}EE") for k in ("action_sample_masked_kernel", "action_logp_masked_kernel",
                                                       "sample_rows_masked_kernel") for per in (1, 5, 8)] + \
    [("score_kernels.hip", f"{k}ILi{per}EE") for k in ("action_score_masked_kernel", "action_score_ragged_masked_kernel")
     for per in (0, 1, 5, 8)]


@pytest.mark.parametrize("src,kernel", MASKED)
def test_masked_instances_need_no_scratch_and_spill_nothing(src, kernel):
    r = _one(_res(src), kernel)
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["AGPRs"] == 0, r


# needle in the mangled name -> (VGPRs, LDS bytes per block) of the build before the masks; scratch and spills were 0 everywhere
_STAGE = {1: 1024, 5: 5120, 8: 8192}
PARENT = {("sample_kernels.hip", "action_argmax_kernelE"): (10, 0)}
for _per, _v in zip((1, 5, 8), ((30, 34, 28, 28, 34), (44, 46, 48, 42, 50), (54, 57, 64, 52, 64))):
    for _k, _n in zip(("action_sample_kernel", "action_sample_slots_kernel", "action_logp_kernel", "sample_tokens_kernel",
                       "sample_rows_kernel"), _v):
        PARENT[("sample_kernels.hip", f"{_k}ILi{_per}EE")] = (_n, _STAGE[_per])
for _per, _n, _lds in ((0, 47, 0), (1, 43, 1024), (5, 43, 5120), (8, 43, 8192)):
    for _k in ("action_score_kernel", "action_score_ragged_kernel"):
        PARENT[("score_kernels.hip", f"{_k}ILi{_per}EE")] = (_n, _lds)


@pytest.mark.parametrize("src,kernel", sorted(PARENT))
def test_unmasked_instances_keep_the_resources_they_had(src, kernel):
    r = _one(_res(src), kernel)
    vgprs, lds = PARENT[(src, kernel)]
    assert r["VGPRs"] == vgprs and r["LDS Size [bytes/block]"] == lds, (r, vgprs, lds)
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, r
