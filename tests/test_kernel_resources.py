"""CPU (hipcc cross-compiles): register / LDS budgets the engine's co-residency reasoning relies on.

Several launch decisions assume how many workgroups of one kernel fit on a CU BESIDE another kernel's (DESIGN.md section 0 item 3,
profiles/r05_ab_206m_chain.txt, r05_ab_read_pass_lds_cap.txt):
  * the sliced-head read pass (206M geometry) is held at two workgroups per CU by its REGISTER count (> 170 VGPRs: twelve registers
    are kept live across the pass for exactly this), so that the other slice's projection workgroups find room;
  * those projection workgroups must fit into what two such read passes leave: the two-stage pre-split GEMM <= 128 VGPRs and about
    65 KB of LDS, the two-stage on-the-fly GEMM <= 160 VGPRs and 48 KB;
  * the 256-wide-head read pass stays at <= 128 VGPRs (three workgroups per CU at 41 KB of LDS, two at 54 KB).
A compiler upgrade that moves these numbers silently changes occupancy, not results -- no parity test would notice."""
import os
import re
import shutil
import subprocess

import pytest

from lram_amd import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lram_amd", "csrc")


def _resources(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc] + list(build.FLAGS) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src),
                                         "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|LDS Size \[bytes/block\]|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]):\s+(\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    assert res, out[-2000:]
    return res


def _one(res, *needles):
    hits = [k for k in res if all(n in k for n in needles)]
    assert len(hits) == 1, (needles, hits)
    return res[hits[0]]


def test_read_pass_register_budgets():
    res = _resources("mlstm_lazy.hip")
    sliced = _one(res, "mlstm_lazy_cell_kernelILi3ELi32ELi16ELin1E")          # T = 3, 128-column slices, scores from the score kernel
    assert 171 <= sliced["VGPRs"] <= 256 and sliced["AGPRs"] == 0, sliced        # two workgroups per CU, by registers
    assert sliced["VGPRs Spill"] == 0
    wide = _one(res, "mlstm_lazy_cell_kernelILi3ELi64ELi8ELi4E")                 # T = 3, 256-wide heads (the headline kernel)
    assert wide["VGPRs"] <= 128 and wide["VGPRs Spill"] == 0, wide


def test_projection_workgroups_fit_beside_two_read_passes():
    res = _resources("gemm_f16x2p.hip")
    two_stage = _one(res, "gemm_f16x2p_kernelILb0ELb0ELi2ELi2ELi2ELi2E")         # 128 x 128 tile, two LDS stages
    assert two_stage["VGPRs"] <= 128 and two_stage["LDS Size [bytes/block]"] <= 68 * 1024, two_stage
    one_stage = _one(res, "gemm_f16x2p_kernelILb0ELb0ELi1ELi2ELi2ELi2E")         # 128 x 128 tile, one stage: four per CU
    assert one_stage["VGPRs"] <= 128 and one_stage["LDS Size [bytes/block]"] <= 36 * 1024, one_stage


def test_on_the_fly_projection_workgroup_budget():
    res = _resources("gemm_f16x2.hip")
    two_stage = _one(res, "gemm_f16x2_kernelILb0ELb1ELi64ELb0ELb1E")            # proj_down of chain-bound slices: 64-row tile, two stages
    assert two_stage["VGPRs"] <= 160 and two_stage["LDS Size [bytes/block]"] <= 48 * 1024, two_stage
    gated = _one(res, "gemm_f16x2_kernelILb0ELb1ELi64ELb1ELb0E")                # proj_down of the headline: 64-row tile, gate in the staging
    assert gated["VGPRs"] <= 128 and gated["LDS Size [bytes/block]"] <= 36 * 1024, gated


# The GEMM kernels outside the f16x2 family share their batch addressing, tile order, K range and epilogue through macros and
# inlined functions (csrc/gemm_tile.h, the macros of gemm_narrow.hip): what an instance occupies must not move with them.
# (LDS bytes per workgroup, waves per SIMD) of the build the sharing was introduced on; no scratch and no spill in any of them.
_PINNED = {
    "gemm_bf16x3.hip": {"gemm_bf16x3_kernelILb0ELb0ELi128ELb0E": (61440, 2),       # 128-row tile
                        "gemm_bf16x3_kernelILb0ELb0ELi64ELb0E": (46080, 3),        # 64-row tile
                        "gemm_bf16x3_kernelILb0ELb1ELi64ELb1E": (46080, 3)},       # ... gated (proj_down)
    "gemm_f32.hip": {"gemm_f32_kernelILb0ELb0E": (36864, 3),
                     "gemm_skinny_kernelILb0ELb0ELi4ELi8ELb0ELb0E": (16896, 4)},
    "gemm_narrow.hip": {**{f"gemm_narrow_kernelILi{j}ELb0E": v for j, v in
                           zip(range(1, 7), ((20480, 4), (24576, 3), (28672, 2), (32768, 2), (36864, 1), (40960, 1)))},
                        **{f"gemm_narrow16_kernelILi{j}ELb0E": v for j, v in
                           zip(range(1, 7), ((20608, 4), (24704, 2), (28800, 2), (32896, 1), (36992, 1), (41088, 1)))}},
}


@pytest.mark.parametrize("src", sorted(_PINNED))
def test_shared_gemm_pieces_cost_no_scratch_lds_or_occupancy(src):
    res = _resources(src)
    for needle, (lds, occupancy) in _PINNED[src].items():
        r = _one(res, needle)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (needle, r)
        assert r["LDS Size [bytes/block]"] == lds and r["Occupancy [waves/SIMD]"] == occupancy, (needle, r)
