"""CPU (hipcc cross-compiles): the per-slot state kernels (csrc/slot_state.hip) are pure streaming -- four 16-byte pieces in
flight per lane -- plus one small FMA tile kernel.  None of them may need scratch memory or spill a register: a spill would
turn a copy at HBM rate into one with a scratch round trip per piece, and no parity test would notice."""
import os
import re
import shutil
import subprocess

import pytest

from lram_amd import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lram_amd", "csrc")
FIELDS = "VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \\[bytes/lane\\]|LDS Size \\[bytes/block\\]"


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
        m = re.search(r"remark:\s+(%s):\s+(\d+)" % FIELDS, line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    assert res, out[-2000:]
    return res


def _one(res, needle):
    hits = [k for k in res if needle in k]
    assert len(hits) == 1, (needle, hits)
    return res[hits[0]]


def test_slot_state_source_is_part_of_the_build():
    assert "slot_state.hip" in build.SOURCES


@pytest.mark.parametrize("kernel", ["slot_copy_kernel", "slot_save_kernel", "slot_load_kernel", "slot_lazy_save_kernel",
                                    "slot_y_range_kernel"])
def test_no_scratch_no_spills(kernel):
    r = _one(_resources("slot_state.hip"), kernel)
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] <= 64 and r["AGPRs"] == 0, r           # eight waves per SIMD: a streaming kernel lives on loads in flight
    if kernel == "slot_lazy_save_kernel":
        assert r["LDS Size [bytes/block]"] <= 32 * 1024, r    # two workgroups per CU at least
