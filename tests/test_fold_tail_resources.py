"""CPU (hipcc cross-compiles): the bookkeeping kernel that completes a tail fold outside its step (mlstm_lazy_folded_kernel) is a
handful of loads and stores per lane -- no LDS, no scratch, no spills."""
import os
import re
import shutil
import subprocess

import pytest

from lram_amd import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lram_amd", "csrc")


def test_folded_kernel_uses_no_lds_and_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc] + list(build.FLAGS) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                         os.path.join(CSRC, "mlstm_lazy.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(LDS Size \[bytes/block\]|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill):\s+(\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    hits = [k for k in res if "mlstm_lazy_folded_kernel" in k]
    assert len(hits) == 1, (hits, out[-2000:])
    r = res[hits[0]]
    assert r == {"LDS Size [bytes/block]": 0, "ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}, r
