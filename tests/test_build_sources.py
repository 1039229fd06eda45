"""Every translation unit under lram_amd/csrc is part of the build and of the build id: a new *.hip file cannot be left out of
`build.SOURCES` (the link would miss its symbols) nor an entry of SOURCES point at nothing."""
import glob
import os

from lram_amd import build


def test_sources_are_exactly_the_hip_files_of_csrc():
    on_disk = {os.path.basename(f) for f in glob.glob(os.path.join(build.CSRC, "*.hip"))}
    assert len(build.SOURCES) == len(set(build.SOURCES)), "a source is listed twice"
    assert set(build.SOURCES) == on_disk, (sorted(on_disk - set(build.SOURCES)), sorted(set(build.SOURCES) - on_disk))
