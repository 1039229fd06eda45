"""Where the library may read the environment: the knob table of lram_create and the helpers of the
standalone test / micro-benchmark entries -- nothing on the step path, no process-wide copy of a knob, and the Python layer
never edits the environment to reach a kernel."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lram_amd", "csrc")


def _sources():
    paths = sorted(p for pat in ("*.hip", "*.h", "*.cpp", "*.inl") for p in glob.glob(os.path.join(CSRC, pat)))
    assert len(paths) > 30
    return {os.path.basename(p): open(p, encoding="utf-8").read() for p in paths}


def test_getenv_only_where_an_engine_is_created_and_in_the_standalone_entries():
    readers = sorted(name for name, text in _sources().items() if "getenv" in text)
    assert set(readers) <= {"engine.hip", "engine_gemm.hip", "engine_state.hip"}, readers
    assert "engine.hip" in readers   # (the knob loop itself)


def test_no_process_wide_gemm_knobs():
    for name, text in _sources().items():
        assert "gemm_knobs_reload" not in text and "g_knobs" not in text, name


def test_the_python_engine_does_not_touch_the_environment():
    with open(os.path.join(ROOT, "lram_amd", "engine.py"), encoding="utf-8") as f:
        assert "environ" not in f.read()
