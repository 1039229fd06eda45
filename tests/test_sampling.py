"""CPU: the sampling head's host side and the references its GPU tests lean on.

  * tests/sampling_ref.py (float64 numpy restatement of the row rule of lram_set_sampling) reproduces the probabilities
    recorded from the reference's own sample_from_logits (tests/golden/sampling_reference.npz) to 1e-12, so it may stand in
    for the reference on live logits;
  * its Philox4x32-10 gives the published Random123 known answers;
  * `a_sample_kwargs` travels YAML override -> load_agent_params -> spec_from_agent_params -> RecurrentAgent -> the engine;
  * the library exports and binds the four new entries; the new kernels compile without spills."""
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from lram_amd import build, engine, load_agent_params, preset, spec_from_agent_params
from tests import sampling_ref as sr
from tests.test_config_weights import _write_tree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_reference.npz")
NEW_SYMBOLS = ("lram_set_sampling", "lram_get_sampling", "lram_sample_tokens", "lram_sample_uniforms")


def test_restatement_reproduces_the_recorded_reference_probabilities():
    g = np.load(GOLDEN)
    C = len(g["n"])
    assert C >= 64 and set(int(x) for x in g["n"]) == {18, 274}
    seen = set()
    for c in range(C):
        n, t, k, p = int(g["n"][c]), float(g["temperature"][c]), int(g["top_k"][c]), float(g["top_p"][c])
        seen.add((t, k if k not in (18, 274) else "n", p))
        want = g["probs"][c, :n]
        assert abs(want.sum() - 1.0) < 1e-12 and not g["probs"][c, n:].any()
        got = sr.row_probs(g["logits"][c, :n], t, k, p)
        assert got is not None, g["name"][c]
        assert np.array_equal(got > 0, want > 0), g["name"][c]          # the same support
        assert np.abs(got - want).max() <= 1e-12, (g["name"][c], np.abs(got - want).max())
    for kw in [(1.0, 0, 0.0), (0.75, 0, 0.5), (1.0, 0, 0.5), (2.0, 5, 0.0), (1.0, 10, 0.9), (1.0, 50, 0.9), (0.5, 1, 0.0), (1.0, "n", 0.0)]:
        assert kw in seen, kw
    names = " ".join(str(x) for x in g["name"])
    for kind in ("flat", "neginf", "ties", "peaked40"):
        assert kind in names


def test_restatement_edge_rules():
    row = np.array([0.5, 2.0, -1.0, 2.0, 0.25], dtype=np.float32)
    p = sr.row_probs(row, 1.0, 1, 0.0)              # a tie at the k-th place: the lowest index stays
    assert p[1] == 1.0 and p.sum() == 1.0
    tok, _ = sr.inverse_cdf(np.array([0.0, 0.25, 0.0, 0.75, 0.0]), np.array([0.0, 0.2499, 0.25, np.nextafter(1.0, 0.0)]))
    assert tok.tolist() == [1, 1, 3, 3]            # zero-probability entries are never returned, u = 0 and u -> 1 included
    assert sr.row_probs(np.array([0.0, np.nan, 1.0], dtype=np.float32)) is None
    assert sr.row_probs(np.array([0.0, np.inf, 1.0], dtype=np.float32)) is None
    assert sr.argmax_rule(np.array([0.0, np.nan, 7.0, np.nan])) == 1 and sr.argmax_rule(np.array([1.0, 3.0, 3.0])) == 1
    flat = sr.row_probs(np.full(18, 0.625, dtype=np.float32), 1.0, 0, 0.5)   # the quantile equals the maximum: nothing is dropped
    assert np.allclose(flat, 1.0 / 18)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = sr.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert tuple(int(x) for x in got) == want
    # the counter / key layout of the head: (slot, dim, draw lo, draw hi) / (seed lo, seed hi)
    u = sr.uniforms(seed=0x299f31d0a4093822, slot_base=0x243f6a88 - 1, n_slots=2, act_dim=0x85a308d3 % 7 + 1, draw=0)
    assert u.shape == (2, 0x85a308d3 % 7 + 1) and (u >= 0).all() and (u < 1).all()
    one = sr.philox4x32_10(np.array([0x243f6a88, 3, 0x13198a2e, 0x03707344], dtype=np.uint64),
                           np.array([0xa4093822, 0x299f31d0], dtype=np.uint64))
    got = sr.uniforms(seed=0x299f31d0a4093822, slot_base=0x243f6a88 - 1, n_slots=2, act_dim=4, draw=0x0370734413198a2e)
    assert got[1, 3] == float(one[0]) * 2.0 ** -32
    # two shards draw what one engine over all slots would
    whole = sr.uniforms(7, 0, 16, 3, 5)
    assert np.array_equal(whole[8:], sr.uniforms(7, 8, 8, 3, 5))


class _RecorderEngine:
    """Stands in for lram_amd.engine.Engine inside RecurrentAgent (as test_agent_predict_follows_the_reference_trace does)."""
    made = []

    def __init__(self, spec, state_dict, batch, device=None):
        self.spec, self.batch, self.device = spec, batch, torch.device("cpu")
        self.sampling_calls, self.closed = [], False
        _RecorderEngine.made.append(self)

    def set_sampling(self, temperature=1.0, top_k=0, top_p=0.0, seed=0, slot_base=0):
        self.sampling_calls.append(dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, slot_base=slot_base))

    def set_graph_mode(self, on):
        pass

    def close(self):
        self.closed = True


def test_a_sample_kwargs_travel_from_the_config_to_the_engine(tmp_path, monkeypatch):
    from lram_amd import agent as agent_mod
    _write_tree(str(tmp_path))
    base = ["agent_params/huggingface=xl_med", "agent_params.kind=MDDXLSTM"]
    spec0 = spec_from_agent_params(load_agent_params(str(tmp_path), "multi_domain", base))
    assert spec0.a_sample_kwargs is None
    ap = load_agent_params(str(tmp_path), "multi_domain", base + ["+agent_params.a_sample_kwargs={temperature: 0.75, top_k: 10}"])
    spec = spec_from_agent_params(ap)
    assert spec.a_sample_kwargs == {"temperature": 0.75, "top_k": 10}
    assert spec_from_agent_params(load_agent_params(str(tmp_path), "multi_domain", base + ["+agent_params.a_sample_kwargs={}"])
                                  ).a_sample_kwargs == {}
    assert dataclasses.replace(spec, a_sample_kwargs=None) == spec0
    for name in ("xlstm_16m", "mamba_48m", "xlstm_tiny"):
        assert preset(name).a_sample_kwargs is None

    monkeypatch.setattr(agent_mod, "Engine", _RecorderEngine)
    tiny = preset("xlstm_tiny")
    a = agent_mod.RecurrentAgent(tiny, {}, n_envs=2)                       # None: the engine is never armed
    assert a.a_sample_kwargs is None and a.engine.sampling_calls == [] and "a_sample_kwargs" not in a.trajectory_mode
    a = agent_mod.RecurrentAgent(tiny, {}, n_envs=2, a_sample_kwargs={}, sample_seed=11, sample_slot_base=64)
    want = dict(temperature=1.0, top_k=0, top_p=0.5, seed=11, slot_base=64)  # sample_from_logits' own defaults
    assert a.engine.sampling_calls == [want]
    assert a.trajectory_mode["a_sample_kwargs"] == want
    first = a.engine
    a.make_pickleable()
    assert first.closed and a.engine is None
    a.reinit_cuda_kernels()
    assert a.engine is not first and a.engine.sampling_calls == [want]      # armed again on the fresh engine
    a = agent_mod.RecurrentAgent(dataclasses.replace(tiny, a_sample_kwargs={"temperature": 0.75, "top_k": 10}), {}, n_envs=1)
    assert a.engine.sampling_calls == [dict(temperature=0.75, top_k=10, top_p=0.5, seed=0, slot_base=0)]
    a = agent_mod.RecurrentAgent(tiny, {}, n_envs=1, discrete=True, a_sample_kwargs={"top_k": 18, "top_p": 0.0})
    assert a.engine.sampling_calls[0]["top_k"] == 18
    with pytest.raises(KeyError):
        agent_mod.RecurrentAgent(tiny, {}, a_sample_kwargs={"temp": 1.0})
    for bad in ({"temperature": 0.0}, {"temperature": -1.0}, {"temperature": float("inf")}, {"temperature": float("nan")},
                {"top_p": 1.5}, {"top_p": -0.1}, {"top_k": -1}, {"top_k": tiny.n_vocab + 1}, {"top_k": 2.5}):
        with pytest.raises(ValueError):
            agent_mod.RecurrentAgent(tiny, {}, a_sample_kwargs=bad)
    with pytest.raises(ValueError):                                            # the discrete head has n_discrete logits per row
        agent_mod.RecurrentAgent(tiny, {}, discrete=True, a_sample_kwargs={"top_k": tiny.n_discrete + 1})


def test_library_exports_and_binds_the_sampling_entries(hip_lib):
    header = open(os.path.join(build.CSRC, "..", "..", "include", "lram_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in engine._SYMBOLS and getattr(hip_lib, name).argtypes == engine._SYMBOLS[name][1]
        assert re.search(r"\b%s\s*\(" % name, header)
    assert "sample_kernels.hip" in build.SOURCES
    assert hip_lib.lram_abi_version() == 1
    # argument checks that need no device: a null engine / null pointers are errors with a text
    assert hip_lib.lram_set_sampling(None, 1, 1.0, 0, 0.0, 0, 0) != 0 and b"lram_set_sampling" in hip_lib.lram_last_error()
    assert hip_lib.lram_sample_tokens(None, 1, 18, 18, 1.0, 0, 0.0, None, None, None) != 0
    assert b"lram_sample_tokens" in hip_lib.lram_last_error()
    assert hip_lib.lram_destroy(None) == 0 and hip_lib.lram_last_error() == b""   # (a success clears the thread's error text)
    for name in ("set_sampling", "sampling"):
        assert hasattr(engine.Engine, name)
    assert callable(engine.sample_tokens) and callable(engine.sample_uniforms)


def test_sampling_kernels_have_no_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc] + list(build.FLAGS) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                         os.path.join(build.CSRC, "sample_kernels.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]):\s+(\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    heads = [k for k in res if "action_sample_kernel" in k]
    assert len(heads) == 3 and any("sample_tokens_kernel" in k for k in res), sorted(res)
    for k, r in res.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert r["VGPRs"] <= 64, (k, r)     # eight waves per SIMD
