"""CPU: the argument rules of the stored contexts from frames (lram_amd.engine.check_frame_contexts, Engine.embed_frames'
shape rule, RecurrentAgent._prepare_contexts) and the agreement of the ctypes table with include/lram_hip.h on the four new
entries.  No GPU, no library: the engine methods are run on an object that has only the fields the checks read."""
import ctypes
import os
import re

import pytest
import torch

from lram_amd import engine
from lram_amd.engine import Engine, check_frame_contexts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lram_hip.h")
NEW_SYMBOLS = ("lram_embed_frames", "lram_prefill_frames", "lram_score_frames", "lram_image_counts")


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m is not None, f"{name} is not declared in include/lram_hip.h"
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_ctypes_table_and_header_agree_on_the_frame_entries():
    for name in NEW_SYMBOLS:
        args = _declaration(name)
        restype, argtypes = engine._SYMBOLS[name]
        assert restype is ctypes.c_int32 and len(argtypes) == len(args), name
        for decl, ct in zip(args, argtypes):
            if "*" in decl:
                assert ct is engine._VP or issubclass(ct, ctypes._Pointer), (name, decl)
            elif decl.startswith("int64_t"):
                assert ct is ctypes.c_int64, (name, decl)
            elif decl.startswith("double"):
                assert ct is ctypes.c_double, (name, decl)
            else:
                assert decl.startswith("int32_t") and ct is ctypes.c_int32, (name, decl)
    # the dense entries' arguments plus frames, channels, height, width, lengths and append, less obs_is_embedding (the
    # observations of a frames call are the vector slots' and never embeddings)
    for frames, dense in (("lram_prefill_frames", "lram_prefill"), ("lram_score_frames", "lram_score")):
        mine, theirs = _declaration(frames), _declaration(dense)
        assert len(mine) == len(theirs) + 5 and "int32_t obs_is_embedding" in theirs and "int32_t obs_is_embedding" not in mine
        assert [a for a in theirs if a in mine] == [a for a in mine if a in theirs]      # in the same order
    assert "lram_embed_images" in engine._SYMBOLS     # stays as it is


def test_frame_context_shapes():
    f = torch.zeros(7, 21, 3, 21, 21, dtype=torch.uint8)
    assert check_frame_contexts(f, None, 7, None, 20) == (21, 3, 21, 21)
    assert check_frame_contexts(f, torch.zeros(2, 2), 7, None, 20) == (21, 3, 21, 21)      # nobody reads it: not looked at
    assert check_frame_contexts(f, None, 7, 7, 20) == (21, 3, 21, 21)                      # a table of image slots only
    obs = torch.zeros(9, 21, 20)
    assert check_frame_contexts(f, obs, 9, 7, 20) == (21, 3, 21, 21)                       # 7 image slots among 9
    for bad, needle in ((f.float(), "uint8"), (f[0], "uint8 tensor [n, L, C, H, W]"), ("frames", "uint8"),
                        (f[:6], "expected 7 rows"), (f[:, :0], ">= 1")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            check_frame_contexts(bad, None, 7, None, 20)
    with pytest.raises(ValueError, match="one row per image slot"):
        check_frame_contexts(f, obs, 9, 3, 20)
    with pytest.raises(ValueError, match="no image slot"):
        check_frame_contexts(f, obs, 9, 0, 20)
    with pytest.raises(ValueError, match="vector slots"):
        check_frame_contexts(f, None, 9, 7, 20)
    for wrong in (torch.zeros(9, 20, 20), torch.zeros(9, 21, 19), torch.zeros(7, 21, 20), torch.zeros(9, 21, 20, dtype=torch.float64)):
        with pytest.raises(ValueError, match="obs_seq: expected float32"):
            check_frame_contexts(f, wrong, 9, 7, 20)


class _Bare:
    """What Engine's frame methods read before they reach the library."""
    def __init__(self, batch, slot_image=None):
        from lram_amd.config import ModelSpec
        self.batch, self._live, self._slot_image = batch, batch, slot_image
        self.spec = ModelSpec(backbone="xlstm", d_model=128, n_blocks=2, slstm_at=[1], image_shape=(3, 21, 21))
        self.device = torch.device("cpu")

    def _need_all_live(self, what):
        pass

    _frames_context_call = Engine._frames_context_call


def test_engine_methods_refuse_bad_arguments_before_the_library():
    bare = _Bare(7)
    f = torch.zeros(7, 4, 3, 21, 21, dtype=torch.uint8)
    rtg = torch.zeros(7, 4)
    with pytest.raises(ValueError, match="rtg_seq"):
        Engine.prefill_frames(bare, f, torch.zeros(7, 5), rtg)
    with pytest.raises(ValueError, match="reward_seq"):
        Engine.prefill_frames(bare, f, rtg, rtg.double())
    with pytest.raises(ValueError, match="expected 7 rows"):
        Engine.prefill_frames(bare, f[:3], rtg, rtg)
    with pytest.raises(ValueError, match="lengths"):
        Engine.prefill_frames(bare, f, rtg, rtg, lengths=[4, 4, 4, 5, 0, 0, 0])
    with pytest.raises(ValueError, match="every length is 0"):
        Engine.score_frames(bare, f, rtg, rtg, lengths=[0] * 7, append=True)
    with pytest.raises(ValueError, match="unknown output"):
        Engine.score_frames(bare, f, rtg, rtg, want=("logits",))
    with pytest.raises(ValueError, match="reset_mask"):
        Engine.prefill_frames(bare, f, rtg, rtg, reset_mask=torch.zeros(7))
    mixed = _Bare(7, slot_image=torch.tensor([1, 1, 1, 0, 0, 0, 0], dtype=torch.bool))
    with pytest.raises(ValueError, match="one row per image slot"):
        Engine.prefill_frames(mixed, f, rtg, rtg, obs_seq=torch.zeros(7, 4, mixed.spec.state_dim))
    with pytest.raises(ValueError, match="vector slots"):
        Engine.prefill_frames(mixed, f[:3], rtg, rtg)
    for bad in (torch.zeros(3, 21, 21), torch.zeros(2, 3, 21, 21), torch.zeros(0, 3, 21, 21, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="frames"):
            Engine.embed_frames(bare, bad)


def test_agent_prepares_frames_and_pairs():
    from lram_amd.agent import RecurrentAgent
    from lram_amd.domains import Domain, SlotTable

    class _Agent:
        _prepare_contexts = RecurrentAgent._prepare_contexts
        _prepare_obs = RecurrentAgent._prepare_obs

        def __init__(self, n, table=None, encoder=True):
            self.n_envs, self.slot_table, self.has_image_encoder = n, table, encoder
            self.spec, self.device, self.is_discrete = _Bare(n).spec, torch.device("cpu"), False
            self.state_mean = self.state_std = None

    f = torch.randint(0, 256, (4, 6, 3, 21, 21), dtype=torch.uint8)
    rtg = torch.zeros(4, 6)
    obs, frames, r, rew, lengths, discrete = _Agent(4)._prepare_contexts(f, rtg, None, [6, 2, 0, 1])
    assert obs is None and torch.equal(frames, f) and frames.is_contiguous() and lengths == [6, 2, 0, 1] and discrete is False
    assert rew.shape == (4, 6) and not rew.any()
    with pytest.raises(RuntimeError, match="embed_image"):
        _Agent(4, encoder=False)._prepare_contexts(f, rtg, None, None)
    with pytest.raises(ValueError, match="expected uint8"):
        _Agent(5)._prepare_contexts(f, torch.zeros(5, 6), None, None)
    with pytest.raises(ValueError, match="slot table"):
        _Agent(4)._prepare_contexts((torch.zeros(4, 6, 3), f), rtg, None, None)
    tab = SlotTable.from_domains([(Domain("procgen", True, 1, image=True), 2), (Domain("metaworld", False, 3), 2)], max_act_dim=8)
    agent = _Agent(4, tab)
    vec = torch.ones(4, 6, 5)
    obs, frames, _, _, _, discrete = agent._prepare_contexts((vec, f[:2]), rtg, None, None)
    assert discrete == "per_slot" and frames.shape[0] == 2 and obs.shape == (4, 6, agent.spec.state_dim)
    assert bool((obs[..., :5] == 1).all()) and not obs[..., 5:].any()
    for bad, needle in (((vec, f), "expected uint8 [2,"), ((None, f[:2]), "vector_obs"), ((vec[:, :5], f[:2]), "vector_obs"),
                        (f, "pair"), ((vec, None), "frames")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            agent._prepare_contexts(bad, rtg, None, None)
    # vector observations go on as before
    obs, frames, _, _, _, _ = _Agent(4)._prepare_contexts(torch.ones(4, 6, 5), rtg, None, None)
    assert frames is None and obs.shape == (4, 6, agent.spec.state_dim)
