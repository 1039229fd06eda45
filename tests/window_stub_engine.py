"""Recording stand-in for lram_amd.engine.Engine in context-window mode, on the CPU (test infrastructure of
tests/test_window_api.py).  It keeps the per-env history the way the device ring does (tests/window_cases.History), checks the
control arrays with Engine's own host checks, and records, per step_window call, what it was handed and the padded windows
that call would feed the model."""
import torch

from lram_amd.engine import check_window_controls, check_window_timesteps
from tests.stub_engine import StubEngine
from tests.window_cases import History


class WindowStubEngine(StubEngine):
    def __init__(self, spec, state_dict, batch, device=None):
        super().__init__(spec, batch, torch.device("cpu"))
        self.K, self.hist, self.pad, self.calls = 0, None, None, []

    # -- what RecurrentAgent asks of an engine at construction
    def set_slot_table(self, *a):
        pass

    def set_sampling(self, *a, **k):
        pass

    def set_sampling_slots(self, *a, **k):
        pass

    def reset(self, mask=None):
        pass

    def set_live(self, n):
        raise AssertionError("window mode parks nobody")

    # -- the window calls
    def alloc_window(self, K):
        self.K = check_window_timesteps(K, self.batch, self.spec.d_model)
        self.hist = History(self.batch, self.K)

    def set_window_pad(self, vec, is_embedding=False):
        assert tuple(vec.shape) == ((self.spec.d_model if is_embedding else self.spec.state_dim),)
        self.pad = (vec.clone(), bool(is_embedding))

    def step_window(self, obs, rtg, prev_reward, reset=None, relabel=None, keep=None, pad="reference", discrete=False,
                    obs_is_embedding=False):
        assert self.K > 0 and pad in ("reference", "none")
        assert pad == "none" or (self.pad is not None and self.pad[1] == bool(obs_is_embedding))
        reset, relabel, keep = check_window_controls(reset, relabel, keep, self.batch)
        self.hist.step(obs, rtg, prev_reward, reset=reset, relabel=relabel, keep=keep)
        states, rtgs, rews = self.hist.tensors(pad_vec=self.pad[0] if pad == "reference" else None)
        self.calls.append({"prev_reward": prev_reward.clone(), "reset": reset, "relabel": relabel, "keep": keep, "pad": pad,
                           "states": states, "returns_to_go": rtgs, "rewards": rews, "counts": self.hist.counts})
        a = obs[:, :self.spec.act_dim] * 0.5 + rtg.view(-1, 1)
        return a, (a * 64).round().to(torch.int32)
