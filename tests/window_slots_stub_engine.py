"""Recording stand-in for lram_amd.engine.Engine in context-window mode with set_window_slots("own"), on the CPU (test
infrastructure of tests/test_window_slots_api.py).  On top of tests/window_stub_engine.WindowStubEngine it keeps a live count,
steps the live prefix of its per-slot histories only, moves whole histories the way the window movers move windows (with
Engine's own host checks of the lists) and logs every slot call in `moves`."""
import copy

import torch

from lram_amd.engine import check_slot_lists, check_swap_lists, check_window_controls
from tests.window_cases import History
from tests.window_stub_engine import WindowStubEngine


class WindowSlotsStubEngine(WindowStubEngine):
    def __init__(self, spec, state_dict, batch, device=None):
        super().__init__(spec, state_dict, batch, device)
        self.live, self.window_slots, self.moves, self.rows_stepped = batch, "shared", [], 0

    def set_window_slots(self, mode):
        assert mode in ("shared", "own") and self.K > 0
        self.window_slots = mode

    def set_live(self, n):
        assert 1 <= n <= self.batch
        self.live = int(n)
        self.moves.append(("set_live", int(n)))

    def swap_slots(self, a, b):
        a, b = check_swap_lists(a, b, self.batch)
        self.moves.append(("swap_slots", a, b))

    def copy_slots(self, *a):
        raise AssertionError("own-window mode forks windows, not recurrent state")

    save_slots = load_slots = copy_slots

    # -- the window movers
    def swap_window_slots(self, a, b):
        a, b = check_swap_lists(a, b, self.batch)
        for x, y in zip(a, b):
            self.hist.rows[x], self.hist.rows[y] = self.hist.rows[y], self.hist.rows[x]
        self.moves.append(("swap_window_slots", a, b))

    def copy_window_slots(self, src, dst):
        src, dst = check_slot_lists(src, dst, self.batch)
        for x, y in zip(src, dst):
            self.hist.rows[y] = copy.deepcopy(self.hist.rows[x])
        self.moves.append(("copy_window_slots", src, dst))

    @property
    def window_slot_numel(self):
        return self.K * (self.spec.state_dim + 2) + 1

    def save_window_slots(self, slots):
        """Records in the engine's layout over the stub's entries (prepared observations in place of embeddings)."""
        K, W = self.K, self.spec.state_dim
        out = torch.zeros(len(slots), self.window_slot_numel)
        for i, b in enumerate(slots):
            h = self.hist.rows[b]
            for j, (v, g, r) in enumerate(h):
                t = K - len(h) + j
                out[i, t * W:(t + 1) * W], out[i, K * W + t], out[i, K * W + K + t] = v, float(g), float(r)
            out[i, -1] = len(h)
        self.moves.append(("save_window_slots", list(slots)))
        return out

    def load_window_slots(self, slots, records):
        import numpy as np
        slots, _ = check_slot_lists(slots, None, self.batch)
        K, W = self.K, self.spec.state_dim
        for i, b in enumerate(slots):
            n = int(records[i, -1])
            self.hist.rows[b] = [[records[i, t * W:(t + 1) * W].clone(), np.float32(records[i, K * W + t]),
                                  np.float32(records[i, K * W + K + t])] for t in range(K - n, K)]
        self.moves.append(("load_window_slots", slots))

    # -- the step: the live prefix in "own" mode
    def step_window(self, obs, rtg, prev_reward, reset=None, relabel=None, keep=None, pad="reference", discrete=False,
                    obs_is_embedding=False):
        if self.window_slots != "own":
            assert self.live == self.batch, "shared mode steps every slot"
            self.rows_stepped += self.batch
            return super().step_window(obs, rtg, prev_reward, reset, relabel, keep, pad, discrete, obs_is_embedding)
        n = self.live
        assert obs.shape[0] == rtg.shape[0] == prev_reward.shape[0] == n, "own mode takes `live` rows"
        reset, relabel, keep = check_window_controls(reset, relabel, keep, n)
        part = History(n, self.K)
        part.rows = self.hist.rows[:n]      # (the same lists: the live slots' histories are stepped in place)
        part.step(obs, rtg, prev_reward, reset=reset, relabel=relabel, keep=keep)
        self.rows_stepped += n
        self.calls.append({"prev_reward": prev_reward.clone(), "reset": reset, "relabel": relabel, "keep": keep, "pad": pad,
                           "obs": obs.clone(), "rtg": rtg.clone(), "live": n, "counts": self.hist.counts})
        a = obs[:, :self.spec.act_dim] * 0.5 + rtg.view(-1, 1)
        return a, (a * 64).round().to(torch.int32)
