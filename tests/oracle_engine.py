"""Stand-in for lram_amd.engine.Engine backed by the fp32 CPU oracle, with defects to plant (test infrastructure for
tests/test_bench_replay.py; bench.py --engine-factory).

Without a defect it computes what the oracle computes, so a replay of it (tests/bench_replay.py) must come out green; each
defect is one way a fast engine could be wrong in a bench sequence, and the replay must name the call and the row it shows in."""
import torch

from lram_amd import init_state_dict
from oracle.dt_ref import OraclePolicy, minmax_inv_tokenize
from tests.bench_replay import RecordingMixin

DEFECTS = (None, "ignore_reset_row", "stale_rtg", "previous_ring_slot", "action_off_by_one_bin")


class OracleEngine:
    """step() of all env slots through OraclePolicy (weights init_state_dict(spec, seed=0), as bench.py builds them).

    defect: "ignore_reset_row"      row `defect_row` keeps its state where its reset mask is set (after the first step);
            "stale_rtg"             every step embeds the previous call's returns-to-go;
            "previous_ring_slot"    every step reads the previous call's observations (ring slot t - 1);
            "action_off_by_one_bin" on call `defect_call`, action dim 0 of row `defect_row` is one bin higher."""

    def __init__(self, spec, batch, device, defect=None, defect_row=0, defect_call=0):
        assert defect in DEFECTS, defect
        self.spec, self.batch, self.device = spec, batch, torch.device(device)
        self.sd = init_state_dict(spec, seed=0)
        self.ora = OraclePolicy(spec, self.sd)
        self.defect, self.defect_row, self.defect_call = defect, defect_row, defect_call
        self.state_mode = "materialised"
        self.calls, self._prev, self._dbg = 0, None, None

    def set_micro_batches(self, n):
        pass

    def set_graph_mode(self, on):
        pass

    def reset(self, env_mask=None):
        if self.ora.state is None:
            return
        m = torch.ones(self.batch, dtype=torch.uint8) if env_mask is None else torch.as_tensor(env_mask).cpu()
        from oracle import mamba_ref, xlstm_ref
        mod = mamba_ref if self.spec.backbone == "mamba" else xlstm_ref
        self.ora.state = mod.reset_state_rows(self.ora.state, m.bool())

    def step(self, obs, rtg, reward, reset_mask=None, discrete=False, obs_is_embedding=False, **kw):
        assert not obs_is_embedding
        obs, rtg, reward = obs.cpu().clone(), rtg.cpu().clone(), reward.cpu().clone()
        mask = None if reset_mask is None else reset_mask.cpu().clone()
        use_obs, use_rtg = obs, rtg
        if self._prev is not None and self.defect == "stale_rtg":
            use_rtg = self._prev[1]
        if self._prev is not None and self.defect == "previous_ring_slot":
            use_obs = self._prev[0]
        self._prev = (obs, rtg)
        if mask is not None and self.defect == "ignore_reset_row" and self.calls > 0:
            mask[self.defect_row] = 0
        a, self._dbg = self.ora.step(use_obs, use_rtg, reward, mask, discrete=discrete, return_debug=True)
        lg = self._dbg["logits"]
        tok = (lg.argmax(-1) if not discrete else lg[:, 0, : self.spec.n_discrete].argmax(-1, keepdim=True)).to(torch.int32)
        if discrete:   # (column 0 holds the action, as on the engine)
            a = torch.zeros(self.batch, self.spec.act_dim).index_copy_(1, torch.tensor([0]), a.float())
            tok = torch.zeros(self.batch, self.spec.act_dim, dtype=torch.int32).index_copy_(1, torch.tensor([0]), tok)
        if self.defect == "action_off_by_one_bin" and self.calls == self.defect_call:
            tok[self.defect_row, 0] += 1
            a[self.defect_row, 0] = minmax_inv_tokenize(tok[self.defect_row, 0].long(), self.spec.action_channels,
                                                        self.spec.n_discrete)
        self.calls += 1
        return a.to(self.device), tok.to(self.device)

    def taps(self):
        return self._dbg["tokens"], self._dbg["hidden"], self._dbg["logits"].reshape(self.batch, -1)

    def _state_tensor(self, block, which):
        s = self.ora.state
        if self.spec.backbone == "mamba":
            return s[block][{3: 0, 0: 1}[which]]
        b = s[f"block_{block}"]
        if block in self.spec.slstm_at:
            return b["slstm_state"] if which == 0 else b["conv_state"][0]
        return b["mlstm_state"][which] if which < 3 else b["conv_state"][0]

    def export_state_tensor(self, block, which):
        return self._state_tensor(block, which).clone()

    def import_state_tensor(self, block, which, t):
        self._state_tensor(block, which).copy_(t)

    def close(self):
        pass


class RecordingOracleEngine(RecordingMixin, OracleEngine):
    def __init__(self, spec, batch, device, **kw):
        super().__init__(spec, batch, device, **kw)
        self._rec_start(spec, batch, self.sd, self.device)

    def close(self):
        self._rec_finish()
        super().close()


def recording_factory(session, **kw):
    """An engine_factory(spec, batch, device) for bench.main that builds RecordingOracleEngine into `session`."""
    cls = type("RecordingOracleEngine", (RecordingOracleEngine,), {"session": session})
    return lambda spec, batch, device: cls(spec, batch, device, **kw)
