"""Record what bench.py hands its engines, call for call, and replay it through the CPU oracle.  TEST INFRASTRUCTURE.

`RecordingEngine` is lram_amd.engine.Engine with a recorder in front of every call that consumes inputs or changes the
recurrent state.  bench.main, step_leg and prefill_leg import `Engine` from lram_amd.engine inside the function, so

    monkeypatch.setattr("lram_amd.engine.Engine", recording_engine(session))

captures every engine the bench builds without touching bench.py.  Each call's inputs and outputs are cloned on the caller's
current stream at the moment of the call (the host-IO leg refills its input buffers in place and the observation rings repeat),
and only a fixed sample of env rows is kept.  close() exports the sampled rows' final state of every block (and the last
step's hidden tap) before the engine is destroyed.

`replay` runs one engine's record through OraclePolicy in fp32 -- and, where the final hidden tap needs it, through
tests.helpers.Fp64Oracle -- in the recorded call order, and holds every call's actions and token ids, the final hidden tap
and the final state to the bars of the oracle parity tests.  A recorded call it does not model fails the replay."""
import torch

from lram_amd import init_state_dict
from lram_amd.engine import Engine
from oracle import mamba_ref, xlstm_ref
from oracle.dt_ref import OraclePolicy
from tests.helpers import (Fp64Oracle, assert_actions_match, assert_close_or_as_close_as_fp32_oracle, relaxed_rows_fraction,
                           relaxed_rows_reset, state_vs_oracle)

GAP_TOL = 2e-4      # the oracle's top-2 logit margin below which a differing argmax is a numerical tie (assert_actions_match)
RELAXED_MAX = 0.05  # share of the hidden tap's rows that may need the float64 rule


class ReplayError(AssertionError):
    pass


def slice_bounds(spec, batch, micro, graph):
    """[(first, end)] of the env slices one engine call runs, by the rule of make_slices (lram_amd/csrc/engine_streams.hip): n = the
    lram_set_micro_batches value, 0 = auto = two slices where one mLSTM block's matrix memory over the batch (B x n_heads x
    head_dim^2 x 4 bytes) is at least 512 MiB (xLSTM) or from 1024 env slots (Mamba), else one; graph mode always one; n is
    clamped to [1, min(B, 8)]; slices of B / n rows each, the first B % n of them one row more."""
    n = micro
    if n == 0:
        if spec.backbone == "mamba":
            n = 2 if batch >= 1024 else 1
        else:
            n = 2 if batch * spec.n_heads * spec.head_dim ** 2 * 4 >= 512 * 1024 ** 2 else 1
    if graph:
        n = 1
    n = max(1, min(n, batch, 8))
    base, rem = divmod(batch, n)
    out, b0 = [], 0
    for i in range(n):
        nb = base + (1 if i < rem else 0)
        out.append((b0, b0 + nb))
        b0 += nb
    return out


def slice_ends(spec, batch, micro, graph):
    return {r for lo, hi in slice_bounds(spec, batch, micro, graph) for r in (lo, hi - 1)}


def bench_rows(spec, batch, ep_len, window, micro=(0, 1), graph=False):
    """The row sample of one engine driven by a bench schedule (`phase = arange(B) % ep_len`, reset where the age is 0): rows 0
    and B - 1, both ends of every env slice of each lram_set_micro_batches value in `micro`, two rows whose reset falls inside
    the first `window` steps (at step ep_len - phase) where the batch has them, and one row that does not reset."""
    rows = {0, batch - 1}
    for m in micro:
        rows |= slice_ends(spec, batch, m, graph)
    for t in (max(1, window // 4), max(2, 3 * window // 4)):
        if t < window and ep_len - t < batch:        # phase ep_len - t resets at step t: in the first and the last episode block
            rows |= {ep_len - t, ep_len - t + (batch - 1 - (ep_len - t)) // ep_len * ep_len}
    quiet = batch // 3
    while quiet in rows or (quiet % ep_len) > ep_len - window:
        quiet += 1
    rows.add(quiet)
    return sorted(r for r in rows if 0 <= r < batch)


# ---- the recorder ---------------------------------------------------------------------------------------------------------
class Record:
    def __init__(self, label, spec, batch, rows, image, weights_sum):
        self.label, self.spec, self.batch, self.rows = label, spec, batch, list(rows)
        self.image, self.weights_sum = image, weights_sum
        self.calls = []          # {"kind", "args": {...}, "out": {...}}
        self.final_state = None  # {(block, which): tensor of the sampled rows}
        self.hidden = None       # the last step's hidden tap [n, T, D] (when the last call was a step)
        self.closed = False


class Session:
    """The records of every engine built while the recorder is installed.  rows_for(spec, batch) -> the row sample of an engine
    (all rows: list(range(batch)))."""

    def __init__(self, rows_for):
        self.rows_for = rows_for
        self.records = []

    def close_all(self):
        """Close what the caller left open (bench.main keeps its engine when it runs no config legs and no CPU baseline)."""
        for r in self.records:
            if not r.closed:
                r._engine.close()


# recorded calls the replayer models (encoder_step is recorded, but no bench path makes it: its replay fails)
MODELLED = ("step", "step_images", "embed_images", "prefill", "reset", "set_compat_mode", "set_state_mode", "set_micro_batches",
            "set_graph_mode")
# setters that change neither the recurrent state nor the last step's taps (the representation and the scheduling only)
PURE_SETTERS = ("set_state_mode", "set_micro_batches", "set_graph_mode")


def ends_with_a_step(calls):
    """Whether the last call that is not a pure setter is a step: then the engine's taps are that step's (bench.main's
    standalone sub-leg ends with set_micro_batches after its steps)."""
    rest = [c["kind"] for c in calls if c["kind"] not in PURE_SETTERS]
    return bool(rest) and rest[-1] in ("step", "step_images")


class RecordingMixin:
    """In front of an engine class: records every call that consumes inputs or changes the recurrent state.  The state-changing
    calls the replayer does not model (import_state_tensor, load_weights / alloc after construction) are recorded under their
    own name, so that the replay fails on them."""

    session = None   # the Session it records into (a subclass per session: recording_engine)
    _rec = None

    def _rec_start(self, spec, batch, sd_or_none, device):
        image = bool(sd_or_none) and any(k.startswith("embed_image.") for k in sd_or_none)
        wsum = None if sd_or_none is None else sum(float(v.double().sum()) for v in sd_or_none.values())
        rows = list(self.session.rows_for(spec, batch))
        assert rows == sorted(set(rows)) and 0 <= rows[0] and rows[-1] < batch, rows
        rec = Record(f"engine {len(self.session.records)} ({spec.backbone} d_model {spec.d_model}, {batch} envs)", spec,
                     batch, rows, image, wsum)
        rec._engine = self
        rec._idx = torch.as_tensor(rows, device=device)
        rec._full = len(rows) == batch
        rec._micro, rec._graph = 0, False
        self.session.records.append(rec)
        self._rec = rec

    # -- helpers --------------------------------------------------------------------------------------------------------
    def _rows(self, t, axis=0):
        if t is None:
            return None
        rec = self._rec
        if rec._full:
            return t.detach().clone()
        return t.detach().index_select(axis, rec._idx.to(t.device))

    def _log(self, kind, args, out=None):
        if self._rec is None:   # (the engine's own constructor)
            return
        self._rec.calls.append({"kind": kind, "args": args, "out": out or {}})

    def _slices_sampled(self):
        rec = self._rec
        if rec is None or rec._full:
            return
        ends = slice_ends(rec.spec, rec.batch, rec._micro, rec._graph)
        missing = ends - set(rec.rows)
        assert not missing, (f"{rec.label}: the row sample {rec.rows} lacks slice ends {sorted(missing)} of "
                             f"micro={rec._micro} graph={rec._graph}")

    # -- recorded calls -------------------------------------------------------------------------------------------------
    def step(self, obs, rtg, reward, reset_mask=None, discrete=False, obs_is_embedding=False, **kw):
        self._slices_sampled()
        args = {"obs": self._rows(obs), "rtg": self._rows(rtg), "reward": self._rows(reward),
                "mask": self._rows(reset_mask), "discrete": bool(discrete), "obs_is_embedding": bool(obs_is_embedding)}
        a, tok = super().step(obs, rtg, reward, reset_mask, discrete=discrete, obs_is_embedding=obs_is_embedding, **kw)
        self._log("step", args, {"actions": self._rows(a), "tokens": self._rows(tok)})
        return a, tok

    def step_images(self, images, rtg, reward, reset_mask=None, discrete=False, **kw):
        self._slices_sampled()
        args = {"obs": self._rows(images), "rtg": self._rows(rtg), "reward": self._rows(reward),
                "mask": self._rows(reset_mask), "discrete": bool(discrete), "obs_is_embedding": False}
        a, tok = super().step_images(images, rtg, reward, reset_mask, discrete=discrete, **kw)
        self._log("step_images", args, {"actions": self._rows(a), "tokens": self._rows(tok)})
        return a, tok

    def embed_images(self, images, out=None):
        self._slices_sampled()
        args = {"images": self._rows(images)}
        out = super().embed_images(images, out)
        self._log("embed_images", args, {"embedding": self._rows(out)})
        return out

    def prefill(self, obs_seq, rtg_seq, reward_seq, reset_mask=None, discrete=False, obs_is_embedding=False,
                want_action=True):
        args = {"obs": self._rows(obs_seq), "rtg": self._rows(rtg_seq), "reward": self._rows(reward_seq),
                "mask": self._rows(reset_mask), "discrete": bool(discrete), "obs_is_embedding": bool(obs_is_embedding),
                "want_action": bool(want_action)}
        a, tok = super().prefill(obs_seq, rtg_seq, reward_seq, reset_mask, discrete=discrete,
                                 obs_is_embedding=obs_is_embedding, want_action=want_action)
        self._log("prefill", args, {"actions": self._rows(a), "tokens": self._rows(tok)})
        return a, tok

    def encoder_step(self, inputs_embeds, reset_mask=None):
        self._slices_sampled()
        args = {"inputs_embeds": self._rows(inputs_embeds), "mask": self._rows(reset_mask)}
        out = super().encoder_step(inputs_embeds, reset_mask)
        self._log("encoder_step", args, {"hidden": self._rows(out)})
        return out

    def reset(self, env_mask=None):
        self._log("reset", {"mask": None if env_mask is None else self._rows(torch.as_tensor(env_mask))})
        return super().reset(env_mask)

    def set_compat_mode(self, mamba_repeat=1, stale_state=False):
        super().set_compat_mode(mamba_repeat, stale_state)
        self._log("set_compat_mode", {"mamba_repeat": int(mamba_repeat), "stale_state": bool(stale_state)})

    def set_state_mode(self, mode, fold_period=0):
        super().set_state_mode(mode, fold_period)
        self._log("set_state_mode", {"mode": mode, "fold_period": fold_period})

    def set_micro_batches(self, n):
        super().set_micro_batches(n)
        if self._rec is not None:
            self._rec._micro = int(n)
        self._log("set_micro_batches", {"n": int(n)})

    def set_graph_mode(self, enable):
        super().set_graph_mode(enable)
        if self._rec is not None:
            self._rec._graph = bool(enable)
        self._log("set_graph_mode", {"enable": bool(enable)})

    def import_state_tensor(self, block, which, t):
        self._log("import_state_tensor", {"block": block, "which": which})
        return super().import_state_tensor(block, which, t)

    def load_weights(self, state_dict):
        self._log("load_weights", {})
        return super().load_weights(state_dict)

    def alloc(self, batch):
        self._log("alloc", {"batch": int(batch)})
        return super().alloc(batch)

    # -- the end of the engine ------------------------------------------------------------------------------------------
    def _rec_finish(self):
        rec = self._rec
        if rec is None or rec.closed:
            return
        spec = rec.spec
        state = {}
        for i in range(spec.n_blocks):
            kinds = (0, 3) if (spec.backbone == "mamba" or i in spec.slstm_at) else (0, 1, 2, 3)
            for w in kinds:
                t = self.export_state_tensor(i, w)
                state[(i, w)] = self._rows(t, axis=1 if (spec.backbone == "xlstm" and i in spec.slstm_at and w == 0) else 0)
                del t
        rec.final_state = state
        if ends_with_a_step(rec.calls):
            rec.hidden = self._rows(self.taps()[1])
        rec.closed = True


class RecordingEngine(RecordingMixin, Engine):
    """lram_amd.engine.Engine under the recorder (see recording_engine for the session it records into)."""

    def __init__(self, spec, state_dict, batch, device=None):
        super().__init__(spec, state_dict, batch, device=device)
        self._rec_start(spec, batch, state_dict, self.device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._rec_finish()
            torch.cuda.synchronize(self.device)   # (the exports are enqueued; the engine's buffers go next)
        super().close()


def recording_engine(session):
    """A RecordingEngine class bound to `session` (monkeypatch it over lram_amd.engine.Engine)."""
    return type("RecordingEngine", (RecordingEngine,), {"session": session})


# ---- the replayer ---------------------------------------------------------------------------------------------------------
def _cpu(t):
    return None if t is None else t.detach().cpu()


def _oracle_reset(ora, mask):
    """What OraclePolicy.step does with a reset mask, alone (lram_reset; stale_state: layer 0 only)."""
    if ora.state is None or mask is None or not bool(mask.any()):
        return
    mod = mamba_ref if ora.spec.backbone == "mamba" else xlstm_ref
    if ora.stale_state:
        ora.state = {**ora.state, 0: mod.reset_state_rows({0: ora.state[0]}, mask.bool())[0]}
    else:
        ora.state = mod.reset_state_rows(ora.state, mask.bool())


class _Replay:
    def __init__(self, rec, sd, fp64):
        self.rec, self.spec, self.fp64 = rec, rec.spec, fp64
        self.o = Fp64Oracle(self.spec, sd) if fp64 else OraclePolicy(self.spec, sd)   # (state: zero until the first step)
        self.ties, self.hidden, self.embedded = 0, None, None

    @property
    def ora(self):
        return self.o.ora if self.fp64 else self.o

    def _dtype(self):
        return torch.float64 if self.fp64 else torch.get_default_dtype()

    def reset(self, mask):
        prev = torch.get_default_dtype()
        torch.set_default_dtype(self._dtype())
        try:
            _oracle_reset(self.ora, mask)
        finally:
            torch.set_default_dtype(prev)

    def check_outputs(self, i, kind, out, a_ref, logits, discrete):
        """Actions (tie rule) and token ids (wherever the oracle's margin is no tie) of call i, row by row."""
        rec, spec = self.rec, self.spec
        a_got, tok_got = _cpu(out.get("actions")), _cpu(out.get("tokens"))
        if a_got is None:
            return
        lg = logits.reshape(a_ref.shape[0], -1, spec.n_vocab)
        if discrete:
            a_got, tok_got = a_got[:, :1], tok_got[:, :1]
            lg_cmp = lg[:, :1, : spec.n_discrete]
        else:
            lg_cmp = lg
        top2 = lg_cmp.float().topk(2, dim=-1).values
        tie = (top2[..., 0] - top2[..., 1]) < GAP_TOL
        tok_ref = lg_cmp.argmax(-1)
        for j, row in enumerate(rec.rows):
            what = f"{rec.label}: call {i} ({kind}) row {row}"
            self.ties += assert_actions_match(a_got[j:j + 1], a_ref[j:j + 1].float(), lg[j:j + 1].float(), spec,
                                              discrete=discrete, gap_tol=GAP_TOL, what=what)
            bad = (tok_got[j].long() != tok_ref[j]) & ~tie[j]
            if bool(bad.any()):
                raise ReplayError(f"{what}: token ids {tok_got[j][bad].tolist()} where the oracle's are "
                                  f"{tok_ref[j][bad].tolist()} (action dims {bad.nonzero().view(-1).tolist()})")

    def one_step(self, obs, rtg, rew, mask, discrete):
        a, dbg = self.o.step(obs, rtg, rew, mask, discrete=discrete, return_debug=True)
        self.hidden = dbg["hidden"]
        return a, dbg["logits"]

    def run(self, check):
        rec = self.rec
        for i, c in enumerate(rec.calls):
            kind, args, out = c["kind"], c["args"], c["out"]
            if kind not in MODELLED:
                raise ReplayError(f"{rec.label}: call {i} ({kind}) changes the engine in a way the replayer does not model")
            if kind in ("set_state_mode", "set_micro_batches", "set_graph_mode"):
                continue    # representation / scheduling only: results do not depend on them
            if kind == "set_compat_mode":
                if rec.spec.backbone != "mamba" and (args["mamba_repeat"] != 1 or args["stale_state"]):
                    raise ReplayError(f"{rec.label}: call {i}: compat mode on an xLSTM engine")
                self.ora.mamba_repeat, self.ora.stale_state = args["mamba_repeat"], args["stale_state"]
                continue
            if kind == "reset":
                m = args["mask"]
                self.reset(torch.ones(len(rec.rows), dtype=torch.uint8) if m is None else _cpu(m))
                continue
            if kind == "embed_images":
                self.embedded = (_cpu(args["images"]), _cpu(out["embedding"]))
                continue
            obs, rtg, rew, mask = (_cpu(args[k]) for k in ("obs", "rtg", "reward", "mask"))
            discrete = args["discrete"]
            if args["obs_is_embedding"]:
                # the two-call image path: the embedding must be the one embed_images just produced for these frames
                if self.embedded is None or not torch.equal(self.embedded[1], obs):
                    raise ReplayError(f"{rec.label}: call {i}: a step on an embedding that no recorded embed_images made")
                obs = self.embedded[0]
            if kind in ("step", "step_images"):
                a_ref, logits = self.one_step(obs, rtg, rew, mask, discrete)
            else:   # prefill: L oracle steps, the reset mask before the first
                if self.ora.mamba_repeat != 1:
                    raise ReplayError(f"{rec.label}: call {i}: prefill in the repeated-forward mode is not modelled")
                for t in range(obs.shape[1]):
                    a_ref, logits = self.one_step(obs[:, t], rtg[:, t], rew[:, t], mask if t == 0 else None, discrete)
                if not args["want_action"]:
                    continue
            if check:
                self.check_outputs(i, kind, out, a_ref, logits, discrete)


def replay(rec, report=None):
    """Replay one engine's record through the oracle and assert it (module docstring).  Returns {"calls", "ties", "relaxed"};
    "relaxed" (the hidden tap's float64-rule row fraction) is None where no hidden tap was compared (a record that does not
    end with a step).  A record that ends with a step must hold the hidden tap."""
    spec = rec.spec
    assert rec.closed, f"{rec.label}: the engine was never closed, so its final state was never exported"
    sd = init_state_dict(spec, seed=0, with_image_encoder=rec.image)
    if rec.weights_sum is not None:   # the bench's weights, rebuilt: init_state_dict(spec, seed=0, with_image_encoder=...)
        wsum = sum(float(v.double().sum()) for v in sd.values())
        assert wsum == rec.weights_sum, f"{rec.label}: rebuilt weights differ from the engine's ({wsum} vs {rec.weights_sum})"
    r32 = _Replay(rec, sd, fp64=False)
    r32.run(check=True)
    relaxed_rows_reset()
    frac = None   # (no hidden tap compared: no float64-rule fraction either)
    if ends_with_a_step(rec.calls):
        assert rec.hidden is not None, f"{rec.label}: the record ends with a step but holds no hidden tap"
        got = _cpu(rec.hidden)
        try:   # fp32 oracle alone first: the float64 replay is needed only for rows outside the fixed tolerance
            assert_close_or_as_close_as_fp32_oracle(got, r32.hidden, r32.hidden, what=f"{rec.label}: final hidden tap")
        except AssertionError:
            relaxed_rows_reset()
            r64 = _Replay(rec, sd, fp64=True)
            r64.run(check=False)
            assert_close_or_as_close_as_fp32_oracle(got, r32.hidden, r64.hidden, what=f"{rec.label}: final hidden tap")
        frac = relaxed_rows_fraction()
        assert frac <= RELAXED_MAX, f"{rec.label}: {frac:.1%} of the hidden tap's rows needed the float64 rule"
    state = {k: _cpu(v) for k, v in rec.final_state.items()}
    last = len(rec.calls) - 1
    state_vs_oracle(lambda i, w: state[(i, w)], r32.ora.state, spec, f"{rec.label}: final state after call {last}",
                    rows=rec.rows)
    res = {"calls": len(rec.calls), "ties": r32.ties, "relaxed": frac}
    if report is not None:
        report(f"{rec.label}: {res['calls']} calls replayed over {len(rec.rows)} rows, ties {r32.ties}, "
               "float64-rule rows " + ("n/a (no hidden tap)" if frac is None else f"{frac:.2%}"))
    return res

