"""Rollout surface of the reference's recurrent agents on top of the HIP engine.

Keeps the attribute / method surface that `custom_evaluate_policy` touches on the agent
(src/callbacks/evaluation.py:97-129,134-139,238-251):

    predict(policy, observation, actions, rewards, returns_to_go, timesteps, state=None, episode_start=None,
            deterministic=True, context_len=5, prompt=None, task_id=None, is_eval=False, env_act_dim=None)
                                                   (src/algos/decision_transformer_sb3.py:621-667)
    get_action_pred(policy, states, actions, rewards, returns_to_go, timesteps, attention_mask,
                    deterministic, prompt, is_eval=False, task_id=None, env_act_dim=None)
                                                   (src/algos/discrete_decision_transformer_sb3.py:13-72,
                                                    src/algos/decision_mamba.py:76-127)
    get_action(...)  alias named by BASELINE.json's north_star
    attributes: policy, device, eval_context_len, use_inference_cache, past_key_values,
                inference_params.reset(), persist_context, compile, replay_buffer.{seqs_per_sample,
                max_state_dim, max_act_dim}, target_return_type, compute_target_return_val(),
                get_reward_scale_for_env()

The single-env methods are thin views (batch slot 0 of a B=1 engine, exactly the reference's operating
point); `predict_batch` is the native entry: one call advances all B envs by one timestep.
"""
from __future__ import annotations

import contextlib
import copy
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from .config import ModelSpec
from .engine import Engine, ScoreResult, check_context_lengths
from .rollout import SlotScheduler


SAMPLE_DEFAULTS = {"temperature": 1.0, "top_k": 0, "top_p": 0.5}   # sample_from_logits' own (model_utils.py:7)


def resolve_sample_kwargs(kwargs: Optional[dict], n_head: int) -> Optional[dict]:
    """`a_sample_kwargs` -> the settings the engine is armed with: None stays None (argmax); a dict -- `{}` included --
    is completed with the reference's defaults.  Unknown keys raise KeyError, values the head refuses ValueError
    (`n_head`: logits per row of the head in use)."""
    if kwargs is None:
        return None
    unknown = set(kwargs) - set(SAMPLE_DEFAULTS)
    if unknown:
        raise KeyError(f"unknown key(s) in a_sample_kwargs: {sorted(unknown)} (sample_from_logits takes "
                       f"{sorted(SAMPLE_DEFAULTS)})")
    out = {**SAMPLE_DEFAULTS, **kwargs}
    t, k, p = float(out["temperature"]), out["top_k"], float(out["top_p"])
    if not (t > 0.0 and t < float("inf")):
        raise ValueError(f"a_sample_kwargs.temperature must be finite and > 0 (it multiplies the logits), got {t}")
    if int(k) != k or not 0 <= int(k) <= n_head:
        raise ValueError(f"a_sample_kwargs.top_k must be an integer in 0 .. {n_head} (the head's logits per row), got {k}")
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"a_sample_kwargs.top_p must be in [0, 1], got {p}")
    return {"temperature": t, "top_k": int(k), "top_p": p}


class _InferenceParams:
    """Stand-in for the reference's InferenceParams (src/algos/decision_mamba.py:9-25): reset() clears the
    cache -- every layer by default; with the agent's `compat_stale_state` only layer 0, as the reference does
    (SURVEY.md 3.5 Q1)."""

    def __init__(self, agent: "RecurrentAgent"):
        self._agent = agent
        self.seqlen_offset = 0

    def reset(self):
        self.seqlen_offset = 0
        self._agent.engine.reset()


def _take(x, envs, n_envs: int, name: str):
    """The entries of a full-width host control array (one per env, or None) that belong to `envs`, in that order."""
    if x is None:
        return None
    x = x.reshape(-1).tolist() if torch.is_tensor(x) else list(x)
    if len(x) != n_envs:
        raise ValueError(f"{name}: expected {n_envs} entries (one per env), got {len(x)}")
    return [x[e] for e in envs]


class RecurrentAgent:
    def __init__(self, spec: ModelSpec, state_dict: Dict[str, torch.Tensor], n_envs: int = 1, device=None,
                 discrete: bool = False, state_mean: Optional[torch.Tensor] = None,
                 state_std: Optional[torch.Tensor] = None, target_return: float = 0.0, reward_scale: float = 1.0,
                 graph: bool = False, reprime_context: bool = False, persist_context: bool = False,
                 compat_mamba_repeat: bool = False,
                 compat_stale_state: bool = False,
                 a_sample_kwargs: Optional[dict] = None, sample_seed: int = 0, sample_slot_base: int = 0,
                 slot_table=None, use_inference_cache: Optional[bool] = None, eval_context_len: Optional[int] = None,
                 window_slots: str = "shared"):
        self.spec = spec
        # slot_table (lram_amd.domains.SlotTable): the batch holds envs of several domains -- head mode, action dims and
        # observation kind per env slot (the reference passes `env_act_dim` / `is_discrete` per call for its one env,
        # src/callbacks/evaluation.py:90-138).  predict_batch then takes (vector_obs, images) and every slot gets its own head.
        self.slot_table = slot_table
        if slot_table is not None:
            if slot_table.n_slots != n_envs:
                raise ValueError(f"slot_table lays out {slot_table.n_slots} env slots, the agent has n_envs = {n_envs}")
            if int(slot_table.act_dim.max()) > spec.act_dim:
                raise ValueError(f"slot_table: a domain uses {int(slot_table.act_dim.max())} action dims, the model has {spec.act_dim}")
            if compat_mamba_repeat:
                raise ValueError("compat_mamba_repeat advances the state once per action dim of the env; that differs per "
                                 "slot of a mixed batch and cannot be combined with slot_table")
            discrete = False
        # a_sample_kwargs (src/algos/discrete_decision_transformer_sb3.py:8-11): None = argmax actions, today's behaviour;
        # a dict = actions drawn on the device (Engine.set_sampling), with sample_from_logits' keyword names and defaults
        # (src/algos/models/model_utils.py:7).  `deterministic` is accepted and ignored by predict / get_action_pred, as in
        # the reference, where a_sample_kwargs alone decides.
        # Not given here: what the configuration set (agent_params.a_sample_kwargs -> ModelSpec.a_sample_kwargs; no preset does).
        if a_sample_kwargs is None:
            a_sample_kwargs = spec.a_sample_kwargs
        # With a slot table the agent-level setting is checked against the head of every domain that falls back on it (a
        # domain with its own Domain.a_sample_kwargs is checked against its own head), so a discrete domain in the table no
        # longer caps the top_k of the continuous ones.
        if slot_table is None:
            self.a_sample_kwargs = resolve_sample_kwargs(a_sample_kwargs, spec.n_discrete if discrete else spec.n_vocab)
        else:
            self.a_sample_kwargs = resolve_sample_kwargs(a_sample_kwargs, spec.n_vocab)
            slot_table.sample_settings(spec.n_discrete, spec.n_vocab, a_sample_kwargs)   # (raises what the head would refuse)
        self.sample_seed, self.sample_slot_base = int(sample_seed), int(sample_slot_base)
        self._slot_sampling = {}   # set_slot_sampling: slot -> resolved dict | "greedy" (plain data: crosses a pickle)
        self._slot_actions = {}    # set_slot_actions: slot -> tuple of allowed indices (plain data too)
        if slot_table is not None:
            slot_table.action_mask(spec.n_vocab, spec.n_discrete)   # (raises where a domain's set leaves its head's range)
        # host copy of the weights: lets the agent cross a process boundary (make_pickleable / reinit_cuda_kernels)
        self._state_dict = {k: v.detach().to("cpu") for k, v in state_dict.items()}
        self._graph = bool(graph)
        self.engine = Engine(spec, state_dict, n_envs, device)
        self.device = self.engine.device
        self.n_envs = n_envs
        self.is_discrete = bool(discrete)
        self.policy = self  # `model.predict(model.policy, ...)`: the policy argument is accepted and ignored
        self.state_mean = None if state_mean is None else state_mean.to(self.device, torch.float32)
        self.state_std = None if state_std is None else state_std.to(self.device, torch.float32)
        # image observations go through the engine's own IMPALA-CNN kernels (lram_embed_images): one backend in the package
        # (the PyTorch / MIOpen module that cross-checks them lives with the tests: tests/torch_image_encoder.py)
        self.has_image_encoder = any(k.startswith("embed_image.") for k in state_dict) and spec.image_shape is not None
        # attributes read by the evaluation loop
        self.eval_context_len = spec.max_length if eval_context_len is None else int(eval_context_len)
        # True: the recurrent state is stepped forever (the reference's cached path).  False -- the reference's default and what
        # its shipped configs run: every env-step runs the model from an empty state over the env's last eval_context_len
        # timesteps (Engine.step_window; decision_transformer_sb3.py:621-691).  See predict_batch.  Not given here: what the
        # configuration set (agent_params.use_inference_cache -> ModelSpec.use_inference_cache; every preset says True).
        self.use_inference_cache = bool(spec.use_inference_cache if use_inference_cache is None else use_inference_cache)
        # Window mode only.  "shared" (default): every env is stepped in every call, and set_active / fork_slots / save_slots /
        # load_slots refuse.  "own": every slot's window has its own ring position (Engine.set_window_slots), so envs can be
        # parked and windows forked, saved and loaded with their slots.
        if window_slots not in ("shared", "own"):
            raise ValueError(f'window_slots: unknown mode {window_slots!r} (choose "shared" or "own")')
        if window_slots == "own" and self.use_inference_cache:
            raise ValueError('window_slots="own" belongs to use_inference_cache=False (context-window inference)')
        self.window_slots = window_slots
        self.reset_inf_cache_freq = spec.reset_inf_cache_freq
        # reference behaviour (False): the context is dropped when the cache is reset;
        # True: the last eval_context_len stored timesteps are fed back through Engine.prefill
        self.reprime_context = bool(reprime_context)
        # evaluation.py:213-236: keep the context (here: the recurrent cache) across episode ends
        self.persist_context = bool(persist_context)
        self.compile = False
        self.target_return_type = "predefined"
        self.target_return = float(target_return) / float(reward_scale)
        self.reward_scale = float(reward_scale)
        self.replay_buffer = SimpleNamespace(seqs_per_sample=1, max_state_dim=spec.state_dim, max_act_dim=spec.act_dim)
        self.inference_params = _InferenceParams(self)
        self.inf_dummy_batch_size = None
        if graph:
            self.engine.set_graph_mode(True)
        self._zero_reward = torch.zeros(n_envs, dtype=torch.float32, device=self.device)
        self.scheduler = SlotScheduler(n_envs)   # env id <-> engine slot while envs are parked (set_active)
        # Reference-trajectory modes of the Mamba agent (lram_set_compat_mode).  Off: one state
        # advance per env-step and a reset empties every layer.  On: the trajectory the reference's
        # DiscreteDecisionMamba.get_action_pred / InferenceParams.reset() actually produce.
        if (compat_mamba_repeat or compat_stale_state) and spec.backbone != "mamba":
            raise ValueError("compat_mamba_repeat / compat_stale_state reproduce quirks of the reference's Mamba agent "
                             "(src/algos/decision_mamba.py); the xLSTM agent has neither")
        self.compat_mamba_repeat = bool(compat_mamba_repeat)
        self.compat_stale_state = bool(compat_stale_state)
        self._compat_repeat_now = 1
        if self.compat_stale_state:
            self.engine.set_compat_mode(1, True)
        self._arm_sampling()
        self._apply_slot_table()
        self._alloc_window()

    def _window_kind(self) -> Optional[str]:
        """None with the inference cache on; else what every slot's observation is in window mode: "vector" or "image".
        A slot table is refused in this mode (ValueError): one that mixes vector and image slots cannot be served -- the ring
        has one front end for the batch -- and per-slot heads over the ring are not wired yet."""
        if getattr(self, "use_inference_cache", True):
            return None
        if getattr(self, "slot_table", None) is not None:
            raise ValueError("use_inference_cache=False: slot tables are not served in context-window mode (one that mixes "
                             "vector and image slots cannot be: the ring has one front end for the batch)")
        return "image" if self.has_image_encoder else "vector"

    def _alloc_window(self):
        """Window mode: the ring of eval_context_len timesteps per env and the pad entry -- the reference pads the states with
        zeros BEFORE it normalises them (pad_inputs, then (s - mean) / std), so the pad observation is (0 - state_mean) /
        state_std through _prepare_obs; an image agent's is the embedding of an all-zero frame."""
        kind = self._window_kind()
        if kind is None:
            return
        if self.compat_mamba_repeat or self.compat_stale_state:
            raise ValueError("use_inference_cache=False: compat_mamba_repeat / compat_stale_state describe the cached path")
        if self.eval_context_len < 1:
            raise ValueError(f"use_inference_cache=False: eval_context_len must be >= 1, got {self.eval_context_len}")
        self.engine.alloc_window(self.eval_context_len)
        if kind == "image":
            frame = torch.zeros(self.n_envs, *self.spec.image_shape, dtype=torch.uint8, device=self.device)
            self.engine.set_window_pad(self.engine.embed_images(frame)[0].clone(), is_embedding=True)
        else:
            pad, _ = self._prepare_obs(torch.zeros(1, self.spec.state_dim, device=self.device))
            self.engine.set_window_pad(pad[0])
        if getattr(self, "window_slots", "shared") == "own":
            self.engine.set_window_slots("own")

    def _apply_slot_table(self):
        if getattr(self, "slot_table", None) is not None:
            self.engine.set_slot_table(*self.slot_table.engine_arrays())
        mask = self.slot_action_mask()
        if mask is not None:   # (the table's sets, then set_slot_actions'; an engine without one is never asked)
            self.engine.set_action_mask(mask)

    def slot_action_mask(self) -> Optional[torch.Tensor]:
        """The allowed sets the engine is given (Engine.set_action_mask's argument), bool [n_envs, n_vocab], or None where
        every slot may take everything: the domains' own sets (SlotTable.action_mask), then set_slot_actions'."""
        table = getattr(self, "slot_table", None)
        own = getattr(self, "_slot_actions", {})
        mask = None if table is None else table.action_mask(self.spec.n_vocab, self.spec.n_discrete)
        if mask is None:
            if not own:
                return None
            mask = torch.ones(self.n_envs, self.spec.n_vocab, dtype=torch.bool)
        for b, acts in own.items():
            mask[b] = False
            mask[b, list(acts)] = True
        return mask

    def set_slot_actions(self, slots, allowed):
        """The allowed set of single env slots, with or without a slot table -- an Atari game on its minimal action set beside
        games on the full one.  `allowed`: indices (actions below n_discrete on a discrete slot, vocabulary tokens otherwise;
        unique, non-empty), for every slot in `slots`; None gives the slots back their domain's set, or everything.  The sets
        stay with the slot index, like the slot's sampling setting."""
        slots = [int(b) for b in (slots.tolist() if isinstance(slots, torch.Tensor) else slots)]
        acts = None
        if allowed is not None:
            acts = [a for a in (allowed.tolist() if isinstance(allowed, torch.Tensor) else allowed)]
            if not acts or any(isinstance(a, bool) or int(a) != a or a < 0 for a in acts) or len(set(acts)) != len(acts):
                raise ValueError(f"set_slot_actions: expected distinct indices >= 0 (at least one), got {acts}")
            acts = tuple(int(a) for a in acts)
        new = dict(self._slot_actions)
        for b in slots:
            if not 0 <= b < self.n_envs:
                raise IndexError(f"set_slot_actions: slot {b} outside 0 .. {self.n_envs - 1}")
            if acts is None:
                new.pop(b, None)
                continue
            if max(acts) >= self._head_width(b):
                raise ValueError(f"set_slot_actions: slot {b} selects among {self._head_width(b)} logits, got index {max(acts)}")
            new[b] = acts
        had, old = self.slot_action_mask() is not None, self._slot_actions
        self._slot_actions = new
        if self.engine is None:
            return
        mask = self.slot_action_mask()
        if mask is not None or had:
            try:
                self.engine.set_action_mask(mask)
            except Exception:
                self._slot_actions = old   # a refused mask leaves the engine's as it was: so does the agent's record
                raise

    @property
    def slot_is_discrete(self) -> torch.Tensor:
        """bool [n_envs]: which env slots read the discrete head (every slot, or none, without a slot table)."""
        if getattr(self, "slot_table", None) is not None:
            return self.slot_table.discrete.clone()
        return torch.full((self.n_envs,), self.is_discrete, dtype=torch.bool)

    def _head_width(self, slot: int) -> int:
        return self.spec.n_discrete if bool(self.slot_is_discrete[slot]) else self.spec.n_vocab

    def slot_sample_settings(self) -> Optional[dict]:
        """The per-slot table the engine is given (Engine.set_sampling_slots' arguments), or None where the agent-level
        setting serves every slot: the domains' own settings (SlotTable.sample_settings), then set_slot_sampling's.  A slot
        with no setting of its own, of its domain or of the agent is greedy."""
        table = getattr(self, "slot_table", None)
        own = getattr(self, "_slot_sampling", {})
        cols = None if table is None else table.sample_settings(self.spec.n_discrete, self.spec.n_vocab, self.a_sample_kwargs)
        if cols is None:
            if not own:
                return None
            base = self.a_sample_kwargs
            cols = {"temperature": torch.full((self.n_envs,), 1.0 if base is None else base["temperature"], dtype=torch.float64),
                    "top_k": torch.full((self.n_envs,), 0 if base is None else base["top_k"], dtype=torch.int32),
                    "top_p": torch.full((self.n_envs,), 0.0 if base is None else base["top_p"], dtype=torch.float64),
                    "greedy": torch.full((self.n_envs,), base is None, dtype=torch.bool)}
        for b, s in own.items():
            cols["greedy"][b] = s == "greedy"
            if s != "greedy":
                cols["temperature"][b], cols["top_k"][b], cols["top_p"][b] = s["temperature"], s["top_k"], s["top_p"]
        return cols

    def _arm_sampling(self):
        cols = self.slot_sample_settings()
        if self.a_sample_kwargs is not None:
            self.engine.set_sampling(seed=self.sample_seed, slot_base=self.sample_slot_base, **self.a_sample_kwargs)
        elif cols is not None and not bool(cols["greedy"].all()):
            # only slots / domains sample: the engine-wide settings are placeholders the table overrides on every slot
            self.engine.set_sampling(temperature=1.0, top_k=0, top_p=0.0, seed=self.sample_seed, slot_base=self.sample_slot_base)
        else:
            return
        if cols is not None:
            self.engine.set_sampling_slots(temperature=cols["temperature"], top_k=cols["top_k"], top_p=cols["top_p"],
                                           greedy=cols["greedy"])

    def set_slot_sampling(self, slots, setting):
        """Sampling settings of single env slots, with or without a slot table -- a temperature ladder over the forks of one
        context (fork_slots), greedy evaluation slots beside exploring ones.  `setting`: a dict of sample_from_logits'
        keywords (completed with its defaults, checked against the slot's own head width), "greedy", or None (back to the
        slot's domain / the agent's setting); one for all `slots`, or a sequence with one entry per slot.  Seed, slot_base and
        the draw count are kept while sampling is armed; the first sampled slot of an agent that took the argmax everywhere
        arms it (draw count 0)."""
        slots = [int(b) for b in (slots.tolist() if isinstance(slots, torch.Tensor) else slots)]
        one = setting is None or isinstance(setting, (dict, str))
        settings = [setting] * len(slots) if one else list(setting)
        if len(settings) != len(slots):
            raise ValueError(f"set_slot_sampling: {len(slots)} slots and {len(settings)} settings")
        new = dict(self._slot_sampling)
        for b, s in zip(slots, settings):
            if not 0 <= b < self.n_envs:
                raise IndexError(f"set_slot_sampling: slot {b} outside 0 .. {self.n_envs - 1}")
            if s is None:
                new.pop(b, None)
            elif isinstance(s, str):
                if s != "greedy":
                    raise ValueError(f"set_slot_sampling: expected a dict, \"greedy\" or None, got {s!r}")
                new[b] = "greedy"
            else:
                new[b] = resolve_sample_kwargs(s, self._head_width(b))
        was_armed = self._sampling_armed()
        self._slot_sampling = new
        if self.engine is None:
            return
        cols = self.slot_sample_settings()
        if not was_armed or not self._sampling_armed():
            if was_armed:
                self.engine.set_sampling(None)
            self._arm_sampling()
        elif cols is None:
            self.engine.set_sampling_slots(None)
        else:
            self.engine.set_sampling_slots(temperature=cols["temperature"], top_k=cols["top_k"], top_p=cols["top_p"],
                                           greedy=cols["greedy"])

    def _sampling_armed(self) -> bool:
        if self.a_sample_kwargs is not None:
            return True
        cols = self.slot_sample_settings()
        return cols is not None and not bool(cols["greedy"].all())

    @property
    def trajectory_mode(self) -> dict:
        """Which trajectory semantics the rollout uses (logged by rollout / bench)."""
        mode = {"compat_mamba_repeat": self.compat_mamba_repeat, "compat_stale_state": self.compat_stale_state}
        if getattr(self, "a_sample_kwargs", None) is not None:   # (argmax actions: the record stays as it always was)
            mode["a_sample_kwargs"] = dict(self.a_sample_kwargs, seed=self.sample_seed, slot_base=self.sample_slot_base)
        cols = self.slot_sample_settings() if hasattr(self, "_slot_sampling") else None
        if cols is not None:
            # per distinct setting, the slot ranges that hold it: a domain is one entry, a ladder one entry per rung
            groups = {}
            for b in range(self.n_envs):
                key = ("greedy",) if bool(cols["greedy"][b]) else (float(cols["temperature"][b]), int(cols["top_k"][b]),
                                                                   float(cols["top_p"][b]))
                runs = groups.setdefault(key, [])
                if runs and runs[-1][1] == b:
                    runs[-1][1] = b + 1
                else:
                    runs.append([b, b + 1])
            mode["a_sample_slots"] = [
                {"slots": [tuple(r) for r in runs],
                 "setting": "greedy" if key == ("greedy",) else {"temperature": key[0], "top_k": key[1], "top_p": key[2]}}
                for key, runs in groups.items()]
            if "a_sample_kwargs" not in mode and self._sampling_armed():
                mode["a_sample_kwargs"] = {"seed": self.sample_seed, "slot_base": self.sample_slot_base}
        mask = self.slot_action_mask() if hasattr(self, "_slot_actions") else None
        if mask is not None:   # per distinct allowed set, the slot ranges that hold it (a set that allows everything: "all")
            groups = {}
            for b in range(self.n_envs):
                key = tuple(torch.nonzero(mask[b]).reshape(-1).tolist())
                runs = groups.setdefault(key, [])
                if runs and runs[-1][1] == b:
                    runs[-1][1] = b + 1
                else:
                    runs.append([b, b + 1])
            mode["a_allowed"] = [{"slots": [tuple(r) for r in runs],
                                  "allowed": "all" if len(key) == self.spec.n_vocab else list(key)}
                                 for key, runs in groups.items()]
        return mode

    # ---- cache handle: `model.past_key_values = None` resets, reading exports the reference layout ----
    @property
    def past_key_values(self):
        return self.engine.export_past_key_values()

    @past_key_values.setter
    def past_key_values(self, value):
        if value is None:
            self.engine.reset()
        else:
            self.engine.import_past_key_values(value)

    # ---- per-slot cache handle: fork / snapshot / restore single env slots (n_envs > 1) ----
    def _own_windows(self) -> bool:
        """Window mode with window_slots="own": an env's context is its window, and it moves with the slot."""
        return not getattr(self, "use_inference_cache", True) and getattr(self, "window_slots", "shared") == "own"

    def _need_batch(self, what: str):
        if not getattr(self, "use_inference_cache", True) and not self._own_windows():
            raise RuntimeError(f"{what}() moves the recurrent state of env slots; with use_inference_cache=False an env's context "
                               f"is its window on the device ring, which these calls do not move")
        if self.n_envs <= 1:
            raise RuntimeError(f"{what}() moves state between env slots of a batched agent; this agent has n_envs = 1 "
                               f"(use past_key_values for its one env)")

    def fork_slots(self, src, dst):
        """Slot dst[i] continues from slot src[i]'s context (Engine.copy_slots): the recurrent state is copied, nothing else of
        the batch is touched.  With a_sample_kwargs the forked slots draw independent continuations (the sampling stream belongs
        to the slot index); slot-table entries are not moved, so fork within one domain.
        use_inference_cache=False with window_slots="own": fork_slots / save_slots / load_slots address the slots' WINDOWS
        (Engine.copy_window_slots / save_window_slots / load_window_slots) -- there the window is the context."""
        self._need_batch("fork_slots")
        if self._own_windows():   # (the context is the window: every step restarts the recurrent state from it)
            return self.engine.copy_window_slots(src, dst)
        self.engine.copy_slots(src, dst)

    def save_slots(self, slots) -> torch.Tensor:
        """float32 [n, engine.slot_state_numel] records of the listed slots (Engine.save_slots): a per-env checkpoint."""
        self._need_batch("save_slots")
        if self._own_windows():   # float32 [n, engine.window_slot_numel]: the windows, position-free
            return self.engine.save_window_slots(slots)
        return self.engine.save_slots(slots)

    def load_slots(self, slots, records: torch.Tensor):
        """Restore records (save_slots of this or another agent of the same model) into the listed slots."""
        self._need_batch("load_slots")
        if self._own_windows():
            return self.engine.load_window_slots(slots, records)
        self.engine.load_slots(slots, records)

    # ---- parked envs: step only the envs that have something to do -------------------------------------
    @property
    def active(self):
        """Env ids the agent steps, in engine slot order (every env unless set_active parked some)."""
        sch = getattr(self, "scheduler", None)
        return list(range(self.n_envs)) if sch is None else sch.live_envs()

    def _slots_alike(self, a: int, b: int) -> Optional[str]:
        """None where slots a and b carry the same slot-table entry, per-slot sampling setting and allowed set, else what differs."""
        table = getattr(self, "slot_table", None)
        if table is not None:
            for name in ("discrete", "act_dim", "image"):
                col = getattr(table, name)
                if col[a] != col[b]:
                    return f"slot-table entry `{name}`"
        cols = self.slot_sample_settings()
        if cols is not None:
            for name, col in cols.items():
                if col[a] != col[b]:
                    return f"per-slot sampling setting `{name}`"
        if self._slot_allowed(a) != self._slot_allowed(b):
            return "allowed-action set"
        return None

    def _slot_allowed(self, b: int):
        """Slot b's allowed set as slot_action_mask() states it, without building the mask: a frozenset of indices, or None
        where the slot may take every token."""
        acts = getattr(self, "_slot_actions", {}).get(b)
        if acts is None and getattr(self, "slot_table", None) is not None:
            acts = self.slot_table.domain_of(b).allowed_actions
        if acts is None or len(set(acts)) == self.spec.n_vocab:
            return None
        return frozenset(acts)

    def set_active(self, env_ids):
        """The envs predict_batch steps from now on (at least one).  The others are parked: their recurrent state stays in the
        engine and a step costs them nothing (Engine.set_live); their rows of predict_batch's result hold 0.  The engine steps a
        prefix of its slots, so parking and resuming exchange the state of slot pairs (Engine.swap_slots; at most one swap per
        parked or resumed env, SlotScheduler).  Slot-table entries, per-slot sampling settings and the sampling stream stay
        with the slot index: a change that would exchange two slots whose entries differ is refused (ValueError) with nothing
        done.  fork_slots / save_slots / load_slots keep addressing engine SLOTS (scheduler.slot_of maps an env id).
        use_inference_cache=False: refused unless window_slots="own"; then every slot exchange also exchanges the windows
        (Engine.swap_window_slots), and a parked env saves the K-timestep prefill a window step would have cost it."""
        import copy
        want = [int(e) for e in env_ids]
        if len(set(want)) != len(want) or any(not 0 <= e < self.n_envs for e in want):
            raise ValueError(f"set_active: expected distinct env ids in 0 .. {self.n_envs - 1}")
        if not getattr(self, "use_inference_cache", True) and not self._own_windows() and len(want) != self.n_envs:
            raise ValueError("set_active: use_inference_cache=False steps every env slot (the window ring has one push "
                             "position for the batch); parked envs are refused in this mode")
        if not want:
            raise ValueError("set_active: at least one env must stay active")
        sch = copy.deepcopy(self.scheduler)
        now = set(sch.live_envs())
        calls = []
        # resume first: a change to a disjoint set (active {0} -> {1}) must not pass through an empty live set
        resume = sorted(set(want) - now)
        if resume:
            calls.append(sch.resume(resume))
        park = sorted(now - set(want))
        if park:
            calls.append(sch.park(park))
        for a, b, _ in calls:
            for sa, sb in zip(a, b):
                diff = self._slots_alike(sa, sb)
                if diff is not None:
                    raise ValueError(f"set_active: would exchange engine slots {sa} and {sb}, whose {diff} differs -- those stay "
                                     f"with the slot index (park envs of one domain and setting among themselves)")
        for a, b, n_live in calls:
            if a:
                self.engine.swap_slots(a, b)
                if self._own_windows():   # (an env's window goes where its state goes)
                    self.engine.swap_window_slots(a, b)
            self.engine.set_live(n_live)
        self.scheduler = sch

    def _live_index(self) -> Optional[torch.Tensor]:
        """Env id of every live slot as a device index, or None on today's path: every env active, identity permutation."""
        sch = getattr(self, "scheduler", None)
        if sch is None or (sch.n_live == sch.n and sch.identity):
            return None
        return torch.as_tensor(sch.live_envs(), dtype=torch.long, device=self.device)

    def _scatter_rows(self, rows: torch.Tensor, idx: torch.Tensor, fill=0) -> torch.Tensor:
        out = torch.full((self.n_envs, *rows.shape[1:]), fill, dtype=rows.dtype, device=rows.device)
        out[idx] = rows
        return out

    @contextlib.contextmanager
    def _context_envs(self, envs, lengths):
        """The stored-context calls on a subset of the envs (prime_contexts / extend_contexts / score_trajectories, `envs=`):
        brings the listed envs -- None: the active ones -- into a prefix of the engine's slots, makes that prefix the live one and
        the engine's context rows "started" or "live", and yields the env id of every row of the call in slot order (a device
        index); afterwards the slots, the live count and mode "all" are as before, so an env that was parked is parked again.
        With `lengths` the envs are sorted by descending length, which is what mode "started" asks for; where that would
        exchange two slots whose slot-table entry or per-slot sampling setting differs (_slots_alike) they keep the given order
        and the mode is "live".  Yields None, with nothing done, on today's path: envs=None, every env active in its own slot."""
        sch = self.scheduler
        if envs is None and sch.n_live == sch.n and sch.identity:
            yield None
            return
        part = sch.live_envs() if envs is None else [int(e) for e in envs]
        if not part or len(set(part)) != len(part) or any(not 0 <= e < self.n_envs for e in part):
            raise ValueError(f"envs: expected distinct env ids in 0 .. {self.n_envs - 1}, at least one")

        def plan(order):
            trial = copy.deepcopy(sch)
            lists = trial.arrange(order)
            for a, b in lists:
                for sa, sb in zip(a, b):
                    diff = self._slots_alike(sa, sb)
                    if diff is not None:
                        return None, (sa, sb, diff)
            return trial, lists

        trial, mode = None, "live"
        if lengths is not None:
            trial, lists = plan(sorted(part, key=lambda e: -int(lengths[e])))   # (stable: equal lengths keep their order)
            mode = "started" if trial is not None else "live"
        if trial is None:
            trial, lists = plan(part)
            if trial is None:
                sa, sb, diff = lists
                raise ValueError(f"envs: would exchange engine slots {sa} and {sb}, whose {diff} differs -- those stay with the "
                                 f"slot index (list envs of one domain and setting)")
        for a, b in lists:
            self.engine.swap_slots(a, b)
        trial.n_live = len(part)
        self.engine.set_live(len(part))
        self.engine.set_context_rows(mode)
        self.scheduler = trial
        try:
            yield torch.as_tensor(trial.live_envs(), dtype=torch.long, device=self.device)
        finally:
            self.engine.set_context_rows("all")
            for a, b in reversed(lists):   # (every list is an involution: the same lists in reverse order undo the arrangement)
                self.engine.swap_slots(a, b)
            self.engine.set_live(sch.n_live)
            self.scheduler = sch

    def _gather_contexts(self, idx, obs, frames, rtg, rew, lengths):
        """The rows of the prepared contexts (_prepare_contexts) that a call on the envs `idx` (slot order) hands the engine.
        With a slot table the frames are one row per image ENV in env-id order; the call takes those of the listed image envs."""
        take = (lambda t: None if t is None else t[idx].contiguous())
        envs = idx.tolist()
        table = getattr(self, "slot_table", None)
        if frames is not None and table is not None:
            rank, k = {}, 0
            for e in range(self.n_envs):
                if table.image[e]:
                    rank[e] = k
                    k += 1
            rows = [rank[e] for e in envs if e in rank]
            frames = frames[torch.as_tensor(rows, dtype=torch.long, device=frames.device)].contiguous() if rows else None
            if len(rows) == len(envs):
                obs = None   # (every listed env is an image env)
        elif frames is not None:
            frames = take(frames)
        return take(obs), frames, take(rtg), take(rew), None if lengths is None else [lengths[e] for e in envs]

    # ---- multiprocess evaluation (src/callbacks/custom_eval_callback.py:22-33, decision_xlstm.py:243-267) ----
    def make_pickleable(self, replace_cell: bool = False):
        """The native engine handle cannot be serialised: release it (spec and host weights stay), as the reference
        unsets its sLSTM CUDA kernels before handing the model to loky workers."""
        if self.engine is not None:
            self.engine.close()
            self.engine = None

    def reinit_cuda_kernels(self, replace_cell: bool = False):
        """Worker-side counterpart of make_pickleable: build a fresh engine (recurrent state starts empty; sampling is
        armed again with the same settings, the per-slot ones included, and its draw count restarts at 0)."""
        if self.engine is None:
            self.engine = Engine(self.spec, self._state_dict, self.n_envs, self.device)
            self.scheduler = SlotScheduler(self.n_envs)   # (fresh state: every env live, in its own slot)
            if self._graph:
                self.engine.set_graph_mode(True)
            if self.compat_stale_state or self._compat_repeat_now != 1:
                self.engine.set_compat_mode(self._compat_repeat_now, self.compat_stale_state)
            self._arm_sampling()
            self._apply_slot_table()
            self._alloc_window()

    def __getstate__(self):
        d = dict(self.__dict__)
        d["engine"] = None          # never pickled; reinit_cuda_kernels() rebuilds it
        d["policy"] = None          # self-reference, restored below
        d["inference_params"] = None
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self.policy = self
        self.inference_params = _InferenceParams(self)

    def compute_target_return_val(self, env=None, task_id=0):
        """Target return in model units (already divided by the reward scale).  With a slot table: of the domain `task_id`
        names -- a domain name or its position in the table (decision_transformer_sb3.py:542-559 looks it up per task)."""
        if getattr(self, "slot_table", None) is not None and task_id is not None:
            dom = self.slot_table.find(task_id)
            return float(dom.target_return) / float(dom.reward_scale)
        return self.target_return

    def get_reward_scale_for_env(self, envid=None):
        """With a slot table: the reward scale of the domain `envid` names (decision_transformer_sb3.py:373-382)."""
        if getattr(self, "slot_table", None) is not None and envid is not None:
            return float(self.slot_table.find(envid).reward_scale)
        return self.reward_scale

    # ---- native batched entry ---------------------------------------------------------------------
    def _prepare_obs(self, obs: torch.Tensor):
        """pad_inputs + normalisation (src/algos/decision_xlstm.py:11-28, decision_transformer_sb3.py:650-651)
        or the image encoder; returns (tensor, is_embedding)."""
        obs = obs.to(self.device)
        if obs.dim() == 4:
            if not self.has_image_encoder:
                raise RuntimeError("image observation given but the state dict has no embed_image.* weights")
            return self.engine.embed_images(obs.to(torch.uint8).contiguous()), True
        obs = obs.to(torch.float32)
        pad = self.spec.state_dim - obs.shape[-1]
        if pad < 0:
            raise ValueError(f"observation dim {obs.shape[-1]} exceeds max_state_dim {self.spec.state_dim}")
        if pad > 0:
            obs = torch.cat([obs, torch.zeros(*obs.shape[:-1], pad, device=self.device)], dim=-1)
        if self.state_mean is not None and self.state_std is not None:
            obs = (obs - self.state_mean) / self.state_std
        return obs.contiguous(), False

    @torch.no_grad()
    def predict_batch(self, observation: torch.Tensor, returns_to_go: torch.Tensor,
                      rewards: Optional[torch.Tensor] = None, reset_mask: Optional[torch.Tensor] = None,
                      env_act_dim: Optional[int] = None, prev_rewards: Optional[torch.Tensor] = None, relabel=None,
                      keep=None) -> torch.Tensor:
        """observation [B, obs_dim] (or uint8 [B,3,64,64]), returns_to_go [B] -> actions [B, env_act_dim]
        (float32; for discrete agents int64 [B, 1]).  The returned tensor is a view of an engine-owned
        buffer that the next call overwrites.
        With a slot table `observation` is the pair (vector_obs [B, obs_dim] or None, images uint8 [n_image, C, H, W] or None):
        rows of vector_obs that belong to image slots are never read, frame k belongs to the k-th image slot.  Returns float32
        [B, act_dim]: a continuous slot's action in the columns below its act_dim, a discrete slot's index in column 0 (exact in
        fp32), 0.0 elsewhere; `env_act_dim` is ignored.
        With parked envs (set_active) the tensors stay full-width in env-id order: the live rows are gathered in slot order,
        stepped, and the actions scattered back; the rows of parked envs hold 0 (then a fresh tensor, not an engine buffer), and
        their reset flags are not looked at.
        use_inference_cache=False (context-window inference, Engine.step_window): the model runs from an empty state over
        every env's last eval_context_len timesteps, left-padded as the reference pads them.  `prev_rewards` [B] is the scaled
        reward the PREVIOUS step earned (None: zeros) -- it becomes the reward of the newest stored timestep; `rewards` is not
        looked at (the current timestep's reward token is 0, evaluation.py:132).  `reset_mask[b]` empties env b's window;
        `relabel` / `keep` (host lists of B ints or None) are the episode-end bookkeeping of persist_context
        (evaluation.py:213-237): relabel = m rewrites the returns-to-go of the newest m timesteps to the returns obtained,
        keep = k prunes the window to its newest k timesteps.  Frames go through embed_images first.  A slot table -- one that
        mixes vector and image slots, or any other -- is refused in this mode (at construction), and so are parked envs
        (set_active) unless the agent was created with window_slots="own": then the tensors and the host lists stay
        full-width in env-id order, the live envs' entries are gathered into slot order, and the rows of parked envs hold 0."""
        if not getattr(self, "use_inference_cache", True):
            return self._predict_batch_window(observation, returns_to_go, reset_mask, env_act_dim, prev_rewards, relabel, keep)
        if prev_rewards is not None or relabel is not None or keep is not None:
            raise ValueError("prev_rewards / relabel / keep belong to use_inference_cache=False (context-window inference)")
        if getattr(self, "slot_table", None) is not None:
            return self._predict_batch_slots(observation, returns_to_go, rewards, reset_mask)
        idx = self._live_index()   # (None: every env active in its own slot -- no gather)
        if idx is not None:
            observation = observation.to(self.device)[idx]
            returns_to_go = returns_to_go.to(self.device).reshape(-1)[idx]
            rewards = None if rewards is None else rewards.to(self.device).reshape(-1)[idx]
            reset_mask = None if reset_mask is None else reset_mask.to(self.device).reshape(-1)[idx]
        images = observation.dim() == 4
        if images:   # frames go to the engine as they are: lram_step_images runs the CNN inside the step (per env slice)
            if not self.has_image_encoder:
                raise RuntimeError("image observation given but the state dict has no embed_image.* weights")
            obs, is_emb = observation.to(self.device).to(torch.uint8).contiguous(), True
        else:
            obs, is_emb = self._prepare_obs(observation)
        rtg = returns_to_go.to(self.device, torch.float32).reshape(-1).contiguous()
        rew = self._zero_reward[:rtg.shape[0]] if rewards is None else rewards.to(self.device, torch.float32).reshape(-1).contiguous()
        if reset_mask is not None:
            reset_mask = reset_mask.to(self.device, torch.uint8).contiguous()
        if getattr(self, "compat_mamba_repeat", False):
            # one forward per action dim of the env (decision_mamba.py:107: env_act_dim, else the padded action width)
            rep = 1 if self.is_discrete else int(self.spec.act_dim if env_act_dim is None else env_act_dim)
            if rep != self._compat_repeat_now:
                self.engine.set_compat_mode(rep, self.compat_stale_state)
                self._compat_repeat_now = rep
        if images:
            actions, _ = self.engine.step_images(obs, rtg, rew, reset_mask, discrete=self.is_discrete)
        else:
            actions, _ = self.engine.step(obs, rtg, rew, reset_mask, discrete=self.is_discrete, obs_is_embedding=is_emb)
        if idx is not None:   # back to env-id order; the rows of parked envs hold 0
            actions = self._scatter_rows(actions, idx)
        if self.is_discrete:
            return actions[:, :1].to(torch.int64)
        return actions if env_act_dim is None else actions[:, :env_act_dim]

    def _predict_batch_window(self, observation, returns_to_go, reset_mask, env_act_dim, prev_rewards, relabel, keep):
        if not torch.is_tensor(observation) or observation.shape[0] != self.n_envs:
            raise ValueError(f"observation: expected a tensor with one row per env slot ({self.n_envs})")
        obs, is_emb = self._prepare_obs(observation)   # (frames: embed_images, then embeddings)
        rtg = returns_to_go.to(self.device, torch.float32).reshape(-1).contiguous()
        prev = self._zero_reward if prev_rewards is None else prev_rewards.to(self.device, torch.float32).reshape(-1).contiguous()
        reset = None if reset_mask is None else [bool(v) for v in torch.as_tensor(reset_mask).reshape(-1).tolist()]
        idx = self._live_index() if self._own_windows() else None   # (None: every env active in its own slot -- no gather)
        if idx is not None:   # full-width arguments in env-id order -> the live slots' rows, in slot order
            envs = idx.tolist()
            obs, rtg, prev = obs[idx].contiguous(), rtg[idx].contiguous(), prev[idx].contiguous()
            reset, relabel, keep = (_take(x, envs, self.n_envs, name) for x, name in
                                    ((reset, "reset_mask"), (relabel, "relabel"), (keep, "keep")))
        actions, _ = self.engine.step_window(obs, rtg, prev, reset=reset, relabel=relabel, keep=keep, pad="reference",
                                             discrete=self.is_discrete, obs_is_embedding=is_emb)
        if idx is not None:   # back to env-id order; the rows of parked envs hold 0
            actions = self._scatter_rows(actions, idx)
        if self.is_discrete:
            return actions[:, :1].to(torch.int64)
        return actions if env_act_dim is None else actions[:, :env_act_dim]

    def _prepare_contexts(self, observations, returns_to_go, rewards, lengths):
        """What the stored-context calls share: observations [B, L, obs_dim] padded and normalised (_prepare_obs), returns_to_go
        and rewards (None: zeros) as float32 [B, L] on the device, `lengths` checked (check_context_lengths; None stays None)
        and the head mode the engine is to use.  Image observations: uint8 frames [B, L, C, H, W], or with a slot table the pair
        (vector_obs [B, L, obs_dim] or None, frames uint8 [n_image, L, C, H, W] in slot order), as predict_batch takes one
        timestep; the frames go to the engine as they are (Engine.prefill_frames / score_frames run the CNN inside the call).
        Returns (obs, frames, rtg, rew, lengths, discrete): frames None for vector observations; with frames, obs is the vector
        slots' rows or None."""
        B = self.n_envs
        table = getattr(self, "slot_table", None)
        frames = None
        if isinstance(observations, (tuple, list)):
            if table is None or len(observations) != 2:
                raise ValueError("observations: the pair (vector_obs, frames) goes with a slot table")
            observations, frames = observations
            if frames is None and table.n_image > 0:
                raise ValueError(f"frames: expected uint8 [{table.n_image}, L, C, H, W] (one row per image slot, in slot order)")
        elif observations.dim() == 5:
            if table is not None:
                raise ValueError("observations: with a slot table image contexts are the pair (vector_obs, frames)")
            observations, frames = None, observations
        if frames is not None:
            if not self.has_image_encoder:
                raise RuntimeError("image observation given but the state dict has no embed_image.* weights")
            n = B if table is None else table.n_image
            if frames.dim() != 5 or frames.shape[0] != n:
                raise ValueError(f"frames: expected uint8 [{n}, L, C, H, W], got {tuple(frames.shape)}")
            frames = frames.to(self.device).to(torch.uint8).contiguous()
            if table is not None and n == B:
                observations = None   # (every slot takes frames)
            elif table is not None and observations is None:
                raise ValueError("vector_obs: None is allowed only when every slot is an image slot")
        if frames is None and (observations.dim() != 3 or observations.shape[0] != B):
            raise ValueError(f"observations: expected [{B}, L, obs_dim], got {tuple(observations.shape)}")
        L = (observations if frames is None else frames).shape[1]
        obs = None
        if observations is not None:
            if observations.dim() != 3 or observations.shape[0] != B or observations.shape[1] != L:
                raise ValueError(f"vector_obs: expected [{B}, {L}, obs_dim], got {tuple(observations.shape)}")
            obs, _ = self._prepare_obs(observations.reshape(B * L, -1))
            obs = obs.view(B, L, -1).contiguous()
        if lengths is not None:
            lengths = check_context_lengths(torch.as_tensor(lengths).reshape(-1), B, L)
        rtg = returns_to_go.to(self.device, torch.float32).reshape(B, L).contiguous()
        rew = torch.zeros(B, L, dtype=torch.float32, device=self.device) if rewards is None else \
            rewards.to(self.device, torch.float32).reshape(B, L).contiguous()
        discrete = "per_slot" if getattr(self, "slot_table", None) is not None else self.is_discrete
        return obs, frames, rtg, rew, lengths, discrete

    def _engine_prefill(self, obs, frames, rtg, rew, **kw):
        if frames is None:
            return self.engine.prefill(obs, rtg, rew, **kw)
        return self.engine.prefill_frames(frames, rtg, rew, obs_seq=obs, **kw)

    def _engine_score(self, obs, frames, rtg, rew, lo=None, hi=None, **kw):
        """Engine.score / score_frames on the timesteps [lo, hi) of the prepared inputs (None: all)."""
        cut = (lambda t: t) if lo is None else (lambda t: None if t is None else t[:, lo:hi].contiguous())
        if frames is None:
            return self.engine.score(cut(obs), cut(rtg), cut(rew), **kw)
        return self.engine.score_frames(cut(frames), cut(rtg), cut(rew), obs_seq=cut(obs), **kw)

    # ---- grading: stored trajectories and the actions just taken --------------------------------------
    @torch.no_grad()
    def score_trajectories(self, observations: torch.Tensor, returns_to_go: torch.Tensor,
                           rewards: Optional[torch.Tensor] = None, actions: Optional[torch.Tensor] = None,
                           lengths: Optional[torch.Tensor] = None, reset: bool = True, over: str = "vocab",
                           temperature: float = 1.0, want=("actions", "tokens", "logp"), logits: bool = False,
                           window: Optional[int] = None, envs=None):
        """Grade stored trajectories (Engine.score): observations [B, L, obs_dim] -- padded and normalised with state_mean /
        state_std as predict_batch does -- returns_to_go [B, L] in model units, rewards [B, L] (None: the reference loop's
        zero reward token), recorded `actions` [B, L, n] (float; n <= act_dim, padded with zeros; a discrete agent's action
        index in column 0) and `lengths` [B] (timesteps that count per env, from the start; None = all L).  The lengths go
        to the engine (Engine.score(lengths=...)): rows beyond an env's length are masked and never read, and the state the call
        leaves is that of each env's own `lengths[b]` timesteps, so predict_batch can continue every env from there (an env of
        length 0 keeps the state it had).  reset=True starts every env from an empty context; a length in 1 .. L - 1 always does,
        so reset=False together with such a length raises ValueError.  Returns the ScoreResult (per-timestep greedy actions / tokens and the log-probability of the recorded
        actions); rollout.score_loss turns it into the reference's loss.  With a slot table every slot is scored with its
        own head.  Image observations: uint8 frames [B, L, C, H, W], or with a slot table the pair (vector_obs, frames
        [n_image, L, C, H, W]) as predict_batch takes one timestep (Engine.score_frames: padded frames are never convolved).
        `window=W` with W < L scores the trajectories in ceil(max(lengths) / W) calls (Engine.score(append=True)): call k covers
        rows [k W, (k + 1) W) with the lengths clamp(lengths[b] - k W, 0, W), every call continuing the state the one before left;
        `reset` is honoured on call 0 only.  The result is one ScoreResult of the full [B, L, ...] shape and the state afterwards
        that of each env's own timesteps, as for the single call (up to fp32 rounding: the chunks differ); the engine embeds
        B x W raw observations per call instead of B x L, which lifts the single call's 2 GiB bound.  Appended contexts never
        replace a state, so reset=False with shorter lengths is accepted here.  window=None (or W >= L): the single call.
        `envs` as in extend_contexts: the envs that are scored (None: the active ones); the others' rows of the result hold
        the fill values of masked rows (0 / token -1) and their state is left alone."""
        obs, frames, rtg, rew, lengths, discrete = self._prepare_contexts(observations, returns_to_go, rewards, lengths)
        B, L = rtg.shape
        target = None
        if actions is not None:
            a = actions.to(self.device, torch.float32).reshape(B, L, -1)
            if a.shape[-1] > self.spec.act_dim:
                raise ValueError(f"actions: {a.shape[-1]} action dims exceed max_act_dim {self.spec.act_dim}")
            target = torch.zeros(B, L, self.spec.act_dim, dtype=torch.float32, device=self.device)
            target[..., : a.shape[-1]] = a
        if window is not None and int(window) < 1:
            raise ValueError(f"score_trajectories: window must be >= 1, got {window}")
        windowed = window is not None and int(window) < L
        if lengths is not None and not windowed and not reset and any(0 < n < L for n in lengths):
            raise ValueError("score_trajectories: a context shorter than L replaces the env's state; reset=False cannot "
                             "be combined with a length in 1 .. L - 1")
        want = tuple(w for w in ((want,) if isinstance(want, str) else want) if w != "logp" or target is not None)
        with self._context_envs(envs, lengths) as idx:
            if idx is not None:   # the rows of the listed envs, in slot order; the others' rows of the result hold the fill values
                obs, frames, rtg, rew, lengths = self._gather_contexts(idx, obs, frames, rtg, rew, lengths)
                target = None if target is None else target[idx].contiguous()
            res = self._score_rows(obs, frames, rtg, rew, target, lengths, discrete, reset, over, temperature, want, logits,
                                   window if windowed else None)
            if idx is not None:
                fills = {"actions": 0, "tokens": -1, "logp": 0, "logits": 0}
                res = ScoreResult(**{name: None if getattr(res, name) is None else self._scatter_rows(getattr(res, name), idx, fills[name])
                                     for name in ScoreResult.__slots__})
        return res

    def _score_rows(self, obs, frames, rtg, rew, target, lengths, discrete, reset, over, temperature, want, logits, window):
        """score_trajectories on the rows it hands the engine: one call, or `window` timesteps per call."""
        B, L = rtg.shape
        mask = torch.ones(B, dtype=torch.uint8, device=self.device) if reset else None
        if window is None:
            return self._engine_score(obs, frames, rtg, rew, actions=target, reset_mask=mask, discrete=discrete, over=over,
                                      temperature=temperature, want=want, logits=logits, lengths=lengths)
        W = int(window)
        n_all = [L] * B if lengths is None else list(lengths)
        A = self.spec.act_dim
        # the fill values of masked rows: what no window covers keeps them
        out = ScoreResult(
            actions=torch.zeros(B, L, A, dtype=torch.float32, device=self.device) if "actions" in want else None,
            tokens=torch.full((B, L, A), -1, dtype=torch.int32, device=self.device) if "tokens" in want else None,
            logp=torch.zeros(B, L, A, dtype=torch.float32, device=self.device) if "logp" in want else None,
            logits=torch.zeros(B, L, A, self.spec.n_vocab, dtype=torch.float32, device=self.device) if logits else None)
        for k in range(-(-max(n_all) // W)):
            lo, hi = k * W, min((k + 1) * W, L)
            part = self._engine_score(obs, frames, rtg, rew, lo, hi,
                                      actions=None if target is None else target[:, lo:hi].contiguous(),
                                      reset_mask=mask if k == 0 else None, discrete=discrete, over=over, temperature=temperature,
                                      want=want, logits=logits, lengths=[min(max(n - lo, 0), hi - lo) for n in n_all], append=True)
            for name in ScoreResult.__slots__:
                if getattr(out, name) is not None:
                    getattr(out, name)[:, lo:hi] = getattr(part, name)
        return out

    @torch.no_grad()
    def extend_contexts(self, observations: torch.Tensor, returns_to_go: torch.Tensor,
                        rewards: Optional[torch.Tensor] = None, lengths=None, restart=None, want_action: bool = False,
                        envs=None):
        """Append to every env's state a stored context of its own length in one call (Engine.prefill(lengths=..., append=True)),
        after which predict_batch continues: the steps envs at different points of their episodes missed, or a demonstration
        that continues an in-context evaluation (persist_context).  observations [B, L, obs_dim] -- native, padded and normalised
        as prime_contexts does, image observations included -- returns_to_go [B, L], rewards [B, L] (None: zeros), `lengths` [B]: env b takes its first
        lengths[b] timesteps (None = all L); an env of length 0 keeps its state bit for bit.  `restart` [B] bool (None: nobody):
        the envs that start from an empty state before their first timestep.  want_action=True returns the action at each env's
        own last timestep (as predict_batch returns it; 0 for an env of length 0), else None.
        `envs`: the env ids that take part (None: the active envs); every tensor stays full-width in env-id order, as in
        predict_batch.  The others -- parked or not -- are not rows of the call: their state is left alone and their rows of the
        result hold 0.  A listed env that was parked is parked again afterwards, its context extended (_context_envs)."""
        B = self.n_envs
        obs, frames, rtg, rew, lengths, discrete = self._prepare_contexts(observations, returns_to_go, rewards, lengths)
        mask = None
        if restart is not None:
            mask = torch.as_tensor(restart).reshape(-1)
            if mask.shape[0] != B:
                raise ValueError(f"restart: expected {B} entries (one per env), got {mask.shape[0]}")
            mask = (mask != 0).to(self.device, torch.uint8).contiguous()
        with self._context_envs(envs, lengths) as idx:
            if idx is not None:
                obs, frames, rtg, rew, lengths = self._gather_contexts(idx, obs, frames, rtg, rew, lengths)
                mask = None if mask is None else mask[idx].contiguous()
            actions, _ = self._engine_prefill(obs, frames, rtg, rew, reset_mask=mask, discrete=discrete, want_action=want_action,
                                              lengths=lengths, append=True)
            if want_action and idx is not None:
                actions = self._scatter_rows(actions, idx)
        if not want_action:
            return None
        return actions[:, :1].to(torch.int64) if self.is_discrete else actions

    @torch.no_grad()
    def prime_contexts(self, observations: torch.Tensor, returns_to_go: torch.Tensor,
                       rewards: Optional[torch.Tensor] = None, lengths=None, want_action: bool = False, envs=None):
        """Prime every env with its own stored context in one call (Engine.prefill(lengths=...)), after which predict_batch
        continues: observations [B, L, obs_dim] -- padded and normalised as predict_batch does -- returns_to_go [B, L], rewards
        [B, L] (None: zeros) and `lengths` [B]: env b's context is its first lengths[b] timesteps (None = all L).  Every env
        with a context starts from an empty state; an env of length 0 keeps the state it has.  want_action=True returns the
        action at each env's own last timestep (as predict_batch returns it), else None.  Image observations as in
        score_trajectories.  `envs` as in extend_contexts: the envs that are primed (None: the active ones)."""
        obs, frames, rtg, rew, lengths, discrete = self._prepare_contexts(observations, returns_to_go, rewards, lengths)
        with self._context_envs(envs, lengths) as idx:
            if idx is not None:
                obs, frames, rtg, rew, lengths = self._gather_contexts(idx, obs, frames, rtg, rew, lengths)
            mask = torch.ones(rtg.shape[0], dtype=torch.uint8, device=self.device)
            actions, _ = self._engine_prefill(obs, frames, rtg, rew, reset_mask=mask, discrete=discrete, want_action=want_action,
                                              lengths=lengths)
            if want_action and idx is not None:
                actions = self._scatter_rows(actions, idx)
        if not want_action:
            return None
        return actions[:, :1].to(torch.int64) if self.is_discrete else actions

    @torch.no_grad()
    def action_log_prob(self, over: str = "selectable") -> torch.Tensor:
        """float32 [n_envs, act_dim]: the log-probability of the tokens the last predict_batch / predict returned, under that
        call's logits (Engine.last_logp) -- the score that ranks the forks of fork_slots, or importance weights.
        over="sampled": under the distribution each token was DRAWN from -- the slot's own temperature, top_k and top_p
        applied (per-slot settings included; a greedy slot's token scores 0).  These are the importance weights of a sampling
        agent: with the reference's default top_p = 0.5 half of every row is outside the support.  Needs sampling armed.
        over="selectable" / "vocab": under the unfiltered softmax -- the agent-level temperature multiplies the logits, top_k,
        top_p and per-slot settings are NOT applied.
        Columns a slot does not use hold 0."""
        idx = self._live_index()
        toks = self.engine._tokens if idx is None else self.engine._tokens[:idx.shape[0]]   # (the live rows)
        if over == "sampled":
            lp = self.engine.last_logp(toks, over="sampled")
        else:
            t = 1.0 if self.a_sample_kwargs is None else float(self.a_sample_kwargs["temperature"])
            lp = self.engine.last_logp(toks, over=over, temperature=t)
        return lp if idx is None else self._scatter_rows(lp, idx)   # (rows of parked envs hold 0)

    def _predict_batch_slots(self, observation, returns_to_go, rewards, reset_mask):
        if not isinstance(observation, (tuple, list)) or len(observation) != 2:
            raise ValueError("with a slot table predict_batch takes observation = (vector_obs, images)")
        vec, images = observation
        idx = self._live_index()
        if idx is not None:
            return self._predict_batch_slots_live(vec, images, returns_to_go, rewards, reset_mask, idx)
        n_img = self.slot_table.n_image
        if n_img > 0:
            if not self.has_image_encoder:
                raise RuntimeError("the slot table holds image slots but the state dict has no embed_image.* weights")
            if images is None or images.dim() != 4 or images.shape[0] != n_img:
                raise ValueError(f"images: expected uint8 [{n_img}, C, H, W] (one frame per image slot, in slot order)")
            images = images.to(self.device).to(torch.uint8).contiguous()
        else:
            images = None
        if vec is None:
            if n_img != self.n_envs:
                raise ValueError("vector_obs: None is allowed only when every slot is an image slot")
        else:
            if vec.dim() != 2 or vec.shape[0] != self.n_envs:
                raise ValueError(f"vector_obs: expected [{self.n_envs}, obs_dim]")
            vec, _ = self._prepare_obs(vec)
        rtg = returns_to_go.to(self.device, torch.float32).reshape(-1).contiguous()
        rew = self._zero_reward if rewards is None else rewards.to(self.device, torch.float32).reshape(-1).contiguous()
        if reset_mask is not None:
            reset_mask = reset_mask.to(self.device, torch.uint8).contiguous()
        actions, _ = self.engine.step_slots(vec, images, rtg, rew, reset_mask)
        return actions

    def _predict_batch_slots_live(self, vec, images, returns_to_go, rewards, reset_mask, idx):
        """The mixed batch with parked envs: an env sits in a slot with its own table entry (set_active refuses anything else),
        so env e's frame is the one its own slot index would take, and the engine gets the frames of the live image slots."""
        n, table = self.n_envs, self.slot_table
        is_img = torch.as_tensor(table.image).bool().cpu()
        rank = torch.cumsum(is_img.long(), 0) - 1   # env id -> its frame among the call's frames
        live = idx.cpu()
        frames = rank[live][is_img[live]]
        if table.n_image > 0 and (images is None or images.dim() != 4 or images.shape[0] != table.n_image):
            raise ValueError(f"images: expected uint8 [{table.n_image}, C, H, W] (one frame per image slot, in slot order)")
        img_l = None
        if frames.numel() > 0:
            img_l = images.to(self.device).to(torch.uint8)[frames.to(self.device)].contiguous()
        if vec is None:
            if frames.numel() != live.numel():
                raise ValueError("vector_obs: None is allowed only when every slot is an image slot")
            vec_l = None
        else:
            if vec.dim() != 2 or vec.shape[0] != n:
                raise ValueError(f"vector_obs: expected [{n}, obs_dim]")
            vec_l, _ = self._prepare_obs(vec.to(self.device)[idx])
        rtg = returns_to_go.to(self.device, torch.float32).reshape(-1)[idx].contiguous()
        rew = self._zero_reward[:rtg.shape[0]] if rewards is None else rewards.to(self.device, torch.float32).reshape(-1)[idx].contiguous()
        if reset_mask is not None:
            reset_mask = reset_mask.to(self.device, torch.uint8).reshape(-1)[idx].contiguous()
        actions, _ = self.engine.step_slots(vec_l, img_l, rtg, rew, reset_mask)
        return self._scatter_rows(actions, idx)

    # ---- reference single-env surface -------------------------------------------------------------
    @torch.no_grad()
    def predict(self, policy, observation, actions, rewards, returns_to_go, timesteps, state=None,
                episode_start=None, deterministic=True, context_len=5, prompt=None, task_id=None, is_eval=False,
                env_act_dim=None):
        if self.n_envs != 1:
            raise RuntimeError("predict() is the reference's single-env entry; use predict_batch() for n_envs > 1")
        obs_shape = observation.shape[1:]
        states = observation.reshape(1, -1, *obs_shape)
        returns_to_go = returns_to_go.reshape(1, -1, 1)
        timesteps = timesteps.reshape(1, -1)
        if rewards is not None:
            rewards = rewards.reshape(1, -1, 1)
        a1, a2 = self.get_action_pred(policy, states, actions, rewards, returns_to_go, timesteps, None,
                                      deterministic, prompt, is_eval=is_eval, task_id=task_id,
                                      env_act_dim=env_act_dim)
        if self.reset_inf_cache_freq is not None:
            current_step = int(timesteps[0, -1])
            if current_step > 0 and current_step % self.reset_inf_cache_freq == 0:
                self.past_key_values = None  # context is dropped, not re-primed
                if self.reprime_context and observation.dim() == 2:
                    n = min(int(self.eval_context_len), states.shape[1])
                    obs_seq, _ = self._prepare_obs(states[0, -n:])
                    rew_seq = torch.zeros(1, n, device=self.device) if rewards is None else \
                        rewards[:, -n:, 0].to(self.device, torch.float32)
                    self.engine.prefill(obs_seq.view(1, n, -1).contiguous(),
                                        returns_to_go[:, -n:, 0].to(self.device, torch.float32).contiguous(),
                                        rew_seq.contiguous(), want_action=False)
        return a1, a2

    @torch.no_grad()
    def get_action_pred(self, policy, states, actions, rewards, returns_to_go, timesteps, attention_mask,
                        deterministic, prompt, is_eval=False, task_id=None, env_act_dim=None):
        """With the inference cache on, only the last timestep's (state, rtg, reward) reach the encoder
        (online_decision_transformer_model.py:466-470).  use_inference_cache=False is served by predict_batch alone (it keeps
        the history on the device); this single-env view raises in that mode."""
        if not getattr(self, "use_inference_cache", True):
            raise RuntimeError("use_inference_cache=False: the single-env predict / get_action_pred surface is not wired to "
                               "the window ring; use predict_batch(..., prev_rewards=, relabel=, keep=)")
        obs = states[:, -1]
        rtg = returns_to_go[:, -1].reshape(1)
        rew = None if rewards is None else rewards[:, -1].reshape(1)
        act = self.predict_batch(obs, rtg, rew, None, env_act_dim).clone()
        a = act[0]
        if self.is_discrete:
            a = a[: (1 if env_act_dim is None else env_act_dim)]
        return a, a

    get_action = get_action_pred
