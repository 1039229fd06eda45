"""Domains of a multi-domain agent and the slot table of a mixed batch (plain data: no engine, usable on the CPU).

One set of weights serves Atari / Procgen (uint8 frames in, one of `n_discrete` actions out) and Meta-World, DMControl,
Composuite, Mimicgen (vector observations, 1-8 tokenised continuous action dims).  The reference's evaluation loop hands
every call the env's own `env_act_dim` and `is_discrete` (src/callbacks/evaluation.py:90-138) and looks reward scale and
target return up per domain (src/algos/decision_transformer_sb3.py:373-382,542-559).  A `SlotTable` states the same per env
slot of ONE batch: contiguous slot ranges, one per domain, plus the arrays `Engine.set_slot_table` takes and per-slot
`reward_scale` / `rtg0` tensors for `BatchedRollout`.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch


@dataclass(frozen=True)
class Domain:
    name: str
    discrete: bool                 # discrete head: the action is an index below n_discrete (act_dim must be 1)
    act_dim: int                   # action dims the env uses (env_act_dim)
    image: bool = False            # observations are uint8 frames (IMPALA-CNN front end), else vectors
    reward_scale: float = 1.0
    target_return: float = 0.0     # in env units; the rtg token starts at target_return / reward_scale
    inv_index: Optional[Sequence[int]] = None   # full-space scatter table of vector observations (obs.inverse_index), or None = zero-pad
    # how this domain's slots pick their tokens: None = the agent's own a_sample_kwargs (argmax where it has none); a dict =
    # sample_from_logits' keywords for this domain, completed with its defaults and checked against THIS domain's head width;
    # "greedy" = argmax for this domain whatever the agent samples elsewhere
    a_sample_kwargs: object = None
    # the actions this domain's envs have: action indices below n_discrete for a discrete domain (Procgen: range(15); Pong on its
    # minimal set: 0, 1, 3, 4, 11, 12), vocabulary token ids for a continuous one; None = every token of the head's range
    allowed_actions: Optional[Sequence[int]] = None

    def __post_init__(self):
        if self.allowed_actions is not None:
            acts = list(self.allowed_actions)
            if not acts:
                raise ValueError(f"domain {self.name!r}: allowed_actions is empty (None allows everything)")
            if any(isinstance(a, bool) or int(a) != a or a < 0 for a in acts):
                raise ValueError(f"domain {self.name!r}: allowed_actions must be integers >= 0, got {acts}")
            if len(set(int(a) for a in acts)) != len(acts):
                raise ValueError(f"domain {self.name!r}: allowed_actions lists an action twice: {acts}")
            object.__setattr__(self, "allowed_actions", tuple(int(a) for a in acts))
        s = self.a_sample_kwargs
        if not (s is None or isinstance(s, dict) or s == "greedy"):
            raise ValueError(f"domain {self.name!r}: a_sample_kwargs must be None, a dict or \"greedy\", got {s!r}")
        if int(self.act_dim) != self.act_dim or self.act_dim < 1:
            raise ValueError(f"domain {self.name!r}: act_dim must be an integer >= 1, got {self.act_dim}")
        if self.discrete and self.act_dim != 1:
            raise ValueError(f"domain {self.name!r}: a discrete domain has act_dim 1, got {self.act_dim}")
        if not (float(self.reward_scale) > 0.0 and float(self.reward_scale) < float("inf")):
            raise ValueError(f"domain {self.name!r}: reward_scale must be finite and > 0, got {self.reward_scale}")
        if self.image and self.inv_index is not None:
            raise ValueError(f"domain {self.name!r}: an image domain has no observation index table")


class SlotTable:
    """Domains laid out as contiguous env-slot ranges, in the order given."""

    def __init__(self, domains: List[Domain], counts: List[int], max_act_dim: Optional[int] = None):
        self.domains, self.counts = list(domains), [int(n) for n in counts]
        self.ranges: List[Tuple[int, int]] = []
        b = 0
        for n in self.counts:
            self.ranges.append((b, b + n))
            b += n
        self.n_slots = b
        self.max_act_dim = max_act_dim
        rep = torch.tensor(self.counts)

        def per_slot(values, dtype):
            return torch.repeat_interleave(torch.tensor(values, dtype=dtype), rep)
        self.slot_domain = per_slot(list(range(len(self.domains))), torch.int64)
        self.discrete = per_slot([bool(d.discrete) for d in self.domains], torch.bool)
        self.image = per_slot([bool(d.image) for d in self.domains], torch.bool)
        self.act_dim = per_slot([int(d.act_dim) for d in self.domains], torch.int64)
        # float64: exactly the Python floats of the domains (BatchedRollout divides them as it divides its float arguments)
        self.reward_scale = per_slot([float(d.reward_scale) for d in self.domains], torch.float64)
        self.target_return = per_slot([float(d.target_return) for d in self.domains], torch.float64)
        # the rtg token of a fresh episode, as BatchedRollout forms it for one domain: float(target) / float(scale), then fp32
        self.rtg0 = per_slot([float(d.target_return) / float(d.reward_scale) for d in self.domains], torch.float32)

    @classmethod
    def from_domains(cls, layout: Sequence[Tuple[Domain, int]], max_act_dim: Optional[int] = None) -> "SlotTable":
        """layout: [(domain, n_slots), ...].  `max_act_dim` (the model's act_dim), when given, bounds every domain's."""
        layout = list(layout)
        if not layout:
            raise ValueError("SlotTable.from_domains: no domain given")
        names = set()
        for dom, n in layout:
            if not isinstance(dom, Domain):
                raise TypeError(f"SlotTable.from_domains: expected (Domain, n_slots) pairs, got {type(dom).__name__}")
            if int(n) != n or n < 1:
                raise ValueError(f"domain {dom.name!r}: n_slots must be an integer >= 1, got {n}")
            if dom.name in names:
                raise ValueError(f"domain {dom.name!r} is listed twice")
            names.add(dom.name)
            if max_act_dim is not None and dom.act_dim > max_act_dim:
                raise ValueError(f"domain {dom.name!r}: act_dim {dom.act_dim} exceeds the model's {max_act_dim}")
        return cls([d for d, _ in layout], [n for _, n in layout], max_act_dim)

    # -- what the engine and the rollout take ----------------------------------------------------
    def engine_arrays(self):
        """(discrete bool [B], act_dim int64 [B], image bool [B]): the arguments of Engine.set_slot_table."""
        return self.discrete, self.act_dim, self.image

    def sample_settings(self, n_discrete: int, n_vocab: int, agent_kwargs: Optional[dict] = None) -> Optional[dict]:
        """Per-slot sampling settings {"temperature": float64 [B], "top_k": int32 [B], "top_p": float64 [B], "greedy": bool [B]}
        (the arguments of Engine.set_sampling_slots), or None when no domain states its own and the agent's setting serves
        every slot.  A domain's dict is completed and checked by resolve_sample_kwargs against that domain's head width
        (n_discrete logits for a discrete domain, n_vocab otherwise); so is `agent_kwargs` for every domain that falls back
        on it.  Domains with neither are greedy."""
        from .agent import resolve_sample_kwargs
        per_domain = []
        for d in self.domains:
            n_head = n_discrete if d.discrete else n_vocab
            s = d.a_sample_kwargs
            if s is None:
                s = agent_kwargs
            per_domain.append(None if s is None or s == "greedy" else resolve_sample_kwargs(s, n_head))
        if all(d.a_sample_kwargs is None for d in self.domains):
            return None
        rep = torch.tensor(self.counts)

        def per_slot(key, fill, dtype):
            return torch.repeat_interleave(torch.tensor([fill if s is None else s[key] for s in per_domain], dtype=dtype), rep)
        return {"temperature": per_slot("temperature", 1.0, torch.float64), "top_k": per_slot("top_k", 0, torch.int32),
                "top_p": per_slot("top_p", 0.0, torch.float64),
                "greedy": torch.repeat_interleave(torch.tensor([s is None for s in per_domain], dtype=torch.bool), rep)}

    def action_mask(self, n_vocab: int, n_discrete: int) -> Optional[torch.Tensor]:
        """The allowed sets of the layout, bool [B, n_vocab] (the argument of Engine.set_action_mask), or None when no domain
        states one.  A domain without a set allows every token.  Every index is checked against the domain's range: below
        n_discrete for a discrete domain, below n_vocab otherwise."""
        if all(d.allowed_actions is None for d in self.domains):
            return None
        rows = []
        for d in self.domains:
            row = torch.ones(int(n_vocab), dtype=torch.bool)
            if d.allowed_actions is not None:
                n = int(n_discrete) if d.discrete else int(n_vocab)
                bad = [a for a in d.allowed_actions if a >= n]
                if bad:
                    raise ValueError(f"domain {d.name!r}: allowed_actions {bad} outside the {n} "
                                     f"{'actions of the discrete head' if d.discrete else 'tokens of the vocabulary'}")
                row = torch.zeros(int(n_vocab), dtype=torch.bool)
                row[list(d.allowed_actions)] = True
            rows.append(row)
        return torch.repeat_interleave(torch.stack(rows), torch.tensor(self.counts), dim=0)

    @property
    def n_image(self) -> int:
        return int(self.image.sum())

    @property
    def image_slots(self) -> torch.Tensor:
        """Env slots with frame observations, ascending: frame k of a step_slots call belongs to image_slots[k]."""
        return torch.nonzero(self.image).reshape(-1)

    @property
    def vector_slots(self) -> torch.Tensor:
        return torch.nonzero(~self.image).reshape(-1)

    def slots_of(self, name: str) -> range:
        for dom, (lo, hi) in zip(self.domains, self.ranges):
            if dom.name == name:
                return range(lo, hi)
        raise KeyError(name)

    def domain_of(self, slot: int) -> Domain:
        if not 0 <= int(slot) < self.n_slots:
            raise IndexError(f"slot {slot} outside 0 .. {self.n_slots - 1}")
        return self.domains[int(self.slot_domain[int(slot)])]

    def find(self, key) -> Domain:
        """A domain by name, or by position in the layout (the `task_id` / `envid` of the agent's per-domain lookups)."""
        if isinstance(key, str):
            for dom in self.domains:
                if dom.name == key:
                    return dom
            raise KeyError(key)
        return self.domains[int(key)]

    def pad_tables(self, state_dim: int):
        """(slot_row int32 [B], inv_index int32 [n_domains, state_dim]) for pad_obs_slots: one row per domain -- its
        `inv_index`, or the identity prefix that zero-pads (image domains: all -1, their rows of the output are unused)."""
        rows = []
        for dom in self.domains:
            if dom.inv_index is not None:
                row = torch.as_tensor(dom.inv_index, dtype=torch.int32).reshape(-1)
                if row.numel() != state_dim:
                    raise ValueError(f"domain {dom.name!r}: inv_index has {row.numel()} entries, expected {state_dim}")
            elif dom.image:
                row = torch.full((state_dim,), -1, dtype=torch.int32)
            else:
                row = torch.arange(state_dim, dtype=torch.int32)   # columns beyond the native width are cut by the caller's n_native
            rows.append(row)
        return self.slot_domain.to(torch.int32), torch.stack(rows)
