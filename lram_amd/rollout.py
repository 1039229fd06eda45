"""Batched multi-env rollout driver (the caller of the hot path) and a synthetic vector env.

Batched counterpart of the reference's single-env loop `custom_evaluate_policy`
(src/callbacks/evaluation.py:130-257): per timestep it feeds (state, rtg, reward-token 0) to the agent,
steps the envs, updates `rtg -= r / reward_scale` (:165), and on `done` resets that env's context
(:238-251).  All bookkeeping is vectorised device tensors; there is no per-step host sync except the one
the caller asks for.  Timing keys follow src/callbacks/custom_eval_callback.py:468-475.

`SyntheticVecEnv` is the batched DummyEnv (src/envs/dummy_env_utils.py:8-35): observations U(-1, 1),
reward 1 every step, episode ends after `ep_len` steps.

`evaluate_policy_batched` keeps the call contract of `custom_evaluate_policy` (evaluation.py:14-271: episode
targets per sub-env, return tuple, `reward_threshold`, per-step `callback`, `persist_context`) for a vector env of
any width, and `eval_log_record` produces the keys `_on_step_logging` records
(src/callbacks/custom_eval_callback.py:439-515, 563-588).
"""
from __future__ import annotations

import time
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

# DMControl full observation space offsets used by cheetah-run (src/envs/dmcontrol_utils.py:44-49):
# 'position' (8 dims) starts at 41, 'velocity' (9 dims) at 14.
CHEETAH_RUN_OBS_INDEX = tuple(range(41, 49)) + tuple(range(14, 23))


class SyntheticVecEnv:
    def __init__(self, n_envs: int, obs_dim: int = 10, act_dim: int = 1, ep_len: int = 1000, device="cpu",
                 seed: int = 1234, stagger: bool = True, obs_index: Optional[Sequence[int]] = None,
                 full_dim: Optional[int] = None, image_shape: Optional[Sequence[int]] = None,
                 success_every: Optional[int] = None):
        self.n_envs, self.obs_dim, self.act_dim, self.ep_len = n_envs, obs_dim, act_dim, ep_len
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device).manual_seed(seed)
        self.image_shape = tuple(image_shape) if image_shape is not None else None
        self.full_dim = full_dim
        self.obs_index = None if obs_index is None else torch.tensor(list(obs_index), device=self.device)
        # env e is `e mod ep_len` steps into its episode at t = 0: resets are staggered over time
        self.t = (torch.arange(n_envs, device=self.device) % ep_len) if stagger else \
            torch.zeros(n_envs, dtype=torch.long, device=self.device)
        # Meta-World-style `is_success` info at episode end (every `success_every`-th episode of an env succeeds)
        self.success_every = success_every
        self.episodes = torch.zeros(n_envs, dtype=torch.long, device=self.device)
        self.last_info: Dict[str, torch.Tensor] = {}

    def _sample(self):
        if self.image_shape is not None:
            return torch.randint(0, 256, (self.n_envs, *self.image_shape), generator=self.gen, device=self.device,
                                 dtype=torch.uint8)
        raw = torch.rand(self.n_envs, self.obs_dim, generator=self.gen, device=self.device) * 2.0 - 1.0
        if self.obs_index is None:
            return raw
        full = torch.zeros(self.n_envs, self.full_dim, device=self.device)
        full[:, self.obs_index] = raw
        return full

    def reset(self):
        return self._sample()

    def step(self, actions):
        self.t = self.t + 1
        done = self.t >= self.ep_len
        self.t = torch.where(done, torch.zeros_like(self.t), self.t)
        reward = torch.ones(self.n_envs, device=self.device)
        self.episodes = self.episodes + done.long()
        if self.success_every is not None:
            self.last_info = {"is_success": done & (self.episodes % self.success_every == 0)}
        return self._sample(), reward, done

    def copy_slots(self, src, dst):
        """Env dst[i] continues from where env src[i] stands: its position in the episode and its episode count."""
        src_t = torch.as_tensor(list(src), dtype=torch.long, device=self.device)
        dst_t = torch.as_tensor(list(dst), dtype=torch.long, device=self.device)
        self.t[dst_t] = self.t[src_t]
        self.episodes[dst_t] = self.episodes[src_t]


class SlotScheduler:
    """Which env sits in which engine slot while some envs are parked (Engine.set_live / swap_slots): pure bookkeeping, no GPU.

    The engine steps the slots [0, n_live) and leaves [n_live, n) alone, so the live envs must sit in a prefix of the slots.
    The scheduler keeps the permutation env id <-> slot; park() and resume() return the slot pairs to exchange and the new live
    count.  Every parked or resumed env takes at most one swap, and all indices of one swap list are distinct (what
    lram_state_swap_slots asks for).  The reference has no counterpart: its loop keeps forwarding an env that has finished its
    share of episodes (src/callbacks/evaluation.py:184,205-212)."""

    def __init__(self, n: int):
        if n < 1:
            raise ValueError("SlotScheduler: n must be >= 1")
        self.n = int(n)
        self.n_live = self.n
        self.slot_of = list(range(self.n))   # env id -> slot
        self.env_at = list(range(self.n))    # slot -> env id

    def live_envs(self) -> List[int]:
        """Env id of every live slot, in slot order."""
        return self.env_at[:self.n_live]

    def is_live(self, env: int) -> bool:
        return self.slot_of[env] < self.n_live

    @property
    def identity(self) -> bool:
        return all(e == s for s, e in enumerate(self.env_at))

    def _ids(self, env_ids, want_live: bool, what: str) -> List[int]:
        ids = [int(e) for e in env_ids]
        if len(set(ids)) != len(ids):
            raise ValueError(f"{what}: an env is listed twice")
        for e in ids:
            if not 0 <= e < self.n:
                raise ValueError(f"{what}: env {e} outside 0 .. {self.n - 1}")
            if self.is_live(e) != want_live:
                raise ValueError(f"{what}: env {e} is {'parked already' if want_live else 'not parked'}")
        return ids

    def _swap(self, pairs):
        for sa, sb in pairs:
            ea, eb = self.env_at[sa], self.env_at[sb]
            self.env_at[sa], self.env_at[sb] = eb, ea
            self.slot_of[ea], self.slot_of[eb] = sb, sa

    def park(self, env_ids):
        """Park the listed live envs.  Returns (a, b, n_live): exchange slots a[i] <-> b[i], then n_live slots are live."""
        ids = self._ids(env_ids, True, "park")
        new_live = self.n_live - len(ids)
        if new_live < 1:
            raise ValueError("park: at least one env must stay live")
        leaving = set(ids)
        # a parked env below the new boundary changes places with a staying env in the stretch that gets parked
        out = sorted(self.slot_of[e] for e in ids if self.slot_of[e] < new_live)
        inn = [s for s in range(new_live, self.n_live) if self.env_at[s] not in leaving]
        pairs = list(zip(out, inn))
        self._swap(pairs)
        self.n_live = new_live
        return [p[0] for p in pairs], [p[1] for p in pairs], new_live

    def resume(self, env_ids):
        """Make the listed parked envs live again.  Returns (a, b, n_live) as park()."""
        ids = self._ids(env_ids, False, "resume")
        new_live = self.n_live + len(ids)
        coming = set(ids)
        # a resumed env beyond the new boundary changes places with a still-parked env in the stretch that goes live
        far = sorted(self.slot_of[e] for e in ids if self.slot_of[e] >= new_live)
        near = [s for s in range(self.n_live, new_live) if self.env_at[s] not in coming]
        pairs = list(zip(near, far))
        self._swap(pairs)
        self.n_live = new_live
        return [p[0] for p in pairs], [p[1] for p in pairs], new_live

    def arrange(self, env_ids):
        """Put the listed envs, live or parked, into slots 0 .. n - 1 in the given order.  Returns the swap lists [(a, b), ...] to
        hand to Engine.swap_slots one after the other -- at most two, however many envs are listed, and all indices of one
        list distinct.  The live count is the caller's business and does not move; an env that is not listed moves only if it
        sits in a slot the listed ones take.  Applying the lists again in reverse order undoes the arrangement.
        Why two: the slots' contents move by a permutation, every cycle (c_0 -> c_1 -> ... -> c_{k-1} -> c_0) of it is a
        rotation j -> j + 1, and a rotation is the product of the reflections j -> -j and j -> 1 - j (mod k), each an
        involution: a list of disjoint swaps.  The first list holds the first reflection of every cycle, the second the second."""
        ids = [int(e) for e in env_ids]
        if len(set(ids)) != len(ids) or any(not 0 <= e < self.n for e in ids):
            raise ValueError(f"arrange: expected distinct env ids in 0 .. {self.n - 1}")
        n = len(ids)
        to = {self.slot_of[e]: i for i, e in enumerate(ids)}   # slot now -> slot afterwards, of the listed envs
        # An unlisted env in the prefix goes to the slot that the chain of listed envs ending at its slot started from: the
        # chains close into cycles and no other slot is touched.
        for f in [s for s in to if s >= n]:
            d = f
            while d in to:
                d = to[d]
            to[d] = f
        first, second, seen = [], [], set()
        for s0 in sorted(to):
            if s0 in seen or to[s0] == s0:
                continue
            cyc = [s0]
            while to[cyc[-1]] != s0:
                cyc.append(to[cyc[-1]])
            seen.update(cyc)
            k = len(cyc)
            first += [(cyc[j], cyc[-j % k]) for j in range(k) if j < -j % k]
            second += [(cyc[j], cyc[(1 - j) % k]) for j in range(k) if j < (1 - j) % k]
        lists = []
        for pairs in (first, second):
            if pairs:
                self._swap(pairs)
                lists.append(([p[0] for p in pairs], [p[1] for p in pairs]))
        return lists


class BatchedRollout:
    """agent: object with predict_batch(obs, rtg, rewards, reset_mask, env_act_dim) (lram_amd.agent.RecurrentAgent); one whose
    `use_inference_cache` is False also takes prev_rewards=, relabel=, keep= (context-window mode, _step_window)."""

    def __init__(self, agent, env: SyntheticVecEnv, target_return, reward_scale,
                 env_act_dim: Optional[int] = None, persist_context: bool = False):
        """target_return / reward_scale: floats, or [n_envs] tensors for a batch of envs from several domains
        (lram_amd.domains.SlotTable.target_return / .reward_scale): slot b then follows rtg - r / reward_scale[b]."""
        self.agent, self.env = agent, env
        # evaluation.py:213-236: with persist_context the (cached) context survives episode ends -- only the
        # target return and the timestep restart; without it the env's cache is reset (:238-251)
        self.persist_context = bool(persist_context)
        dev = env.device
        per_slot = torch.is_tensor(target_return) or torch.is_tensor(reward_scale)
        if per_slot:
            def as_slots(v, name):
                t = torch.as_tensor(v).to(device=dev, dtype=torch.float64)   # (float64 tensors keep what a Python float holds)
                t = t.expand(env.n_envs) if t.dim() == 0 else t
                if tuple(t.shape) != (env.n_envs,):
                    raise ValueError(f"{name}: expected a float or a [{env.n_envs}] tensor, got shape {tuple(t.shape)}")
                return t.contiguous()
            scale64 = as_slots(reward_scale, "reward_scale")
            # slot by slot what the float form computes: float(target) / float(scale) in double, then fp32
            self.rtg0 = (as_slots(target_return, "target_return") / scale64).float()
            self.reward_scale = scale64.float()
        else:
            self.reward_scale = float(reward_scale)
            self.rtg0 = float(target_return) / float(reward_scale)
        self.env_act_dim = env_act_dim
        self.obs = env.reset()
        self.rtg = self.rtg0.clone() if per_slot else torch.full((env.n_envs,), self.rtg0, device=dev)
        self.reset_mask = torch.ones(env.n_envs, dtype=torch.uint8, device=dev)  # every env starts an episode
        self.timestep = torch.zeros(env.n_envs, dtype=torch.long, device=dev)
        self.ep_return = torch.zeros(env.n_envs, device=dev)
        self.finished_returns = []
        self.finished_lengths = []
        # context-window mode (agent.use_inference_cache False; _step_window): the scaled reward of the step before, the relabel /
        # keep lists the next call takes (None: no episode has just ended) and every env's finished episode lengths
        self.prev_reward = torch.zeros(env.n_envs, device=dev)
        self._window_relabel = self._window_keep = None
        self._episode_lengths = [[] for _ in range(env.n_envs)]

    @torch.no_grad()
    def _step_window(self):
        """One step with agent.use_inference_cache False (context-window inference; evaluation.py:130-251 with the cache off):
        the agent is handed the scaled reward of the step before -- it becomes the reward of the newest stored timestep (:153) --
        and at an episode end either the reset flag or, with persist_context, relabel = the episode's length (its returns-to-go
        are rewritten to the returns obtained, :219-222) and keep = min(sum of the last seqs_per_sample - 1 episode lengths,
        eval_context_len), eval_context_len when seqs_per_sample is 1 (:215-217, :223-224).  Episode ends reach the host."""
        n = self.env.n_envs
        actions = self.agent.predict_batch(self.obs, self.rtg, None, self.reset_mask, self.env_act_dim,
                                           prev_rewards=self.prev_reward, relabel=self._window_relabel, keep=self._window_keep)
        obs, reward, done = self.env.step(actions)
        self.ep_return += reward
        self.timestep += 1
        self._window_relabel = self._window_keep = None
        if bool(done.any()):
            self.finished_returns.append(self.ep_return[done].clone())
            self.finished_lengths.append(self.timestep[done].clone())
            if self.persist_context:
                K = int(self.agent.eval_context_len)
                seqs = int(self.agent.replay_buffer.seqs_per_sample) - 1
                self._window_relabel, self._window_keep = [0] * n, [0] * n
                for b in torch.nonzero(done).reshape(-1).tolist():
                    length = int(self.timestep[b])
                    self._episode_lengths[b].append(length)
                    self._window_relabel[b] = length
                    self._window_keep[b] = min(sum(self._episode_lengths[b][-seqs:]), K) if seqs > 0 else K
        rtg0 = self.rtg0 if torch.is_tensor(self.rtg0) else torch.full_like(self.rtg, self.rtg0)
        # (fp32 reward / fp32 scale, as the rtg below; the reference divides the env's float64 reward and rounds once, :152-153)
        self.prev_reward = (reward / self.reward_scale).to(torch.float32)
        self.rtg = torch.where(done, rtg0, self.rtg - reward / self.reward_scale)
        self.timestep = torch.where(done, torch.zeros_like(self.timestep), self.timestep)
        self.ep_return = torch.where(done, torch.zeros_like(self.ep_return), self.ep_return)
        self.reset_mask = torch.zeros_like(self.reset_mask) if self.persist_context else done.to(torch.uint8)
        self.obs = obs
        self.last_reward, self.last_done = reward, done
        return actions

    @torch.no_grad()
    def step(self):
        if not getattr(self.agent, "use_inference_cache", True):
            return self._step_window()
        actions = self.agent.predict_batch(self.obs, self.rtg, None, self.reset_mask, self.env_act_dim)
        obs, reward, done = self.env.step(actions)
        self.ep_return += reward
        self.timestep += 1
        if bool(done.any()):
            self.finished_returns.append(self.ep_return[done].clone())
            self.finished_lengths.append(self.timestep[done].clone())
        # evaluation.py:163-169 (not done) / :238-246 (done: fresh target return, timestep 0)
        rtg0 = self.rtg0 if torch.is_tensor(self.rtg0) else torch.full_like(self.rtg, self.rtg0)
        self.rtg = torch.where(done, rtg0, self.rtg - reward / self.reward_scale)
        self.timestep = torch.where(done, torch.zeros_like(self.timestep), self.timestep)
        self.ep_return = torch.where(done, torch.zeros_like(self.ep_return), self.ep_return)
        self.reset_mask = torch.zeros_like(self.reset_mask) if self.persist_context else done.to(torch.uint8)
        self.obs = obs
        self.last_reward, self.last_done = reward, done
        return actions

    def fork_slots(self, src, dst):
        """Env slot dst[i] becomes a copy of slot src[i] between two steps: the agent's recurrent state (agent.fork_slots), this
        driver's per-slot bookkeeping (observation, return-to-go, timestep, episode return; dst does not start an episode) and,
        where the env offers copy_slots(src, dst), the env's own per-slot state.  Same list rules as Engine.copy_slots."""
        from .engine import check_slot_lists
        src, dst = check_slot_lists(src, dst, self.env.n_envs)
        if not src:
            return
        # src / dst name ENVS, as all of this driver's bookkeeping does; the agent's call addresses engine slots, which differ from
        # env ids once set_active has exchanged slots
        sch = getattr(self.agent, "scheduler", None)
        if sch is not None and not sch.identity:
            self.agent.fork_slots([sch.slot_of[e] for e in src], [sch.slot_of[e] for e in dst])
        else:
            self.agent.fork_slots(src, dst)
        if hasattr(self.env, "copy_slots"):
            self.env.copy_slots(src, dst)
        dev = self.obs.device
        src_t = torch.as_tensor(src, dtype=torch.long, device=dev)
        dst_t = torch.as_tensor(dst, dtype=torch.long, device=dev)
        for name in ("obs", "rtg", "timestep", "ep_return", "prev_reward"):
            t = getattr(self, name)
            t[dst_t] = t[src_t]
        self.reset_mask[dst_t] = 0
        # context-window mode (an agent with window_slots="own" forks windows): what the next call hands over for the env
        for s, d in zip(src, dst):
            self._episode_lengths[d] = list(self._episode_lengths[s])
            for arr in (self._window_relabel, self._window_keep):
                if arr is not None:
                    arr[d] = arr[s]

    def run(self, n_steps: int, sync=None) -> Dict[str, float]:
        if sync is not None:
            sync()
        t0 = time.time()
        for _ in range(n_steps):
            self.step()
        if sync is not None:
            sync()
        wall = time.time() - t0
        n = self.env.n_envs
        out = {
            "time_per_step": wall / max(n_steps, 1),
            "steps_per_second": n_steps / max(wall, 1e-12),               # per env, as the reference logs it
            "total_steps_per_second": n_steps * n / max(wall, 1e-12),     # x batch (inf_dummy_batch_size analogue)
            "n_envs": n, "n_steps": n_steps, "wall_s": wall,
        }
        if self.finished_returns:
            out["mean_reward"] = float(torch.cat(self.finished_returns).float().mean())
            out["mean_ep_length"] = float(torch.cat(self.finished_lengths).float().mean())
        return out


def evaluate_policy_batched(agent, env, n_eval_episodes: int = 10, target_return: Optional[float] = None,
                            reward_scale: Optional[float] = None, env_act_dim: Optional[int] = None,
                            callback: Optional[Callable[[dict, dict], None]] = None,
                            reward_threshold: Optional[float] = None, return_episode_rewards: bool = False,
                            task_id: int = 0, max_steps: Optional[int] = None,
                            is_success_buffer: Optional[List[float]] = None, park_finished: bool = False):
    """`custom_evaluate_policy` (src/callbacks/evaluation.py:14-271) over a vector env of any width.

    Episodes are divided over the sub-envs as evenly as possible (:94-96) and an env stops contributing once it
    has finished its share (:184,205-212); returns (mean_reward, std_reward, mean_episode_time), or the
    (episode_rewards, episode_lengths, episode_times) lists with `return_episode_rewards` (:266-271).
    `target_return` / `reward_scale` default to the agent's `compute_target_return_val` /
    `get_reward_scale_for_env` (:111-122); `agent.persist_context` selects the cross-episode mode; an env's
    `is_success` info at episode end is appended to `is_success_buffer` (the reference collects it through its
    `_log_success_callback`, custom_eval_callback.py:36-52).
    An agent with `use_inference_cache` False is driven in context-window mode (BatchedRollout._step_window): the previous
    step's scaled reward, the reset flag or -- with persist_context -- the relabel / keep of a finished episode go with every
    call; park_finished is refused there, before the first step (ValueError), unless the agent was created with
    window_slots="own" (every slot's window then has its own ring position, and a parked env's window waits with it).
    park_finished=True: an env that has finished its share is parked (agent.set_active) and the agent no longer steps it --
    the reference keeps forwarding it and throws the result away.  The env object still steps all its sub-envs, with action 0
    for the parked ones; rewards, lengths and counts equal those of park_finished=False (envs are independent)."""
    n = env.n_envs
    if target_return is None:
        target_return = agent.compute_target_return_val(env=env, task_id=task_id) * agent.get_reward_scale_for_env(None)
    if reward_scale is None:
        reward_scale = agent.get_reward_scale_for_env(None)
    # every env takes part from the first step on: an agent that comes out of an evaluation with parked envs (park_finished) starts
    # the next one with all of them active again
    if park_finished and not getattr(agent, "use_inference_cache", True) and getattr(agent, "window_slots", "shared") != "own":
        raise ValueError("evaluate_policy_batched: park_finished needs the inference cache; with use_inference_cache=False every "
                         "env slot is stepped (the window ring has one push position for the batch) unless the agent was "
                         'created with window_slots="own"')
    if hasattr(agent, "set_active") and len(agent.active) != n:
        agent.set_active(range(n))
    ro = BatchedRollout(agent, env, target_return, reward_scale, env_act_dim,
                        persist_context=bool(getattr(agent, "persist_context", False)))
    targets = np.array([(n_eval_episodes + i) // n for i in range(n)], dtype=int)
    counts = np.zeros(n, dtype=int)
    cur_r = np.zeros(n)
    cur_l = np.zeros(n, dtype=int)
    start = [time.time()] * n
    episode_rewards: List[float] = []
    episode_lengths: List[int] = []
    episode_times: List[float] = []
    is_success: List[float] = [] if is_success_buffer is None else is_success_buffer
    steps = 0
    while (counts < targets).any():
        ro.step()
        steps += 1
        reward = ro.last_reward.detach().cpu().numpy()
        done = ro.last_done.detach().cpu().numpy().astype(bool)
        info = getattr(env, "last_info", {}) or {}
        succ = info["is_success"].detach().cpu().numpy() if "is_success" in info else None
        cur_r += reward
        cur_l += 1
        for i in range(n):
            if counts[i] < targets[i]:
                if callback is not None:
                    callback(locals(), globals())
                if done[i]:
                    episode_rewards.append(float(cur_r[i]))
                    episode_lengths.append(int(cur_l[i]))
                    episode_times.append(time.time() - start[i])
                    if succ is not None:
                        is_success.append(float(succ[i]))
                    counts[i] += 1
            if done[i]:
                cur_r[i], cur_l[i], start[i] = 0.0, 0, time.time()
        if park_finished:
            active = [i for i in range(n) if counts[i] < targets[i]]
            if active and len(active) != len(agent.active):
                agent.set_active(active)
        if max_steps is not None and steps >= max_steps:
            break
    # evaluation.py:258-261: the cache is dropped when the evaluation ends
    if hasattr(agent, "inference_params"):
        agent.inference_params.reset()
    mean_reward = float(np.mean(episode_rewards)) if episode_rewards else float("nan")
    std_reward = float(np.std(episode_rewards)) if episode_rewards else float("nan")
    if reward_threshold is not None:
        assert mean_reward > reward_threshold, f"Mean reward below threshold: {mean_reward:.2f} < {reward_threshold:.2f}"
    if return_episode_rewards:
        return episode_rewards, episode_lengths, episode_times
    return mean_reward, std_reward, float(np.mean(episode_times)) if episode_times else float("nan")


def eval_log_record(prefix: str, env_name: str, idx: int, episode_rewards, episode_lengths, episode_times=None,
                    is_success=None, inf_batch: Optional[int] = None, num_envs: int = 1,
                    score_ref: Optional[Sequence[float]] = None, score_type: str = "dns") -> Dict[str, float]:
    """The keys `_on_step_logging` records for one evaluated env (custom_eval_callback.py:446-508).
    `score_ref` = (random, data-or-human) reference returns of that env for the normalised score
    (src/envs/dn_scores.py:484-488, hn_scores.py:129-133); `inf_batch` = env slots advanced per step."""
    env_id = f"{env_name}_{idx}"
    mean_reward, mean_len = float(np.mean(episode_rewards)), float(np.mean(episode_lengths))
    rec = {f"{prefix}/{env_id}/mean_reward": mean_reward, f"{prefix}/{env_id}/mean_ep_length": mean_len}
    if episode_times is not None and len(episode_times) > 0:
        t = float(np.mean(episode_times))
        rec[f"{prefix}/{env_id}/mean_ep_time"] = t
        rec[f"{prefix}/{env_id}/time_per_step"] = t / (mean_len + 1e-8)
        rec[f"{prefix}/{env_id}/steps_per_second"] = mean_len / (t + 1e-8)
        if inf_batch is not None:
            rec[f"{prefix}/{env_id}/total_steps_per_second"] = mean_len * inf_batch / (t + 1e-8)
    if num_envs == 1:
        rec[f"{prefix}/mean_reward"] = mean_reward
        rec[f"{prefix}/mean_ep_length"] = mean_len
    if is_success is not None and len(is_success) > 0:
        sr = float(np.mean(is_success))
        rec[f"{prefix}/{env_id}/success_rate"] = sr
        if num_envs == 1:
            rec[f"{prefix}/success_rate"] = sr
    if score_ref is not None:
        rnd, ref = float(score_ref[0]), float(score_ref[1])
        score = float(np.mean((np.asarray(episode_rewards, dtype=np.float64) - rnd) / (ref - rnd)))
        rec[f"{prefix}/{env_id}/{score_type}"] = score
        if num_envs == 1:
            rec[f"{prefix}/{score_type}"] = score
    return rec


def score_loss(result, valid, act_mask=None, reduction: str = "reference") -> torch.Tensor:
    """The action loss of scored trajectories: `result` is what Engine.score / RecurrentAgent.score_trajectories returned (or
    its logp tensor [B, L, act_dim]); the per-entry loss is -logp, the cross-entropy of the recorded token.  `valid` [B, L]
    (the reference's attention_mask), `act_mask` [B, L, act_dim] or [B, act_dim] (its action_mask: the action dims the env
    uses; None = all).
      "reference": universal_decision_transformer_sb3.py:422-434 with an un-reduced loss function -- per valid timestep the
                   masked mean along the action dims, sum(loss * mask) / (sum(mask) + 1e-8), then the mean over the valid
                   timesteps (a timestep whose action mask is all zero counts with loss 0);
      "mean":      the plain mean over the valid, unmasked entries (the reference's reduced loss functions).
    Pure torch, any device; entries that are masked out never reach the sum (a -inf there does no harm)."""
    logp = getattr(result, "logp", result)
    if logp is None:
        raise ValueError("score_loss: the result holds no logp (score with \"logp\" in want and a target)")
    if logp.dim() != 3:
        raise ValueError(f"score_loss: logp must be [B, L, act_dim], got {tuple(logp.shape)}")
    B, L, A = logp.shape
    valid = torch.as_tensor(valid, device=logp.device).reshape(B, L) > 0
    if act_mask is None:
        mask = torch.ones(B, L, A, dtype=torch.bool, device=logp.device)
    else:
        mask = torch.as_tensor(act_mask, device=logp.device) > 0
        mask = (mask.reshape(B, 1, A) if mask.dim() == 2 else mask.reshape(B, L, A)).expand(B, L, A)
    loss = torch.where(mask, -logp, torch.zeros_like(logp))[valid]     # [n_valid, A]
    m = mask[valid].to(logp.dtype)
    if reduction == "reference":
        return (loss.sum(dim=1) / (m.sum(dim=-1) + 1e-8)).mean()
    if reduction == "mean":
        return loss.sum() / m.sum()
    raise ValueError(f'score_loss: reduction must be "reference" or "mean", got {reduction!r}')
