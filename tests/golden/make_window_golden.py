#!/usr/bin/env python3
"""Generate tests/golden/window_trace.npz: what the reference's cache-off evaluation feeds its model, step by step.

Run in the build container only (needs a read-only checkout of the reference at /root/reference; never on the GPU box):
    python tests/golden/make_window_golden.py

EXECUTED from the reference, on a stand-in `self` (their module needs gym / stable_baselines3, which are not installable here):
  * DecisionTransformerSb3.predict and .pad_inputs (src/algos/decision_transformer_sb3.py:621-691): the [-context_len:] slicing,
    the left padding with zeros, the zero-padding of the state to max_state_dim and the normalisation AFTER the padding;
  * discount_cumsum_torch (src/buffers/buffer_utils.py:23-28).
RESTATED here, because custom_evaluate_policy cannot be executed offline (it needs a gym VecEnv, stable_baselines3's type checks
and the env-name tables): the bookkeeping of its loop, src/callbacks/evaluation.py:130-251, for its one env -- append action /
reward placeholders, predict, step the env, rewards[-1] = reward / scale, append state / target return / timestep unless done, the
"safeguard" pruning (:172-177), and at an episode end either the fresh start (:238-246) or, with persist_context, the cutoff
(:215-217), the reconstruction of the target returns (:219-222) and the pruning (:223-224) followed by the reset state (:226-237).
Restated in this file's own terms -- one list of per-timestep records (observation, return-to-go, reward, timestep) where the
reference keeps parallel tensors -- with the same effect on what predict is handed at every step.

Recorded per step: the padded (states, returns_to_go, rewards) that reach get_action_pred, and the attention mask.  Only inputs
and outputs are stored -- no reference source text.  The trace is scripted: three episodes of 3, 6 and 2 steps and 3 steps of a
fourth, context_len 4 (the second episode is longer than the window), native observations of 3 dims padded to 5, rewards that
are multiples of 0.25 and a reward scale of 2, so every number is exact in float32 and the comparison can be bit for bit.

SECURITY NOTE: this generator `exec`s code taken from /root/reference; run it only in a throw-away build container.
"""
import ast
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

K, OBS_DIM, STATE_DIM, ACT_DIM = 4, 3, 5, 2
EPISODES = [3, 6, 2, 3]          # the last one is cut off (never done)
TARGET, SCALE = 12.0, 2.0
MEAN = [0.5, -0.25, 0.0, 1.0, -1.0]
STD = [2.0, 0.5, 1.0, 4.0, 0.25]


def _exec_methods(path, class_name, names):
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name)
    keep = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"torch": torch}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def _exec_functions(path, names):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def script():
    """Per env-step: (observation after the step [OBS_DIM], reward, done); and the first observation."""
    g = torch.Generator().manual_seed(7)
    obs = lambda: (torch.randint(-8, 9, (OBS_DIM,), generator=g).float() / 4).numpy()
    first, steps = obs(), []
    for ep, n in enumerate(EPISODES):
        for t in range(n):
            reward = float(torch.randint(-2, 7, (1,), generator=g)) / 4
            steps.append((obs(), reward, t == n - 1 and ep < len(EPISODES) - 1))
    return first, steps


def run(persist_context, seqs_per_sample):
    ns = _exec_methods(os.path.join(REF, "src/algos/decision_transformer_sb3.py"), "DecisionTransformerSb3", ["predict", "pad_inputs"])
    discount_cumsum_torch = _exec_functions(os.path.join(REF, "src/buffers/buffer_utils.py"), ["discount_cumsum_torch"])["discount_cumsum_torch"]
    rec = []

    def get_action_pred(policy, states, actions, rewards, returns_to_go, timesteps, attention_mask, deterministic, prompt, **kw):
        rec.append((states[0].clone(), returns_to_go[0, :, 0].clone(), rewards[0, :, 0].clone(), attention_mask[0].clone()))
        return torch.zeros(ACT_DIM), None

    Fake = type("Fake", (), {n: ns[n] for n in ("predict", "pad_inputs")})
    model = Fake()
    model.__dict__.update(dict(
        transforms=None, device=torch.device("cpu"), state_mean=torch.tensor(MEAN), state_std=torch.tensor(STD), s_proj_dim=None,
        a_proj_dim=None, s_proj_raw=False, reset_inf_cache_freq=None, get_action_pred=get_action_pred, policy=None,
        replay_buffer=SimpleNamespace(max_state_dim=STATE_DIM, max_act_dim=ACT_DIM, seqs_per_sample=seqs_per_sample),
        eval_context_len=K, persist_context=persist_context))
    first_obs, steps = script()
    # ---- the loop's bookkeeping, restated: ONE list of per-timestep records {obs, rtg, reward, t} instead of the reference's
    # parallel tensors.  The record of the timestep under way is the last one; its reward is 0 until the env has answered.
    context, ep_lengths = [], []

    def open_timestep(obs, rtg, t):
        context.append({"obs": torch.from_numpy(obs).float(), "rtg": float(rtg), "reward": 0.0, "t": t})

    def ask_model():
        """What the loop hands predict: every stored state, return-to-go and timestep, an action row and a reward per state."""
        n = len(context)
        model.predict(model.policy, torch.stack([c["obs"] for c in context]), torch.zeros(n, ACT_DIM),
                      torch.tensor([c["reward"] for c in context], dtype=torch.float32),
                      torch.tensor([[c["rtg"] for c in context]], dtype=torch.float32),
                      torch.tensor([[c["t"] for c in context]], dtype=torch.long), state=None, episode_start=None, deterministic=True,
                      context_len=K, prompt=None, task_id=None, is_eval=True, env_act_dim=ACT_DIM)

    open_timestep(first_obs, TARGET / SCALE, 0)
    t_in_episode = 0
    for next_obs, reward, done in steps:
        ask_model()
        t_in_episode += 1
        context[-1]["reward"] = reward / SCALE                                     # the env's answer, scaled
        if not done:
            open_timestep(next_obs, context[-1]["rtg"] - reward / SCALE, t_in_episode)
            if not persist_context and len(context) > 3 * K + 1:                     # the loop's guard against unbounded growth
                del context[:-(K + 1)]
            continue
        ep_lengths.append(t_in_episode)
        if persist_context:
            # returns actually obtained: the reference's discount_cumsum_torch over EVERY stored reward (gamma 1), older episodes'
            # entries included; then only the newest `cutoff` timesteps stay
            obtained = discount_cumsum_torch(torch.tensor([c["reward"] for c in context], dtype=torch.float32), 1)
            for c, g in zip(context, obtained.tolist()):
                c["rtg"] = g
            older = seqs_per_sample - 1
            cutoff = min(sum(ep_lengths[-older:]), K) if older > 0 else K
            del context[:-cutoff]
        else:
            context.clear()
        open_timestep(next_obs, TARGET / SCALE, 0)
        t_in_episode = 0
    return rec


def main():
    first_obs, steps = script()
    out = {"first_obs": first_obs.astype(np.float32), "obs": np.stack([s[0] for s in steps]).astype(np.float32),
           "reward": np.array([s[1] for s in steps], dtype=np.float32), "done": np.array([s[2] for s in steps], dtype=np.uint8),
           "state_mean": np.array(MEAN, dtype=np.float32), "state_std": np.array(STD, dtype=np.float32)}
    for name, persist, sps in (("plain", False, 1), ("persist_sps1", True, 1), ("persist_sps2", True, 2), ("persist_sps3", True, 3)):
        rec = run(persist, sps)
        out[name + "_states"] = torch.stack([r[0] for r in rec]).numpy().astype(np.float32)
        out[name + "_returns_to_go"] = torch.stack([r[1] for r in rec]).numpy().astype(np.float32)
        out[name + "_rewards"] = torch.stack([r[2] for r in rec]).numpy().astype(np.float32)
        out[name + "_attention_mask"] = torch.stack([r[3] for r in rec]).numpy().astype(np.uint8)
    meta = {"context_len": K, "obs_dim": OBS_DIM, "state_dim": STATE_DIM, "act_dim": ACT_DIM, "episodes": EPISODES,
            "target_return": TARGET, "reward_scale": SCALE,
            "executed_from_reference": ["DecisionTransformerSb3.predict", "DecisionTransformerSb3.pad_inputs",
                                        "buffer_utils.discount_cumsum_torch"],
            "restated_in_generator": "src/callbacks/evaluation.py:98-251 (custom_evaluate_policy's loop bookkeeping; the function "
                                     "needs gym / stable_baselines3 and a VecEnv and cannot be executed offline)"}
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "window_trace.npz"), **out)
    print("wrote window_trace.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
