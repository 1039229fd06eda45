#!/usr/bin/env python3
"""Generate tests/golden/reference_vectors.json by EXECUTING the reference's own importable files.

Run in the build container only (needs /root/reference; never on the GPU box):
    python tests/golden/make_golden_from_reference.py
Importable pieces of the hot path: the action tokenizer package
`src/tokenizers_custom` (MinMaxTokenizer with shift, used at multi_domain_discrete_dt_model.py:56-60)
and `src/algos/models/rms_norm.py` (LlamaRMSNorm, used at decision_xlstm.py:190-191).  Everything else on
the path needs gym / stable_baselines3 / xlstm / mamba_ssm, which are not installable here.
Only inputs and outputs are stored -- no reference source text.

SECURITY NOTE: this generator `exec`s code taken from /root/reference (named classes, functions and top-level assignments of
its files), i.e. it runs untrusted third-party code with the privileges of whoever regenerates the fixtures.  Run it only
in a throw-away build container on a read-only checkout of the reference (as here), never on a developer machine with
credentials and never on the GPU box; nothing in tests/, bench.py or the product package imports or executes it.
"""
import importlib.util
import json
import os
import sys

import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def _exec_pieces(path, names):
    """Execute only the named top-level assignments / functions of a reference file (its imports need robosuite /
    dmc2gym, which are absent): the observation-space tables and `map_flattened_obs_to_full_space`."""
    import ast
    import numpy as np
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body
            if (isinstance(n, ast.Assign) and any(getattr(t, "id", None) in names for t in n.targets))
            or (isinstance(n, ast.FunctionDef) and n.name in names)]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def obs_full_space_vectors(g):
    """Inputs / outputs of the reference's flattened-observation -> full-space mapping for one DMControl and one
    Mimicgen observation spec (src/envs/dmcontrol_utils.py:35-78, src/envs/mimicgen_utils.py:58-78,199-214)."""
    import numpy as np
    out = {}
    cases = {
        "dmc_cheetah_run": ("src/envs/dmcontrol_utils.py", ["DMC_OBSTYPE_TO_DIM", "DMC_FULL_OBS_DIM", "DMC_OBSTYPE_TO_STARTIDX"],
                            [("position", 8), ("velocity", 9)]),
        "dmc_walker_walk": ("src/envs/dmcontrol_utils.py", ["DMC_OBSTYPE_TO_DIM", "DMC_FULL_OBS_DIM", "DMC_OBSTYPE_TO_STARTIDX"],
                            [("orientations", 14), ("height", 1), ("velocity", 9)]),
        "mimicgen_main_lowdim": ("src/envs/mimicgen_utils.py",
                                 ["MIMICGEN_OBSTYPE_TO_DIM", "MIMICGEN_FULL_OBS_DIM", "MIMICGEN_OBSTYPE_TO_STARTIDX"],
                                 [("robot0_eef_pos", 3), ("robot0_eef_quat", 4), ("robot0_gripper_qpos", 2), ("object", 23)]),
    }
    for name, (rel, tables, spec) in cases.items():
        ns = _exec_pieces(os.path.join(REF, rel), tables + ["map_flattened_obs_to_full_space"])
        n = sum(d for _, d in spec)
        x = (torch.rand(4, n, generator=g) * 2 - 1).numpy().astype(np.float32)
        obs_spec = {k: np.zeros(d, dtype=np.float32) for k, d in spec}   # the function reads .shape of each entry
        full = ns["map_flattened_obs_to_full_space"](x, obs_spec)
        dims = ns[tables[0]]
        out[name] = {"spec": [[k, d] for k, d in spec], "x": x.tolist(), "full": np.asarray(full, dtype=np.float32).tolist(),
                     "full_dim": int(ns[tables[1]]), "obstype_to_dim": {k: int(v) for k, v in dims.items()}}
    return out


def _exec_methods(path, class_name, names):
    """Execute only the named methods of one class of a reference file as plain functions (the module's imports
    need gym / stable_baselines3)."""
    import ast
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name)
    keep = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"torch": torch}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def action_from_logits_vectors(g, tok):
    """Head post-processing of the multi-domain model, executed from the reference with a stand-in `self`
    (multi_domain_discrete_dt_model.py:83-108: prepare_action_logits + get_action_from_logits; shared action head,
    8 x 274 logits, 18 discrete actions, min-max tokenizer with shift 18)."""
    from types import SimpleNamespace
    ns = _exec_methods(os.path.join(REF, "src/algos/models/multi_domain_discrete_dt_model.py"),
                       "MultiDomainDiscreteDTModel", ["get_action_from_logits", "prepare_action_logits"])
    me = SimpleNamespace(discrete_actions=18, tokenize_a=True, tok_a_target_only=False, shared_a_head=True,
                         num_actions=274, action_channels=256, config=SimpleNamespace(act_dim=8),
                         inv_tokenize_actions=lambda a: tok.inv_tokenize(a))
    B = 6
    raw = torch.randn(B, 1, 1, 8 * 274, generator=g)          # action_net output at the one prediction position
    cont = ns["get_action_from_logits"](me, ns["prepare_action_logits"](me, raw.clone(), is_discrete=False), is_discrete=False)
    disc = ns["get_action_from_logits"](me, ns["prepare_action_logits"](me, raw.clone(), is_discrete=True), is_discrete=True)
    return {"logits": raw.reshape(B, -1).tolist(), "continuous": cont.reshape(B, 8).tolist(),
            "discrete": disc.reshape(B).tolist()}


def token_front_end_vectors(g):
    """(state, return-to-go, reward) token construction with the inference cache on, executed from the reference
    (online_decision_transformer_model.py:463-530 compute_inputs / embed_inputs, :287-311 getters, :545-612
    construct_inputs_and_masks / prepare_inputs_and_masks) on a stand-in `self` that carries plain nn modules with
    the multi_domain model kwargs (reward_condition, rtg_condition, no action tokens, no time embeddings)."""
    import torch.nn as nn
    names = ["compute_inputs", "embed_inputs", "construct_inputs_and_masks", "prepare_inputs_and_masks",
             "get_state_embeddings", "get_return_embeddings", "get_reward_embeddings"]
    ns = _exec_methods(os.path.join(REF, "src/algos/models/online_decision_transformer_model.py"),
                       "OnlineDecisionTransformerModel", names)
    D, S, B, T = 16, 204, 3, 4
    Fake = type("Fake", (), {n: ns[n] for n in names})
    me = Fake()
    torch.manual_seed(11)
    me.embed_state, me.embed_return, me.embed_rewards = nn.Linear(S, D), nn.Linear(1, D), nn.Linear(1, D)
    me.embed_ln = nn.LayerNorm(D)
    with torch.no_grad():
        me.embed_ln.weight.copy_(torch.randn(D) * 0.3 + 1.0)
        me.embed_ln.bias.copy_(torch.randn(D) * 0.1)
    me.get_action_embeddings = lambda a, attention_mask=None: None
    me.rtg_condition, me.reward_condition, me.action_condition = True, True, False
    me.use_time_embds, me.symlog_transform, me.img_is_encoded, me.separate_ln = False, False, False, False
    me.training, me.p_mask, me.p_token_drop, me.hidden_size = False, 0, 0, D
    me.config = type("Cfg", (), {"add_cross_attention": False, "hidden_size": D})()
    states = torch.rand(B, T, S, generator=g) * 2 - 1
    actions = torch.zeros(B, T, 8)
    rtg = torch.rand(B, T, 1, generator=g) * 5
    rewards = torch.rand(B, T, 1, generator=g)
    timesteps = torch.arange(T).repeat(B, 1)
    mask = torch.ones(B, T, dtype=torch.long)
    with torch.no_grad():
        _, stacked, smask = me.compute_inputs(states, actions, rtg, rewards, timesteps, mask, use_inference_cache=True)
    sd = {"embed_state.weight": me.embed_state.weight, "embed_state.bias": me.embed_state.bias,
          "embed_return.weight": me.embed_return.weight, "embed_return.bias": me.embed_return.bias,
          "embed_rewards.weight": me.embed_rewards.weight, "embed_rewards.bias": me.embed_rewards.bias,
          "embed_ln.weight": me.embed_ln.weight, "embed_ln.bias": me.embed_ln.bias}
    return {"state_dict": {k: v.detach().tolist() for k, v in sd.items()},
            "states": states.tolist(), "returns_to_go": rtg.tolist(), "rewards": rewards.tolist(),
            "stacked_inputs": stacked.tolist(), "stacked_attention_mask": smask.tolist(),
            "tok_to_pred_pos": dict(me.tok_to_pred_pos), "tok_to_pos": dict(me.tok_to_pos)}


def impala_cnn_vectors(g):
    """The reference's ImpalaCNNBlock / ImpalaCNNResidual modules (src/algos/models/image_encoders.py:76-131), executed
    as they are; chained as ImpalaCNN.__init__/forward chain them (:39-66: 16 / 32 / 32 channels, ReLU, Flatten,
    Linear, ReLU) -- the ImpalaCNN class itself derives from stable_baselines3's BaseFeaturesExtractor, which is absent.
    Weights, one uint8 batch and the outputs go to tests/golden/impala_cnn_reference.npz."""
    import ast
    import numpy as np
    import torch.nn as nn
    path = os.path.join(REF, "src/algos/models/image_encoders.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("ImpalaCNNResidual", "ImpalaCNNBlock")]
    ns = {"torch": torch, "nn": nn}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    torch.manual_seed(21)
    ident = lambda p: p
    cnn = nn.ModuleList([ns["ImpalaCNNBlock"](3, 16, norm_func=ident), ns["ImpalaCNNBlock"](16, 32, norm_func=ident),
                         ns["ImpalaCNNBlock"](32, 32, norm_func=ident)])
    D = 24
    linear = nn.Sequential(nn.Linear(32 * 8 * 8, D), nn.ReLU())
    img = torch.randint(0, 256, (2, 3, 64, 64), generator=g, dtype=torch.uint8)
    with torch.no_grad():
        x = img.float() / 255.0                      # online_decision_transformer_model.py:523-525
        per_block = []
        for block in cnn:
            x = block(x)
            per_block.append(x.clone())
        out = linear(nn.Flatten()(torch.relu(x)))
    arrays = {"images": img.numpy(), "out": out.numpy(), "block2": per_block[2].numpy()}
    for k, v in cnn.state_dict().items():
        arrays["embed_image.cnn." + k] = v.numpy()
    for k, v in linear.state_dict().items():
        arrays["embed_image.linear." + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "impala_cnn_reference.npz"), **arrays)
    print("wrote", os.path.join(HERE, "impala_cnn_reference.npz"))


def agent_predict_trace(g):
    """`agent.predict` -> `pad_inputs` -> `get_action_pred` executed from the reference over a short rollout, on a
    stand-in `self` and with a recording stand-in for the policy network (decision_transformer_sb3.py:621-667,
    algos/decision_xlstm.py:11-28, discrete_decision_transformer_sb3.py:13-72; the loop around it follows
    callbacks/evaluation.py:130-177).  Stores what the policy network is handed at every step (padded, normalised
    states; returns-to-go; reward tokens; whether the cache had been dropped) and what `predict` returns."""
    from types import SimpleNamespace
    fns = {}
    fns.update(_exec_methods(os.path.join(REF, "src/algos/decision_transformer_sb3.py"), "DecisionTransformerSb3", ["predict"]))
    fns.update(_exec_methods(os.path.join(REF, "src/algos/decision_xlstm.py"), "DecisionXLSTM", ["pad_inputs"]))
    fns.update(_exec_methods(os.path.join(REF, "src/algos/discrete_decision_transformer_sb3.py"),
                             "DiscreteDecisionTransformerSb3", ["get_action_pred"]))
    obs_dim, env_act_dim, steps, freq = 39, 4, 8, 3          # Meta-World shaped: 39 -> 204, 4 of 8 action dims
    Fake = type("Fake", (), {k: fns[k] for k in ("predict", "pad_inputs", "get_action_pred")})
    me = Fake()
    me.transforms, me.s_proj_dim, me.a_proj_dim, me.s_proj_raw = None, None, None, False
    me.state_mean = torch.randn(204, generator=g) * 0.1
    me.state_std = torch.rand(204, generator=g) + 0.5
    me.reset_inf_cache_freq, me.past_key_values, me.use_inference_cache = freq, None, True
    me.ddp_kwargs, me.target_return_type, me.a_sample_kwargs = {}, "predefined", None
    me.use_amp, me.amp_dtype, me.device = False, torch.bfloat16, torch.device("cpu")
    me.replay_buffer = SimpleNamespace(max_state_dim=204, max_act_dim=8)
    me.policy = SimpleNamespace(tok_a_target_only=False, shared_a_head=True)
    canned = torch.rand(steps, 8, generator=g) * 2 - 1
    seen = []

    def policy(**inputs):
        t = len(seen)
        seen.append({"states": inputs["states"].clone(), "returns_to_go": inputs["returns_to_go"].clone(),
                     "rewards": inputs["rewards"].clone(), "cache_is_none": inputs["past_key_values"] is None,
                     "use_inference_cache": bool(inputs["use_inference_cache"])})
        T = inputs["actions"].shape[1]
        return SimpleNamespace(action_preds=canned[t].expand(1, T, 8).clone(), past_key_values=f"kv{t}")

    # the rollout bookkeeping of custom_evaluate_policy (evaluation.py:104-177), single env, no episode end
    obs_all = torch.rand(steps + 1, obs_dim, generator=g) * 2 - 1
    env_rewards = torch.rand(steps, generator=g)
    reward_scale = 200.0
    states = obs_all[:1].clone()
    actions = torch.zeros((0, env_act_dim))
    rewards = torch.zeros(0)
    target_return = torch.tensor(6.5).reshape(1, 1)
    timesteps = torch.tensor(0).reshape(1, 1)
    returned = []
    for t in range(steps):
        actions = torch.cat([actions, torch.zeros((1, env_act_dim))], dim=0)
        rewards = torch.cat([rewards, torch.zeros(1)])
        a, _ = me.predict(policy, states, actions, rewards, target_return, timesteps, state=None, episode_start=None,
                          deterministic=True, context_len=1, prompt=None, task_id=None, is_eval=True,
                          env_act_dim=env_act_dim)
        returned.append(a.clone())
        actions[-1] = a
        rewards[-1] = env_rewards[t] / reward_scale
        states = torch.cat([states, obs_all[t + 1: t + 2]], dim=0)
        target_return = torch.cat([target_return, (target_return[0, -1] - env_rewards[t] / reward_scale).reshape(1, 1)], dim=1)
        timesteps = torch.cat([timesteps, torch.ones((1, 1), dtype=torch.long) * (t + 1)], dim=1)
    return {"obs": obs_all.tolist(), "env_rewards": env_rewards.tolist(), "reward_scale": reward_scale,
            "target_return0": 6.5, "env_act_dim": env_act_dim, "reset_inf_cache_freq": freq,
            "state_mean": me.state_mean.tolist(), "state_std": me.state_std.tolist(), "canned_action_preds": canned.tolist(),
            "policy_saw": [{"state_last": s["states"][0, -1].tolist(), "n_states": int(s["states"].shape[1]),
                            "rtg_last": float(s["returns_to_go"][0, -1, 0]), "reward_last": float(s["rewards"][0, -1, 0]),
                            "cache_is_none": s["cache_is_none"]} for s in seen],
            "returned_actions": [a.tolist() for a in returned]}


def mamba_agent_trace():
    """The reference's Mamba rollout control flow, executed: `DiscreteDecisionMamba.get_action_pred`
    (src/algos/decision_mamba.py:76-127: one `policy(**inputs)` per action dim with the cache on, action dim i read from
    forward i), the `InferenceParams` dataclass with its `reset()` (:8-25) and `MambaEncoder.forward`
    (src/algos/models/decision_mamba.py:109-166: per-layer choice between the full call and the per-token loop,
    `seqlen_offset` bumped inside the layer loop), over two envs x two episodes with `inference_params.reset()` at the
    episode end as custom_evaluate_policy does (src/callbacks/evaluation.py:248-251).

    mamba_ssm is absent, so each encoder layer is a stand-in that restates what [3P] mamba_ssm Block + Mamba.forward do
    with an `inference_params` (add -> RMSNorm -> mixer; `_get_states_from_cache` allocates zero conv / ssm states for
    an unseen layer_idx; seqlen_offset > 0: `step()` on the cached states in place; seqlen_offset == 0: the
    full-sequence path from an EMPTY state whose final conv / ssm states overwrite the cache) around the oracle's
    `mamba_step` mixer math.  What this vector pins is therefore the reference's control flow -- which layers restart,
    how often the state advances per env-step, which forward each action dim comes from -- not the mixer arithmetic.
    Stored: inputs, the weight seed, and the actions `get_action_pred` returned."""
    import ast
    from dataclasses import dataclass, field
    from types import SimpleNamespace
    from typing import Optional, Tuple, Union
    from transformers.modeling_outputs import BaseModelOutputWithPastAndCrossAttentions
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from lram_amd import init_state_dict, preset
    from oracle import dt_ref, mamba_ref

    # --- reference code, executed ---
    path = os.path.join(REF, "src/algos/decision_mamba.py")
    tree = ast.parse(open(path).read())
    ip_cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "InferenceParams")
    ns = {"dataclass": dataclass, "field": field}
    exec(compile(ast.Module(body=[ip_cls], type_ignores=[]), path, "exec"), ns)
    InferenceParams = ns["InferenceParams"]
    gap_ns = {"torch": torch, "sample_from_logits": None}
    gcls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DiscreteDecisionMamba")
    gfn = [n for n in gcls.body if isinstance(n, ast.FunctionDef) and n.name == "get_action_pred"]
    exec(compile(ast.Module(body=gfn, type_ignores=[]), path, "exec"), gap_ns)
    path2 = os.path.join(REF, "src/algos/models/decision_mamba.py")
    tree2 = ast.parse(open(path2).read())
    ecls = next(n for n in tree2.body if isinstance(n, ast.ClassDef) and n.name == "MambaEncoder")
    efn = [n for n in ecls.body if isinstance(n, ast.FunctionDef) and n.name == "forward"]
    enc_ns = {"torch": torch, "Optional": Optional, "Tuple": Tuple, "Union": Union, "RMSNorm": type(None),
              "rms_norm_fn": None, "layer_norm_fn": None,
              "BaseModelOutputWithPastAndCrossAttentions": BaseModelOutputWithPastAndCrossAttentions}
    exec(compile(ast.Module(body=efn, type_ignores=[]), path2, "exec"), enc_ns)

    seed, env_act_dim, B = 7, 3, 2
    spec = preset("mamba_tiny")
    sd = init_state_dict(spec, seed=seed)

    class Layer:  # [3P] mamba_ssm Block (fused_add_norm off, fp32 residual) + Mamba.forward with inference_params
        def __init__(self, idx):
            self.idx, self.p = idx, f"encoder.layers.{idx}."

        def __call__(self, hidden_states, residual=None, inference_params=None):
            residual = hidden_states + residual if residual is not None else hidden_states
            x = mamba_ref.rms_norm(residual, sd[self.p + "norm.weight"], spec.norm_eps)
            cache = inference_params.key_value_memory_dict
            if self.idx not in cache:
                cache[self.idx] = (torch.zeros(1, spec.d_inner, spec.d_conv), torch.zeros(1, spec.d_inner, spec.d_state))
            conv, ssm = cache[self.idx]
            if inference_params.seqlen_offset > 0:
                assert x.shape[1] == 1
                o, c, s = mamba_ref.mamba_step(sd, self.p + "mixer.", x[:, 0], conv, ssm, spec.dt_rank, spec.d_state)
                conv.copy_(c), ssm.copy_(s)
                return o.unsqueeze(1), residual
            c, s, outs = torch.zeros_like(conv), torch.zeros_like(ssm), []
            for t in range(x.shape[1]):
                o, c, s = mamba_ref.mamba_step(sd, self.p + "mixer.", x[:, t], c, s, spec.dt_rank, spec.d_state)
                outs.append(o)
            conv.copy_(c), ssm.copy_(s)
            return torch.stack(outs, dim=1), residual

    Enc = type("Enc", (), {"forward": enc_ns["forward"]})
    enc = Enc()
    enc.layers = [Layer(i) for i in range(spec.n_blocks)]
    enc.config = SimpleNamespace(fused_add_norm=False, residual_in_fp32=True)
    enc.norm_f = lambda r: mamba_ref.rms_norm(r, sd["encoder.norm_f.weight"], spec.norm_eps)
    enc.norm_f.weight = sd["encoder.norm_f.weight"]

    def make_policy():
        def policy(**inputs):  # cache on: only the last timestep is embedded (online_decision_transformer_model.py:466-470)
            x = dt_ref.embed_tokens(spec, sd, inputs["states"][:, -1], inputs["returns_to_go"][:, -1, 0],
                                    inputs["rewards"][:, -1, 0])
            hidden = enc.forward(inputs_embeds=x, inference_params=inputs["inference_params"]).last_hidden_state
            act, _ = dt_ref.action_head(spec, sd, hidden[:, 1], False)
            return SimpleNamespace(action_preds=act.view(1, 1, -1), attentions=None, cross_attentions=None)
        return policy

    g = torch.Generator().manual_seed(99)
    steps = 7
    ep_end = [{3}, {2, 5}]  # env e: inference_params.reset() after these steps (episode ends)
    obs = torch.rand(steps, B, spec.state_dim, generator=g) * 2 - 1
    rtg = 4.0 - 0.05 * torch.arange(steps).float().view(-1, 1).expand(steps, B).contiguous()
    returned = torch.zeros(steps, B, env_act_dim)
    for e in range(B):
        me = SimpleNamespace(use_inference_cache=True, ddp_kwargs={}, target_return_type="predefined", use_amp=False,
                             amp_dtype=torch.bfloat16, num_timesteps=1, log_attn_maps=False, a_sample_kwargs=None,
                             inference_params=InferenceParams(max_seqlen=spec.max_length, max_batch_size=1))
        policy = make_policy()
        with torch.no_grad():
            for t in range(steps):
                a, _ = gap_ns["get_action_pred"](
                    me, policy, obs[t, e].view(1, 1, -1).clone(), torch.zeros(1, 1, spec.act_dim),
                    torch.zeros(1, 1, 1), rtg[t, e].view(1, 1, 1).clone(), torch.tensor([[t]]), torch.ones(1, 1),
                    True, None, is_eval=True, task_id=None, env_act_dim=env_act_dim)
                returned[t, e] = a
                if t in ep_end[e]:
                    me.inference_params.reset()
    return {"preset": "mamba_tiny", "weight_seed": seed, "env_act_dim": env_act_dim, "obs": obs.tolist(),
            "rtg": rtg.tolist(), "episode_end_after_step": [sorted(x) for x in ep_end],
            "returned_actions": returned.tolist()}


def load_model_weights_trace():
    """`DecisionTransformerSb3.load_model_weights` (src/algos/decision_transformer_sb3.py:1120-1184) executed on a
    stand-in `self`, with `load_from_zip_file` (stable_baselines3, absent) replaced by a function that returns a canned
    (data, params, variables) triple: for several `load_kwargs` / `compile` settings, which keys reach
    `policy.load_state_dict(..., strict=False)` and whether state_mean / state_std are taken over."""
    from types import SimpleNamespace
    keys = ["embed_state.weight", "embed_state.bias", "embed_ln.weight", "action_net.0.weight", "action_net.0.bias",
            "predict_state.weight", "predict_state.bias", "predict_return.weight", "predict_reward.bias",
            "embed_image.cnn.0.conv.weight", "embed_image.linear.0.bias", "encoder.layers.blocks.0.xlstm_norm.weight",
            "encoder.layers.blocks.1.xlstm.slstm_cell._recurrent_kernel_", "encoder.wpe.weight", "action_pred.0.weight",
            "encoder.module.odd.weight"]
    cases = []
    for prefix in ("", "module.", "_orig_mod.", "module._orig_mod.", "_orig_mod.module."):
        for load_kwargs in (None, {"load_action_head": False}, {"load_state_head": True}, {"exclude_heads": True},
                            {"img_encoder_only": True}):
            for compiled in (False, True):
                for with_vars in (True, False):
                    canned = {prefix + k: i for i, k in enumerate(keys)}
                    variables = {"state_mean": "MEAN", "state_std": "STD"} if with_vars else {}
                    got = {}

                    def load_state_dict(d, strict=True, got=got):
                        got["keys"], got["strict"] = list(d.keys()), strict
                        return [], []

                    ns = {"load_from_zip_file": lambda path, device=None, custom_objects=None:
                          ({}, {"policy": dict(canned)}, dict(variables)), "print": lambda *a, **k: None}
                    ns.update(_exec_methods(os.path.join(REF, "src/algos/decision_transformer_sb3.py"),
                                            "DecisionTransformerSb3", ["load_model_weights"]))
                    fn = ns["load_model_weights"]
                    fn.__globals__.update(ns)
                    me = SimpleNamespace(load_kwargs=load_kwargs, device="cpu", compile=compiled, state_mean=None,
                                         state_std=None, freeze_kwargs=None,
                                         policy=SimpleNamespace(load_state_dict=load_state_dict, num_task_heads=1,
                                                                global_pos_embds=True))
                    fn(me, "ckpt.zip")
                    cases.append({"prefix": prefix, "load_kwargs": load_kwargs, "compile": compiled,
                                  "with_variables": with_vars, "loaded_keys": got["keys"], "strict": got["strict"],
                                  "state_mean": me.state_mean, "state_std": me.state_std})
    return {"checkpoint_keys": keys, "cases": cases}


def checkpoint_key_names():
    """Names the checkpoint keys are built from, taken from code rather than recalled:
      * `self.<name> = ...` module attributes assigned in the reference's own model classes (AST walk over the class
        bodies: OnlineDecisionTransformerModel, DiscreteDTModel, MultiDomainDiscreteDTModel, ImpalaCNN, ImpalaCNNBlock,
        ImpalaCNNResidual, MambaEncoder, DecisionMambaModel, xLSTMEncoder, DecisionXLSTMModel);
      * the parameter names of transformers' DecisionTransformerModel (the HF base class the reference model derives
        from, `embed_*` / `predict_*` / `embed_ln`), by instantiating the installed class;
      * `make_head` executed: the action head is an nn.Sequential, hence `action_net.0.{weight,bias}`.
    The third-party backbone sub-keys (`xlstm.*`, `mixer.*`) cannot be derived offline and stay as recalled."""
    import ast
    import torch.nn as nn
    out = {}
    files = {"src/algos/models/online_decision_transformer_model.py": ["OnlineDecisionTransformerModel"],
             "src/algos/models/discrete_decision_transformer_model.py": ["DiscreteDTModel"],
             "src/algos/models/multi_domain_discrete_dt_model.py": ["MultiDomainDiscreteDTModel"],
             "src/algos/models/image_encoders.py": ["ImpalaCNN", "ImpalaCNNBlock", "ImpalaCNNResidual"],
             "src/algos/models/decision_mamba.py": ["MambaEncoder", "DecisionMambaModel"],
             "src/algos/models/decision_xlstm.py": ["xLSTMEncoder", "DecisionXLSTMModel"]}
    for rel, classes in files.items():
        tree = ast.parse(open(os.path.join(REF, rel)).read())
        for cls in [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in classes]:
            names = set()
            for node in ast.walk(cls):
                if isinstance(node, ast.Assign):
                    for t in node.targets:
                        if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self":
                            names.add(t.attr)
            out[cls.name] = sorted(names)
    from transformers import DecisionTransformerConfig, DecisionTransformerModel
    hf = DecisionTransformerModel(DecisionTransformerConfig(state_dim=4, act_dim=2, hidden_size=8, n_layer=1, n_head=1,
                                                            max_ep_len=8))
    out["hf_DecisionTransformerModel_params"] = sorted(k for k in hf.state_dict() if not k.startswith("encoder."))
    ns = _exec_methods(os.path.join(REF, "src/algos/models/online_decision_transformer_model.py"),
                       "OnlineDecisionTransformerModel", ["make_head"])
    make_head = ns["make_head"].__func__ if isinstance(ns["make_head"], staticmethod) else ns["make_head"]
    make_head.__globals__["nn"] = nn
    out["make_head_params"] = sorted(make_head(8, 6, 1).state_dict())
    return out


def reference_presets():
    """Every recurrent model preset of the reference's Hydra tree, parsed and resolved BY THE PACKAGE'S OWN LOADER from the
    reference's YAML files (configs/agent_params/multi_domain.yaml + huggingface/{xlstm,mamba}_*.yaml, the `${...}`
    interpolations included): the resolved `agent_params` dict of each preset is stored, so that
    tests/test_config_weights.py can check `spec_from_agent_params` (and the engine's geometry limits) against every
    configuration the reference ships -- without the reference tree at test time.  Values only, no YAML text."""
    import glob
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from lram_amd.config import load_agent_params
    cfg_dir = os.path.join(REF, "configs")
    out = {}
    for path in sorted(glob.glob(os.path.join(cfg_dir, "agent_params", "huggingface", "*.yaml"))):
        name = os.path.splitext(os.path.basename(path))[0]
        if not (name.startswith("xlstm_") or name.startswith("mamba_")):
            continue
        kind = "MDDXLSTM" if name.startswith("xlstm_") else "MDDMamba"
        ap = load_agent_params(cfg_dir, "multi_domain", [f"agent_params/huggingface={name}", f"agent_params.kind={kind}"])
        out[name] = {k: ap.get(k) for k in ("kind", "huggingface", "model_kwargs", "replay_buffer_kwargs")}
    return json.loads(json.dumps(out, default=lambda o: list(o) if isinstance(o, (tuple, set)) else str(o)))


def evaluate_policy_trace(g):
    """`custom_evaluate_policy` (src/callbacks/evaluation.py:14-271) EXECUTED over three episodes of a scripted
    single-env VecEnv, with stand-ins for what its module imports (gym.spaces, the SB3 VecEnv helpers, extract_env_name)
    and a recording stand-in for the agent.  Stored: the scripted observations / rewards / episode ends, and per
    `model.predict` call what the loop handed over (the last observation, the last return-to-go, the timestep, how many
    states the context held), when the loop dropped the inference cache, and the function's results -- the contract
    lram_amd.rollout.evaluate_policy_batched keeps for vector envs of any width."""
    import ast
    import time as _time
    import warnings as _warnings
    from types import SimpleNamespace
    import numpy as np
    path = os.path.join(REF, "src/callbacks/evaluation.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "custom_evaluate_policy"]

    class Discrete:  # gym.spaces.Discrete
        pass

    class VecEnv:
        pass

    obs_dim, act_dim, ep_lens, reward_scale, target = 6, 3, (4, 2, 3), 50.0, 90.0
    n_steps = sum(ep_lens)
    obs_all = (torch.rand(n_steps + 1, obs_dim, generator=g) * 2 - 1).numpy().astype(np.float32)
    rew_all = torch.rand(n_steps, generator=g).numpy().astype(np.float32) * 10
    ends = set(np.cumsum(ep_lens) - 1)

    class Env(VecEnv):
        num_envs = 1
        observation_space = SimpleNamespace(shape=(obs_dim,))
        action_space = SimpleNamespace(shape=(act_dim,))

        def __init__(self):
            self.t, self.ep_r, self.ep_l = 0, 0.0, 0

        def env_is_wrapped(self, _cls):
            return [True]

        def reset(self):
            return obs_all[:1].copy()

        def step(self, action):
            r = rew_all[self.t]
            self.ep_r += float(r)
            self.ep_l += 1
            done = self.t in ends
            info = {}
            if done:  # what Monitor adds at a true episode end
                info["episode"] = {"r": self.ep_r, "l": self.ep_l}
                self.ep_r, self.ep_l = 0.0, 0
            self.t += 1
            return obs_all[self.t: self.t + 1].copy(), np.array([r], dtype=np.float32), np.array([done]), [info]

    calls, cache_drops = [], []
    canned = torch.rand(n_steps, act_dim, generator=g) * 2 - 1

    class Model:
        device = torch.device("cpu")
        eval_context_len, use_inference_cache, persist_context, compile = 5, True, False, False
        target_return_type = "predefined"
        replay_buffer = SimpleNamespace(seqs_per_sample=1)
        policy = None

        def __init__(self):
            self.inference_params = SimpleNamespace(reset=lambda: cache_drops.append(("inference_params.reset", len(calls))))

        def __setattr__(self, k, v):
            if k == "past_key_values" and v is None:
                cache_drops.append(("past_key_values=None", len(calls)))
            object.__setattr__(self, k, v)

        def compute_target_return_val(self, env=None, task_id=0):
            return target / reward_scale

        def get_reward_scale_for_env(self, envid=None):
            return reward_scale

        def predict(self, policy, states, actions, rewards, returns_to_go, timesteps, state=None, episode_start=None,
                    deterministic=True, context_len=5, prompt=None, task_id=None, is_eval=False, env_act_dim=None):
            calls.append({"obs_last": states[-1].tolist(), "rtg_last": float(returns_to_go[0, -1]),
                          "timestep_last": int(timesteps[0, -1]), "n_states": int(states.shape[0]),
                          "context_len": int(context_len), "env_act_dim": int(env_act_dim),
                          "reward_last": float(rewards[-1]), "n_actions": int(actions.shape[0])})
            return canned[len(calls) - 1].clone(), None

    ns = {"gym": SimpleNamespace(Env=object, spaces=SimpleNamespace(Discrete=Discrete)), "np": np, "torch": torch,
          "time": _time, "warnings": _warnings, "VecEnv": VecEnv, "VecMonitor": object, "VecTransposeImage": None,
          "is_vecenv_wrapped": lambda env, cls: True, "get_action_dim": lambda sp: act_dim,
          "get_obs_shape": lambda sp: (obs_dim,), "is_image_space": lambda sp: False,
          "is_image_space_channels_first": lambda sp: True, "extract_env_name": lambda env, task_id=0: "Scripted-v0",
          "discount_cumsum_torch": None}
    from typing import Any, Callable, Dict, List, Optional, Tuple, Union
    ns.update(Any=Any, Callable=Callable, Dict=Dict, List=List, Optional=Optional, Tuple=Tuple, Union=Union)
    import sys as _sys
    mon = SimpleNamespace(Monitor=object)
    _sys.modules.setdefault("stable_baselines3", SimpleNamespace())
    _sys.modules.setdefault("stable_baselines3.common", SimpleNamespace())
    _sys.modules["stable_baselines3.common.monitor"] = mon   # the function's local `from ... import Monitor`
    try:
        exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
        rewards_out, lengths_out, _times = ns["custom_evaluate_policy"](Model(), Env(), n_eval_episodes=len(ep_lens),
                                                                        return_episode_rewards=True, warn=False)
    finally:
        for k in ("stable_baselines3.common.monitor", "stable_baselines3.common", "stable_baselines3"):
            if isinstance(_sys.modules.get(k), SimpleNamespace):
                del _sys.modules[k]
    return {"obs": obs_all.tolist(), "rewards": rew_all.tolist(), "episode_lengths_scripted": list(ep_lens),
            "reward_scale": reward_scale, "target_return": target, "act_dim": act_dim, "predict_calls": calls,
            "cache_drops": [[k, int(i)] for k, i in cache_drops],
            "episode_rewards": [float(x) for x in rewards_out], "episode_lengths": [int(x) for x in lengths_out]}


def _exec_classes(path, names, ns):
    """Execute whole class definitions of a reference file (every method, the real inheritance chain, zero-argument
    `super()` intact) in a namespace that supplies stand-ins for the bases / imports the file cannot get here."""
    import ast
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    assert len(keep) == len(names), (path, names)
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def xlstm_model_trace():
    """The reference's xLSTM inference wrapper, executed end to end around a stand-in block stack.

    Reference classes executed WHOLE (AST class definitions, their own inheritance chain):
      OnlineDecisionTransformerOutput, OnlineDecisionTransformerModel   (online_decision_transformer_model.py:15-760:
          forward :326-390, compute_hidden_states :392-460 incl. the `x[:, -seq_length*len(inputs):]` slice and the
          [B, tokens, seq, D] permute, compute_inputs / embed_inputs / prepare_inputs_and_masks :463-612)
      DiscreteDTModel            (discrete_decision_transformer_model.py: construct_inputs_and_masks :236-316,
          action_log_prob_logits :318-347, get_predictions :368-383 -- action read at tok_to_pred_pos["a"])
      MultiDomainDiscreteDTModel (multi_domain_discrete_dt_model.py:83-108 head post-processing)
      xLSTMEncoder, DecisionXLSTMModel, MultiDomainDiscreteDecisionXLSTMModel (decision_xlstm.py: xLSTMEncoder.forward
          :138-169 -- one `self.layers.step` per token, hidden states concatenated; handle_inference_cache :222-234)
    and, as plain methods on a stand-in agent, DecisionTransformerSb3.predict (decision_transformer_sb3.py:621-667),
    DecisionXLSTM.pad_inputs (algos/decision_xlstm.py:11-28), DiscreteDecisionTransformerSb3.get_action_pred
    (discrete_decision_transformer_sb3.py:13-72).  Stand-ins: the transformers / xlstm base classes are empty classes
    (no __init__ is run; the instance gets plain nn modules carrying the seeded test weights), and `encoder.layers` is an
    object whose `.step(x, state)` is the oracle's `xlstm_ref.stack_step` -- the xlstm package is absent, so the vector
    pins everything AROUND the block stack (what is embedded when, which tokens reach the stack, how the state is handed
    over and dropped, where the action is read), not the block arithmetic.
    Two envs, each rolled out on its own at batch 1 as the reference does (evaluation.py:80), context_len 5,
    reset_inf_cache_freq 3 (cache drops), one episode end for env 1 (evaluation.py:238-251 sets past_key_values None)."""
    from dataclasses import dataclass
    from types import SimpleNamespace
    from typing import Optional, Tuple, Union
    import torch.nn as nn
    from transformers.modeling_outputs import BaseModelOutputWithPastAndCrossAttentions
    from transformers.models.decision_transformer.modeling_decision_transformer import DecisionTransformerOutput
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    sys.path.insert(0, REF)
    from lram_amd import init_state_dict, preset
    from oracle import xlstm_ref
    from src.tokenizers_custom import make_tokenizer

    class _Base:   # stands in for transformers' DecisionTransformerModel / PreTrainedModel: no behaviour at all
        pass

    rms = importlib.util.spec_from_file_location("ref_rms_norm", os.path.join(REF, "src/algos/models/rms_norm.py"))
    rms_mod = importlib.util.module_from_spec(rms)
    rms.loader.exec_module(rms_mod)
    ns = {"torch": torch, "nn": nn, "dataclass": dataclass, "DecisionTransformerModel": _Base, "PreTrainedModel": _Base,
          "DecisionTransformerOutput": DecisionTransformerOutput, "Optional": Optional, "Tuple": Tuple, "Union": Union,
          "BaseModelOutputWithPastAndCrossAttentions": BaseModelOutputWithPastAndCrossAttentions,
          "LlamaRMSNorm": rms_mod.LlamaRMSNorm, "DecisionTransformerConfig": object,
          "xLSTMLayerNorm": type(None), "MultiHeadLayerNorm": type(None), "LinearHeadwiseExpand": type(None)}
    models = os.path.join(REF, "src/algos/models")
    _exec_classes(os.path.join(models, "online_decision_transformer_model.py"),
                  ["OnlineDecisionTransformerOutput", "OnlineDecisionTransformerModel"], ns)
    _exec_classes(os.path.join(models, "discrete_decision_transformer_model.py"), ["DiscreteDTModel"], ns)
    _exec_classes(os.path.join(models, "multi_domain_discrete_dt_model.py"), ["MultiDomainDiscreteDTModel"], ns)
    _exec_classes(os.path.join(models, "decision_xlstm.py"),
                  ["xLSTMEncoder", "DecisionXLSTMModel", "MultiDomainDiscreteDecisionXLSTMModel"], ns)
    Model, Encoder = ns["MultiDomainDiscreteDecisionXLSTMModel"], ns["xLSTMEncoder"]

    seed = 5
    spec = preset("xlstm_tiny")
    sd = init_state_dict(spec, seed=seed)
    D = spec.d_model

    def linear(w, b):
        m = nn.Linear(sd[w].shape[1], sd[w].shape[0])
        with torch.no_grad():
            m.weight.copy_(sd[w]), m.bias.copy_(sd[b])
        return m

    def build_model():
        me = object.__new__(Model)
        me.config = SimpleNamespace(use_return_dict=True, output_attentions=False, output_hidden_states=False,
                                    add_cross_attention=False, hidden_size=D, act_dim=spec.act_dim, chunkwise_step=False)
        me.hidden_size, me.is_discrete, me.training = D, False, False
        me.embed_state = linear("embed_state.weight", "embed_state.bias")
        me.embed_return = linear("embed_return.weight", "embed_return.bias")
        me.embed_rewards = linear("embed_rewards.weight", "embed_rewards.bias")
        me.embed_ln = nn.LayerNorm(D)
        with torch.no_grad():
            me.embed_ln.weight.copy_(sd["embed_ln.weight"]), me.embed_ln.bias.copy_(sd["embed_ln.bias"])
        me.action_net = Model.make_head(D, spec.n_vocab * spec.act_dim, 1)     # the reference's own head factory
        with torch.no_grad():
            me.action_net[0].weight.copy_(sd["action_net.0.weight"]), me.action_net[0].bias.copy_(sd["action_net.0.bias"])
        torch.manual_seed(3)   # modules whose outputs the rollout never reads (they are evaluated all the same)
        me.predict_state, me.predict_return, me.predict_reward = nn.Linear(D, spec.state_dim), nn.Linear(D, 1), nn.Linear(D, 1)
        me.embed_action_disc = nn.Embedding(spec.n_vocab + 1, D, padding_idx=spec.n_vocab)
        me.action_pad_token, me.a_pos_embds = None, False
        me.action_tokenizer = make_tokenizer("minmax", {"vocab_size": spec.action_channels, "shift": spec.n_discrete})
        me.rtg_condition, me.reward_condition, me.action_condition = True, True, False
        me.use_time_embds, me.symlog_transform, me.img_is_encoded, me.separate_ln = False, False, False, False
        me.tokenize_s, me.tokenize_rtg, me.tokenize_r, me.tokenize_a = False, False, False, True
        me.tok_a_target_only, me.tok_rtg_target_only, me.shared_a_head, me.stochastic_policy = False, False, True, False
        me.patch_size, me.discrete_actions, me.num_actions = None, spec.n_discrete, spec.n_vocab
        me.action_channels, me.num_task_heads, me.global_pos_embds, me.inf_dummy_batch_size = spec.action_channels, 1, False, None
        me.p_mask, me.p_token_drop = 0, 0
        enc = object.__new__(Encoder)
        enc.config = me.config
        calls = []

        class Layers:   # [3P] xLSTMBlockStack stand-in: `.step` is the oracle's restatement
            def step(self, x, state=None):
                calls.append((tuple(x.shape), state is None))
                return xlstm_ref.stack_step(spec, sd, x, state)
        enc.layers = Layers()
        me.encoder = lambda **kw: enc.forward(**kw)
        return me, calls

    fns = {}
    fns.update(_exec_methods(os.path.join(REF, "src/algos/decision_transformer_sb3.py"), "DecisionTransformerSb3", ["predict"]))
    fns.update(_exec_methods(os.path.join(REF, "src/algos/decision_xlstm.py"), "DecisionXLSTM", ["pad_inputs"]))
    fns.update(_exec_methods(os.path.join(REF, "src/algos/discrete_decision_transformer_sb3.py"),
                             "DiscreteDecisionTransformerSb3", ["get_action_pred"]))
    Agent = type("Agent", (), {k: fns[k] for k in ("predict", "pad_inputs", "get_action_pred")})

    steps, freq, ctx = 9, 3, 5
    env_act_dims, obs_dims = [4, 3], [20, 13]
    episode_end_after = [set(), {4}]
    g = torch.Generator().manual_seed(2024)
    out_envs = []
    for e in range(2):
        model, calls = build_model()
        ag = Agent()
        ag.transforms, ag.s_proj_dim, ag.a_proj_dim, ag.s_proj_raw = None, None, None, False
        ag.state_mean = ag.state_std = None
        ag.reset_inf_cache_freq, ag.past_key_values, ag.use_inference_cache = freq, None, True
        ag.ddp_kwargs, ag.target_return_type, ag.a_sample_kwargs = {}, "predefined", None
        ag.use_amp, ag.amp_dtype, ag.device = False, torch.bfloat16, torch.device("cpu")
        ag.replay_buffer = SimpleNamespace(max_state_dim=spec.state_dim, max_act_dim=spec.act_dim)
        ag.policy = model
        ad, od = env_act_dims[e], obs_dims[e]
        obs_all = torch.rand(steps + 1, od, generator=g) * 2 - 1
        env_rewards = torch.rand(steps, generator=g)
        reward_scale, rtg0 = 10.0, 3.5
        # the rollout bookkeeping of custom_evaluate_policy (evaluation.py:104-177, :238-251 at an episode end)
        states, actions, rewards = obs_all[:1].clone(), torch.zeros((0, ad)), torch.zeros(0)
        target_return, timesteps, t_ep = torch.tensor(rtg0).reshape(1, 1), torch.tensor(0).reshape(1, 1), 0
        rec = {"returned": [], "hidden": [], "logits": [], "rtg_in": [], "cache_is_none": [], "stack_calls": []}
        with torch.no_grad():
            for t in range(steps):
                actions = torch.cat([actions, torch.zeros((1, ad))], dim=0)
                rewards = torch.cat([rewards, torch.zeros(1)])
                rec["cache_is_none"].append(ag.past_key_values is None)
                rec["rtg_in"].append(float(target_return[0, -1]))
                n0 = len(calls)
                seen = {}

                def policy(**inputs):
                    o = model.forward(**inputs)
                    seen["hidden"], seen["logits"] = o.last_encoder_output, o.action_logits
                    return o
                a, _ = ag.predict(policy, states, actions, rewards, target_return, timesteps, state=None, episode_start=None,
                                  deterministic=True, context_len=ctx, prompt=None, task_id=None, is_eval=True, env_act_dim=ad)
                rec["returned"].append(a.tolist())
                rec["hidden"].append(seen["hidden"][0, :, 0].tolist())      # [tokens, D]: x[:, tok, t] of the reference
                rec["logits"].append(seen["logits"][0, -1].tolist())        # [act_dim, n_vocab]
                rec["stack_calls"].append([[list(sh), fresh] for sh, fresh in calls[n0:]])
                actions[-1] = a
                rewards[-1] = env_rewards[t] / reward_scale
                t_ep += 1
                if t in episode_end_after[e]:
                    states, actions, rewards = obs_all[t + 1: t + 2].clone(), torch.zeros((0, ad)), torch.zeros(0)
                    target_return, timesteps, t_ep = torch.tensor(rtg0).reshape(1, 1), torch.tensor(0).reshape(1, 1), 0
                    ag.past_key_values = None
                    continue
                states = torch.cat([states, obs_all[t + 1: t + 2]], dim=0)
                target_return = torch.cat([target_return, (target_return[0, -1] - env_rewards[t] / reward_scale).reshape(1, 1)], dim=1)
                timesteps = torch.cat([timesteps, torch.ones((1, 1), dtype=torch.long) * t_ep], dim=1)
        final = ag.past_key_values
        rec["final_state_is_none"] = final is None
        if final is not None:
            rec["final_mlstm_n_block0"] = final["block_0"]["mlstm_state"][1].reshape(-1).tolist()
            rec["final_slstm_block1"] = final["block_1"]["slstm_state"].reshape(-1).tolist()
        out_envs.append({"obs": obs_all.tolist(), "env_rewards": env_rewards.tolist(), "env_act_dim": ad, "obs_dim": od,
                         "episode_end_after_step": sorted(episode_end_after[e]), **rec})
    return {"preset": "xlstm_tiny", "weight_seed": seed, "reset_inf_cache_freq": freq, "context_len": ctx,
            "reward_scale": 10.0, "target_return0": 3.5, "tok_to_pred_pos_a": int(model.tok_to_pred_pos["a"]),
            "tok_to_pos": {k: (v if isinstance(v, int) else list(v)) for k, v in model.tok_to_pos.items()}, "envs": out_envs}


def minmax_tokenizer_vectors():
    """MinMaxTokenizer (src/tokenizers_custom/minmax_tokenizer.py:14-47), executed for channel counts whose bin width is no
    power of two as well (64, 100, 255, 256, 495 channels; shifts 0 / 7 / 18; range [-1, 1]): `inv_tokenize` of EVERY token
    0 .. channels + shift - 1, and `tokenize` of every bin edge k * bin_width - 1 with one fp32 ulp to either side, the ends of
    the range, values beyond them and 200 random values.  Data only, to tests/golden/minmax_tokenizer_reference.npz; the CPU
    oracle is held to it bit for bit (tests/test_oracle_golden.py), and the engine's head kernels to the oracle."""
    import numpy as np
    from src.tokenizers_custom import make_tokenizer
    arrays = {"channels": [], "shift": []}
    g = torch.Generator().manual_seed(495)
    i = 0
    for channels in (64, 100, 255, 256, 495):
        for shift in (0, 7, 18):
            tok = make_tokenizer("minmax", {"vocab_size": channels, "shift": shift})
            edges = torch.arange(channels + 1, dtype=torch.float32) * (2.0 / channels) - 1.0
            up = torch.nextafter(edges, torch.full_like(edges, 2.0))
            down = torch.nextafter(edges, torch.full_like(edges, -2.0))
            extra = torch.tensor([-1.0, 1.0, 1.5, 3e9, -1.5, -3e9, 0.0, -0.0, 0.999999, -0.999999])
            x = torch.cat([edges, up, down, extra, torch.rand(200, generator=g) * 2 - 1]).reshape(1, -1)
            all_tokens = torch.arange(0, channels + shift).reshape(1, -1)
            arrays["channels"].append(channels), arrays["shift"].append(shift)
            arrays[f"x_{i}"] = x.reshape(-1).numpy().copy()
            arrays[f"tokens_{i}"] = tok.tokenize(x.clone()).reshape(-1).numpy().astype(np.int64)
            arrays[f"inv_{i}"] = tok.inv_tokenize(all_tokens.clone()).reshape(-1).numpy().astype(np.float32)
            i += 1
    arrays["channels"], arrays["shift"] = np.asarray(arrays["channels"]), np.asarray(arrays["shift"])
    np.savez_compressed(os.path.join(HERE, "minmax_tokenizer_reference.npz"), **arrays)
    print("wrote", os.path.join(HERE, "minmax_tokenizer_reference.npz"))


def main():
    sys.path.insert(0, REF)
    from src.tokenizers_custom import make_tokenizer  # reference code, executed not copied
    minmax_tokenizer_vectors()
    if "--tokenizer-only" in sys.argv:   # only minmax_tokenizer_reference.npz: needs torch and the tokenizer package alone
        return
    out = {"generator": "tests/golden/make_golden_from_reference.py", "reference": "ml-jku/LRAM @ 2024-11-01"}

    tok = make_tokenizer("minmax", {"vocab_size": 256, "shift": 18})
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.tensor([-1.0, -0.999, -0.5, 0.0, 0.5, 0.9921875, 0.9999, 1.0, -1.5, 1.5, 1e-9, -1e-9]),
                   torch.rand(116, generator=g) * 2 - 1]).reshape(16, 8)
    tokens = tok.tokenize(x.clone())
    all_tokens = torch.arange(0, 274).reshape(1, -1)
    inv = tok.inv_tokenize(all_tokens.clone())
    out["minmax_shift18"] = {"x": x.tolist(), "tokens": tokens.tolist(), "inv_table": inv.reshape(-1).tolist()}

    tok0 = make_tokenizer("minmax", {"vocab_size": 256})
    out["minmax_shift0"] = {"x": x.tolist(), "tokens": tok0.tokenize(x.clone()).tolist(),
                            "inv_table": tok0.inv_tokenize(torch.arange(0, 256).reshape(1, -1)).reshape(-1).tolist()}

    spec = importlib.util.spec_from_file_location("ref_rms_norm", os.path.join(REF, "src/algos/models/rms_norm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cases = []
    for eps in (1e-6, 1e-5):
        norm = mod.LlamaRMSNorm(48, eps=eps)
        with torch.no_grad():
            norm.weight.copy_(torch.randn(48, generator=g) * 0.3 + 1.0)
        xin = torch.randn(5, 3, 48, generator=g) * 2.0
        with torch.no_grad():
            y = norm(xin)
        cases.append({"eps": eps, "weight": norm.weight.tolist(), "x": xin.tolist(), "y": y.tolist()})
    out["llama_rms_norm"] = cases

    out["obs_full_space"] = obs_full_space_vectors(g)
    out["action_from_logits"] = action_from_logits_vectors(g, tok)
    out["token_front_end"] = token_front_end_vectors(g)
    impala_cnn_vectors(g)
    out["agent_predict_trace"] = agent_predict_trace(g)
    out["mamba_agent_trace"] = mamba_agent_trace()
    out["xlstm_model_trace"] = xlstm_model_trace()
    out["load_model_weights_trace"] = load_model_weights_trace()
    out["checkpoint_key_names"] = checkpoint_key_names()
    out["reference_presets"] = reference_presets()
    out["evaluate_policy_trace"] = evaluate_policy_trace(g)

    with open(os.path.join(HERE, "reference_vectors.json"), "w") as fh:
        json.dump(out, fh)
    print("wrote", os.path.join(HERE, "reference_vectors.json"))


if __name__ == "__main__":
    main()
