"""ctypes binding of liblram_hip.so (C ABI: include/lram_hip.h) and the `Engine` host object.

PyTorch is used for device memory, streams and (elsewhere) torch.distributed only: every tensor handed
to the library is passed as a raw device pointer.  There is no CPU / eager fallback: if the HIP library
is missing or fails to load, construction raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional

import torch

from .config import ModelSpec
from .weights import engine_layout

LRAM_ABI_VERSION = 1
LRAM_MAX_BLOCKS = 64
LRAM_HEAD_PER_SLOT = 2    # value of `discrete`: head mode per slot, from the slot table
LRAM_SLOT_DISCRETE = 1    # slot table flag bits
LRAM_SLOT_IMAGE = 2
_LIB_NAME = "liblram_hip.so"


class LramConfig(ctypes.Structure):
    """Field-for-field mirror of `lram_config` in include/lram_hip.h."""
    _fields_ = [
        ("abi_version", ctypes.c_int32), ("backbone", ctypes.c_int32), ("d_model", ctypes.c_int32),
        ("n_blocks", ctypes.c_int32), ("tokens_per_step", ctypes.c_int32), ("pred_token", ctypes.c_int32),
        ("n_heads", ctypes.c_int32), ("conv_k", ctypes.c_int32), ("qkv_blocksize", ctypes.c_int32),
        ("inner", ctypes.c_int32), ("ffn_dim", ctypes.c_int32), ("block_is_slstm", ctypes.c_int32 * LRAM_MAX_BLOCKS),
        ("norm_is_rms", ctypes.c_int32), ("ln_eps", ctypes.c_float),
        ("d_inner", ctypes.c_int32), ("d_state", ctypes.c_int32), ("d_conv", ctypes.c_int32),
        ("dt_rank", ctypes.c_int32), ("norm_eps", ctypes.c_float),
        ("state_dim", ctypes.c_int32), ("act_dim", ctypes.c_int32), ("n_vocab", ctypes.c_int32),
        ("n_discrete", ctypes.c_int32), ("action_channels", ctypes.c_int32),
        ("tok_min", ctypes.c_float), ("tok_max", ctypes.c_float),
    ]


# name -> (restype, argtypes); every symbol include/lram_hip.h declares
_VP = ctypes.c_void_p
_SYMBOLS = {
    "lram_last_error": (ctypes.c_char_p, []),
    "lram_abi_version": (ctypes.c_int32, []),
    "lram_build_id": (ctypes.c_char_p, []),
    "lram_create": (ctypes.c_int32, [ctypes.POINTER(LramConfig), ctypes.c_int32, ctypes.POINTER(_VP)]),
    "lram_destroy": (ctypes.c_int32, [_VP]),
    "lram_set_weight": (ctypes.c_int32, [_VP, ctypes.c_char_p, _VP, ctypes.c_size_t]),
    "lram_finalize": (ctypes.c_int32, [_VP]),
    "lram_state_alloc": (ctypes.c_int32, [_VP, ctypes.c_int32]),
    "lram_state_bytes_per_env": (ctypes.c_int64, [_VP]),
    "lram_reset": (ctypes.c_int32, [_VP, _VP, _VP]),
    "lram_step": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP, _VP, ctypes.c_int32, _VP, _VP, _VP]),
    "lram_prefill": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP, ctypes.c_int32, _VP, _VP,
                                      _VP]),
    "lram_score": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP, ctypes.c_int32, _VP, _VP, _VP,
                                    ctypes.c_int32, ctypes.c_double, _VP, _VP, _VP, _VP, _VP]),
    "lram_prefill_ragged": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP,
                                             _VP, _VP]),
    "lram_score_ragged": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP, _VP,
                                           _VP, ctypes.c_int32, ctypes.c_double, _VP, _VP, _VP, _VP, _VP]),
    "lram_prefill_append": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP,
                                             _VP, _VP]),
    "lram_score_append": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP, _VP, ctypes.c_int32, _VP, _VP,
                                           _VP, ctypes.c_int32, ctypes.c_double, _VP, _VP, _VP, _VP, _VP]),
    "lram_context_plan": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, _VP, ctypes.c_int32, _VP, ctypes.c_int32,
                                           ctypes.POINTER(ctypes.c_int32)]),
    "lram_score_last": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, ctypes.c_double, _VP, _VP]),
    "lram_score_tokens": (ctypes.c_int32, [_VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.c_float, ctypes.c_float, ctypes.c_int32, _VP, _VP, _VP, ctypes.c_int32,
                                           ctypes.c_double, _VP, _VP, _VP, _VP]),
    "lram_encoder_step": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP, _VP]),
    "lram_get_taps": (ctypes.c_int32, [_VP, _VP, _VP, _VP, _VP]),
    "lram_state_numel": (ctypes.c_int64, [_VP, ctypes.c_int32, ctypes.c_int32]),
    "lram_state_export": (ctypes.c_int32, [_VP, ctypes.c_int32, ctypes.c_int32, _VP, _VP]),
    "lram_state_import": (ctypes.c_int32, [_VP, ctypes.c_int32, ctypes.c_int32, _VP, _VP]),
    "lram_set_graph_mode": (ctypes.c_int32, [_VP, ctypes.c_int32]),
    "lram_set_micro_batches": (ctypes.c_int32, [_VP, ctypes.c_int32]),
    "lram_set_compat_mode": (ctypes.c_int32, [_VP, ctypes.c_int32, ctypes.c_int32]),
    "lram_get_compat_mode": (ctypes.c_int32, [_VP, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "lram_set_sampling": (ctypes.c_int32, [_VP, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, ctypes.c_double,
                                           ctypes.c_uint64, ctypes.c_uint64]),
    "lram_get_sampling": (ctypes.c_int32, [_VP, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint64)]),
    "lram_sample_tokens": (ctypes.c_int32, [_VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_double,
                                            ctypes.c_int32, ctypes.c_double, _VP, _VP, _VP]),
    "lram_sample_uniforms": (ctypes.c_int32, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32,
                                              ctypes.c_uint64, _VP, _VP]),
    "lram_set_sampling_slots": (ctypes.c_int32, [_VP, _VP, _VP, _VP, _VP]),
    "lram_get_sampling_slots": (ctypes.c_int32, [_VP, _VP, _VP, _VP, _VP, ctypes.POINTER(ctypes.c_int32)]),
    "lram_score_last_sampled": (ctypes.c_int32, [_VP, _VP, _VP, _VP]),
    "lram_sample_rows": (ctypes.c_int32, [_VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, _VP, _VP, _VP, _VP, _VP, _VP,
                                          _VP, _VP, _VP]),
    "lram_profile_begin": (ctypes.c_int32, [_VP]),
    "lram_profile_begin_sampled": (ctypes.c_int32, [_VP, ctypes.c_int32]),
    "lram_profile_end": (ctypes.c_int32, [_VP, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "lram_profile_end_split": (ctypes.c_int32, [_VP, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64),
                                                ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "lram_gemm_f32": (ctypes.c_int32, [_VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP]),
    "lram_gemm_skinny": (ctypes.c_int32, [_VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP,
                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP]),
    "lram_gemm_narrow": (ctypes.c_int32, [_VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP,
                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP]),
    "lram_gemm_narrow_f16x2": (ctypes.c_int32, [_VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP,
                                                ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP]),
    "lram_gemm_bf16x3": (ctypes.c_int32, [_VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP,
                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP]),
    "lram_gemm_f16x2": (ctypes.c_int32, [_VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP,
                                         ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP]),
    "lram_gemm_f16x2_presplit": (ctypes.c_int32, [_VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP,
                                                  ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP]),
    "lram_gemm_f16x2_presplit_8p": (ctypes.c_int32, [_VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP,
                                                     ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP]),
    "lram_embed_images": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP, _VP]),
    "lram_step_images": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP, _VP, _VP, ctypes.c_int32,
                         _VP, _VP, _VP]),
    "lram_embed_frames": (ctypes.c_int32, [_VP, _VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP, _VP]),
    "lram_prefill_frames": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP, _VP, _VP, ctypes.c_int32,
                                             _VP, ctypes.c_int32, _VP, ctypes.c_int32, _VP, _VP, _VP]),
    "lram_score_frames": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP, _VP, _VP, ctypes.c_int32,
                                           _VP, ctypes.c_int32, _VP, ctypes.c_int32, _VP, _VP, _VP, ctypes.c_int32, ctypes.c_double,
                                           _VP, _VP, _VP, _VP, _VP]),
    "lram_image_counts": (ctypes.c_int32, [_VP, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]),
    "lram_set_state_mode": (ctypes.c_int32, [_VP, ctypes.c_int32, ctypes.c_int32]),
    "lram_get_state_mode": (ctypes.c_int32, [_VP]),
    "lram_lazy_peek": (ctypes.c_int32, [_VP, ctypes.c_int32, ctypes.c_int32, _VP, _VP]),
    "lram_slot_state_numel": (ctypes.c_int64, [_VP]),
    "lram_state_copy_slots": (ctypes.c_int32, [_VP, _VP, _VP, ctypes.c_int32, _VP]),
    "lram_state_save_slots": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP]),
    "lram_state_load_slots": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP]),
    "lram_state_swap_slots": (ctypes.c_int32, [_VP, _VP, _VP, ctypes.c_int32, _VP]),
    "lram_set_live": (ctypes.c_int32, [_VP, ctypes.c_int32, _VP]),
    "lram_get_live": (ctypes.c_int32, [_VP]),
    "lram_set_context_rows": (ctypes.c_int32, [_VP, ctypes.c_int32]),
    "lram_get_context_rows": (ctypes.c_int32, [_VP]),
    "lram_context_counts": (ctypes.c_int32, [_VP, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]),
    "lram_window_alloc": (ctypes.c_int32, [_VP, ctypes.c_int32]),
    "lram_window_set_pad": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP]),
    "lram_step_window": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP, _VP, _VP, _VP, ctypes.c_int32, ctypes.c_int32, _VP,
                                          _VP, _VP]),
    "lram_window_peek": (ctypes.c_int32, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "lram_window_set_slots": (ctypes.c_int32, [_VP, ctypes.c_int32]),
    "lram_window_get_slots": (ctypes.c_int32, [_VP]),
    "lram_window_copy_slots": (ctypes.c_int32, [_VP, _VP, _VP, ctypes.c_int32, _VP]),
    "lram_window_swap_slots": (ctypes.c_int32, [_VP, _VP, _VP, ctypes.c_int32, _VP]),
    "lram_window_slot_numel": (ctypes.c_int64, [_VP]),
    "lram_window_save_slots": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP]),
    "lram_window_load_slots": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, _VP, _VP]),
    "lram_stream_rmw": (ctypes.c_int32, [_VP, ctypes.c_size_t, _VP]),
    "lram_stream_read": (ctypes.c_int32, [_VP, ctypes.c_size_t, _VP, _VP]),
    "lram_gemm_counts": (ctypes.c_int32, [_VP, ctypes.POINTER(ctypes.c_double), ctypes.c_int32]),
    "lram_slstm_counts": (ctypes.c_int32, [_VP, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]),
    "lram_set_slot_table": (ctypes.c_int32, [_VP, _VP, _VP]),
    "lram_get_slot_table": (ctypes.c_int32, [_VP, _VP, _VP, ctypes.POINTER(ctypes.c_int32)]),
    "lram_set_action_mask": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32]),
    "lram_get_action_mask": (ctypes.c_int32, [_VP, _VP, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    "lram_sample_rows_masked": (ctypes.c_int32, [_VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, _VP, _VP, _VP, _VP, _VP,
                                                 _VP, _VP, _VP, _VP, ctypes.c_int32, _VP]),
    "lram_score_tokens_masked": (ctypes.c_int32, [_VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                  ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_int32, _VP, _VP, _VP,
                                                  ctypes.c_int32, ctypes.c_double, _VP, _VP, _VP, _VP, ctypes.c_int32, _VP]),
    "lram_step_slots": (ctypes.c_int32, [_VP, _VP, _VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP, _VP, _VP, _VP, _VP,
                                         _VP]),
    "lram_pad_obs_slots": (ctypes.c_int32, [_VP, ctypes.c_int32, _VP, _VP, _VP, _VP, ctypes.c_int32, _VP, ctypes.c_int32,
                                            ctypes.c_int32, _VP]),
    "lram_pad_obs": (ctypes.c_int32, [_VP, ctypes.c_int32, _VP, _VP, _VP, _VP, ctypes.c_int32, ctypes.c_int32, _VP]),
    "lram_selftest_concurrent": (ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]),
    "lram_stream_copy": (ctypes.c_int32, [_VP, _VP, ctypes.c_size_t, _VP]),
}

_lib = None


def library_path() -> str:
    """The in-tree library; LRAM_LIB_VARIANT=<name> picks csrc/_variants/<name>.so instead -- A/B measurements of two
    builds inside one GPU call (scripts/gpu_ab.sh), never set in tests or by the driver."""
    here = os.path.dirname(os.path.abspath(__file__))
    variant = os.getenv("LRAM_LIB_VARIANT")
    if variant:
        return os.path.join(here, "csrc", "_variants", variant + ".so")
    return os.path.join(here, "csrc", _LIB_NAME)


def load_library():
    """dlopen the in-tree HIP library and bind every declared symbol.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"(hipcc --offload-arch=gfx950). There is no CPU fallback for the engine.")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.lram_abi_version() != LRAM_ABI_VERSION:
        raise RuntimeError("liblram_hip.so ABI version mismatch; rebuild the library")
    _lib = lib
    return lib


class LramError(RuntimeError):
    pass


def _check(lib, rc):
    if rc != 0:
        raise LramError(lib.lram_last_error().decode("utf-8", "replace"))


def make_config(spec: ModelSpec) -> LramConfig:
    c = LramConfig()
    c.abi_version = LRAM_ABI_VERSION
    c.backbone = 1 if spec.backbone == "mamba" else 0
    c.d_model, c.n_blocks = spec.d_model, spec.n_blocks
    c.tokens_per_step, c.pred_token = spec.tokens_per_step, spec.pred_token
    c.n_heads, c.conv_k, c.qkv_blocksize = spec.n_heads, spec.conv_k, spec.qkv_blocksize
    c.inner, c.ffn_dim = spec.inner, spec.ffn_dim
    if spec.n_blocks > LRAM_MAX_BLOCKS:
        raise ValueError(f"n_blocks {spec.n_blocks} > {LRAM_MAX_BLOCKS}")
    for i in spec.slstm_at:
        c.block_is_slstm[i] = 1
    c.norm_is_rms = int(spec.rms_norm)
    c.ln_eps = spec.ln_eps
    c.d_inner, c.d_state, c.d_conv = spec.d_inner, spec.d_state, spec.d_conv
    c.dt_rank = int(spec.dt_rank) if spec.backbone == "mamba" else 0
    c.norm_eps = spec.norm_eps
    c.state_dim, c.act_dim, c.n_vocab = spec.state_dim, spec.act_dim, spec.n_vocab
    c.n_discrete, c.action_channels = spec.n_discrete, spec.action_channels
    c.tok_min, c.tok_max = -1.0, 1.0
    return c


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream_ptr(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _head_mode(discrete) -> int:
    """The `discrete` argument of the C ABI: False / True, or "per_slot" (LRAM_HEAD_PER_SLOT: from the slot table)."""
    if isinstance(discrete, str):
        if discrete != "per_slot":
            raise ValueError(f'discrete must be False, True or "per_slot", got {discrete!r}')
        return LRAM_HEAD_PER_SLOT
    return int(bool(discrete))


def _over_mode(over) -> int:
    """The `over` argument of the scoring entries: "vocab" (all n_vocab logits, the reference's cross-entropy) or
    "selectable" (the range the head in use picks from)."""
    if over not in ("vocab", "selectable"):
        raise ValueError(f'over must be "vocab" or "selectable", got {over!r}')
    return int(over == "selectable")


class ScoreResult:
    """What Engine.score returns: `actions` float32, `tokens` int32, `logp` float32 [B, L, act_dim] and `logits` float32
    [B, L, act_dim, n_vocab]; a field that was not asked for is None.  Masked timesteps and unused columns hold action 0,
    token -1, logp 0 (and zero logits)."""
    __slots__ = ("actions", "tokens", "logp", "logits")

    def __init__(self, actions=None, tokens=None, logp=None, logits=None):
        self.actions, self.tokens, self.logp, self.logits = actions, tokens, logp, logits

    def __repr__(self):
        f = ", ".join(f"{k}={None if getattr(self, k) is None else tuple(getattr(self, k).shape)}" for k in self.__slots__)
        return f"ScoreResult({f})"


def _chk_dev(t: torch.Tensor, dtype, shape, device, name):
    if t.device != device or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got "
                         f"{t.dtype} {tuple(t.shape)} on {t.device} (contiguous={t.is_contiguous()})")


def _int_list(x, name: str, what: str):
    """A list, a numpy array or an integer tensor (moved to the host) as plain ints; `what` names its entries in the message."""
    if isinstance(x, torch.Tensor):
        if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
            raise ValueError(f"{name}: expected integer {what}, got {x.dtype}")
        x = x.reshape(-1).tolist()
    out = []
    for v in x:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name}: expected integer {what}, got {v!r}")
        out.append(int(v))
    return out


def _slot_list(x, name: str):
    """A list of env slot indices as plain ints."""
    return _int_list(x, name, "slot indices")


def check_slot_lists(src, dst, batch: int):
    """The rules of lram_state_copy_slots, checked on the host (no GPU needed): every index in 0 .. batch - 1, `dst` entries
    unique, no slot both source and destination; `src` may repeat (fan-out).  dst=None checks one list the way
    lram_state_load_slots does (in range, unique).  Returns the lists as ints; raises ValueError.  Empty lists are a no-op."""
    src = _slot_list(src, "src")
    for v in src:
        if not 0 <= v < batch:
            raise ValueError(f"src: slot index {v} out of range (batch {batch})")
    if dst is None:
        if len(set(src)) != len(src):
            raise ValueError("slots: a slot is listed twice")
        return src, None
    dst = _slot_list(dst, "dst")
    if len(src) != len(dst):
        raise ValueError(f"src and dst must have the same length, got {len(src)} and {len(dst)}")
    for v in dst:
        if not 0 <= v < batch:
            raise ValueError(f"dst: slot index {v} out of range (batch {batch})")
    if len(set(dst)) != len(dst):
        raise ValueError("dst: a destination slot is listed twice")
    both = set(src) & set(dst)
    if both:
        raise ValueError(f"slots {sorted(both)} are both source and destination (permute by save_slots then load_slots)")
    return src, dst


def check_swap_lists(a, b, batch: int):
    """The rules of lram_state_swap_slots, checked on the host (no GPU needed): check_slot_lists' rules, plus all 2n indices
    distinct (a slot is exchanged at most once per call).  Returns the lists as ints; raises ValueError."""
    a, b = check_slot_lists(a, b, batch)
    if len(set(a)) != len(a):
        raise ValueError("a: a slot is listed twice (all indices of a swap must be distinct)")
    return a, b


def _as_bools(a: torch.Tensor) -> torch.Tensor:
    """A CPU tensor of bools, or of 0 / 1 integers, as bools."""
    if a.dtype == torch.bool:
        return a
    if a.dtype.is_floating_point or a.dtype.is_complex or bool(((a != 0) & (a != 1)).any()):
        raise ValueError(f"action mask: expected bools (or 0 / 1 integers), got {a.dtype}")
    return a != 0


def pack_action_mask(allowed) -> torch.Tensor:
    """bool [rows, n] (tensor or array) -> int32 [rows, ceil(n / 32)] on the CPU holding the uint32 words of
    lram_set_action_mask: bit t & 31 of word t >> 5 = token t is allowed."""
    a = torch.as_tensor(allowed).to("cpu")
    if a.dim() != 2 or a.shape[1] < 1:
        raise ValueError(f"action mask: expected a 2-d bool array [rows, n], got shape {tuple(a.shape)}")
    a = _as_bools(a)
    rows, n = a.shape
    words = (n + 31) // 32
    padded = torch.zeros(rows, words * 32, dtype=torch.int64)
    padded[:, :n] = a
    w = (padded.view(rows, words, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)   # 0 .. 2^32 - 1
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def unpack_action_mask(words: torch.Tensor, n: int) -> torch.Tensor:
    """The inverse: int32 / uint32 words [rows, ceil(n / 32)] -> bool [rows, n]."""
    w = torch.as_tensor(words).to("cpu").to(torch.int64) & 0xFFFFFFFF
    if w.dim() != 2 or w.shape[1] != (int(n) + 31) // 32:
        raise ValueError(f"action mask words: expected [rows, {(int(n) + 31) // 32}], got shape {tuple(w.shape)}")
    bits = (w.unsqueeze(-1) >> torch.arange(32, dtype=torch.int64)) & 1
    return bits.reshape(w.shape[0], -1)[:, :int(n)].bool().contiguous()


def check_action_mask(mask, batch: int, n_vocab: int, n_discrete: int, slot_discrete=None) -> torch.Tensor:
    """The refusal rules of lram_set_action_mask on the host: `mask` bool [batch, n_vocab]; every slot must allow something
    inside its selectable range -- [0, n_discrete) where slot_discrete[b] (the slot table's head mode), [0, n_vocab) otherwise
    and without a table.  Returns the mask as a CPU bool tensor; raises ValueError."""
    m = torch.as_tensor(mask).to("cpu")
    if m.dim() != 2 or tuple(m.shape) != (int(batch), int(n_vocab)):
        raise ValueError(f"action mask: expected bool [{batch}, {n_vocab}] (one row per env slot), got shape {tuple(m.shape)}")
    m = _as_bools(m)
    disc = torch.zeros(int(batch), dtype=torch.bool)
    if slot_discrete is not None:
        disc = torch.as_tensor(slot_discrete).to("cpu").reshape(-1).bool()
        if disc.numel() != int(batch):
            raise ValueError(f"slot_discrete: expected {batch} entries (one per env slot), got {disc.numel()}")
        if bool(disc.any()) and int(n_discrete) < 1:
            raise ValueError("slot_discrete: a discrete slot needs n_discrete >= 1")
    count = torch.where(disc, m[:, :int(n_discrete)].sum(1), m.sum(1))
    empty = torch.nonzero(count == 0).reshape(-1)
    if empty.numel():
        raise ValueError(f"action mask: slot {int(empty[0])} allows nothing inside its selectable range")
    return m.contiguous()


def _i32_array(values):
    return (ctypes.c_int32 * max(1, len(values)))(*values)


CONTEXT_ROWS = ("all", "live", "started")   # LRAM_CONTEXT_ROWS_ALL / _LIVE / _STARTED, by value


def _context_batch(eng) -> int:
    """The rows a stored-context or encoder call of `eng` takes: the batch, or the live count (Engine.set_context_rows)."""
    return eng.batch if getattr(eng, "_context_rows", "all") == "all" else eng._live


def _context_rows_of(eng, buf):
    n = _context_batch(eng)
    return buf if n == eng.batch else buf[:n]


def check_context_lengths(lengths, batch: int, L: int):
    """The length rules of lram_prefill_ragged / lram_score_ragged, checked on the host (no GPU needed): `batch` integer
    entries (a list, a numpy array or an integer tensor, moved to the host), each in 0 .. L, not all 0.  Returns them as ints;
    raises ValueError."""
    out = _int_list(lengths, "lengths", "lengths")
    if len(out) != batch:
        raise ValueError(f"lengths: expected {batch} entries (one per env slot), got {len(out)}")
    for b, v in enumerate(out):
        if not 0 <= v <= L:
            raise ValueError(f"lengths: length {v} of env slot {b} is outside 0 .. {L}")
    if not any(out):
        raise ValueError("lengths: every length is 0 (no env slot has a context)")
    return out


WINDOW_PAD = ("reference", "none")   # LRAM_WINDOW_PAD_REFERENCE / _NONE, by value
WINDOW_SLOTS = ("shared", "own")     # LRAM_WINDOW_SLOTS_SHARED / _OWN, by value


def check_window_timesteps(K, batch: int, d_model: int) -> int:
    """The rules of lram_window_alloc, checked on the host (no GPU needed): K an integer >= 0 (0 frees the ring), d_model a
    multiple of 4 and [batch, K, d_model] floats within 2 GiB.  Returns K; raises ValueError."""
    if isinstance(K, bool) or int(K) != K or K < 0:
        raise ValueError(f"window: timesteps must be an integer >= 1 (0 frees the ring), got {K!r}")
    K = int(K)
    if K > 0 and d_model % 4 != 0:
        raise ValueError(f"window: d_model {d_model} is no multiple of 4 (the ring's kernels move float4)")
    if batch * K * d_model > (1 << 29):
        raise ValueError(f"window: the [{batch}, {K}, {d_model}] windows exceed 2 GiB")
    return K


def check_window_controls(reset, relabel, keep, batch: int):
    """The per-step control arrays of lram_step_window, checked on the host (no GPU needed).  Each is None or has `batch`
    entries (a list, a numpy array or a tensor, moved to the host): `reset` bools or 0 / 1, `relabel` and `keep` integers
    >= 0 (0: leave alone).  A relabel on a reset slot is refused: the reset drops the entries the relabel would rewrite.
    Returns (reset, relabel, keep) as lists of ints or None; raises ValueError."""
    def ints(x, name, what):
        if x is None:
            return None
        if isinstance(x, torch.Tensor):
            x = x.reshape(-1).tolist()
        out = _int_list([int(v) if isinstance(v, bool) and name == "reset" else v for v in x], name, what)
        if len(out) != batch:
            raise ValueError(f"{name}: expected {batch} entries (one per env slot), got {len(out)}")
        return out
    reset = ints(reset, "reset", "flags")
    relabel, keep = ints(relabel, "relabel", "counts"), ints(keep, "keep", "counts")
    for b, v in enumerate(reset or ()):
        if v not in (0, 1):
            raise ValueError(f"reset: flag {v} of env slot {b} is neither 0 nor 1")
    for name, arr in (("relabel", relabel), ("keep", keep)):
        for b, v in enumerate(arr or ()):
            if v < 0:
                raise ValueError(f"{name}: {name} {v} of env slot {b} is negative")
    if reset is not None and relabel is not None:
        for b in range(batch):
            if reset[b] and relabel[b] > 0:
                raise ValueError(f"relabel: env slot {b} is reset and relabelled (relabel {relabel[b]})")
    return reset, relabel, keep


class WindowResult:
    """What Engine.window() returns: the windows end-aligned and oldest to newest, rows ahead of an env's count zeroed --
    `emb` float32 [B, K, d_model], `rtg` and `reward` float32 [B, K] on the device, `counts` a list of B ints."""
    __slots__ = ("emb", "rtg", "reward", "counts")

    def __init__(self, emb, rtg, reward, counts):
        self.emb, self.rtg, self.reward, self.counts = emb, rtg, reward, counts

    def __repr__(self):
        return f"WindowResult(K={self.rtg.shape[1]}, counts={self.counts})"


def check_frame_contexts(frames: torch.Tensor, obs_seq: Optional[torch.Tensor], batch: int, n_image: Optional[int],
                         state_dim: int):
    """The shape rules of lram_prefill_frames / lram_score_frames, checked on the host (no GPU needed).  `frames`: uint8
    [n, L, C, H, W] with n = batch without a slot table (n_image None), else the table's n_image image slots (at least one).
    `obs_seq`: float32 [batch, L, state_dim], required exactly when the table holds vector slots (n_image < batch); otherwise
    nobody reads it and it is not looked at.  Returns (L, C, H, W); raises ValueError."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 5:
        got = f"{frames.dtype} {tuple(frames.shape)}" if isinstance(frames, torch.Tensor) else type(frames).__name__
        raise ValueError(f"frames: expected a uint8 tensor [n, L, C, H, W], got {got}")
    if n_image is not None and n_image < 1:
        raise ValueError("frames: the slot table holds no image slot, so there is no frame to take")
    n = batch if n_image is None else n_image
    if frames.shape[0] != n:
        what = "one row per env slot" if n_image is None else "one row per image slot of the slot table, in slot order"
        raise ValueError(f"frames: expected {n} rows ({what}), got {frames.shape[0]}")
    L, C, H, W = (int(x) for x in frames.shape[1:])
    if min(L, C, H, W) < 1:
        raise ValueError(f"frames: every extent of [n, L, C, H, W] must be >= 1, got {tuple(frames.shape)}")
    mixed = n_image is not None and n_image < batch
    if mixed:
        if obs_seq is None:
            raise ValueError("obs_seq: the slot table holds vector slots, their observations [batch, L, state_dim] are needed")
        if obs_seq.dtype != torch.float32 or tuple(obs_seq.shape) != (batch, L, state_dim):
            raise ValueError(f"obs_seq: expected float32 {(batch, L, state_dim)}, got {obs_seq.dtype} {tuple(obs_seq.shape)}")
    return L, C, H, W


def context_plan(L: int, lengths, cap: int):
    """Mirror of lram_context_plan: the ascending call-timesteps at which the chunks of a call of L timesteps over contexts of
    per-env length start.  The contexts are end-aligned inside the call (env b starts at s_b = L - lengths[b]); the plan begins
    at the smallest s_b over envs with a context, holds every distinct s_b, and cuts each stretch between two of them into
    equal chunks of at most `cap` timesteps.  Where no env starts inside the call the plan is the dense call's: chunks of
    `cap` from 0 on."""
    lengths = check_context_lengths(lengths, len(lengths), L)
    if cap < 1:
        raise ValueError("cap must be >= 1")
    bounds = sorted({L - n for n in lengths if n > 0})
    if bounds == [0]:
        return list(range(0, L, cap))
    bounds.append(L)
    starts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        n = -(-(hi - lo) // cap)
        starts.extend(range(lo, hi, -(-(hi - lo) // n)))
    return starts


def _prefill_tail(eng, call, discrete, want_action: bool):
    """What Engine.prefill() and prefill_frames() share behind their inputs: the action buffers of the call's rows (none unless
    want_action), the call, the result."""
    act = _context_rows_of(eng, eng._actions) if want_action else None
    tok = _context_rows_of(eng, eng._tokens) if want_action else None
    call(_head_mode(discrete), _ptr(act), _ptr(tok))
    return (act, tok) if want_action else (None, None)


def _score_tail(eng, context_call, actions, tokens, valid, discrete, over, temperature, want, logits) -> ScoreResult:
    """What Engine.score() and score_frames() share: `want`, then the inputs (context_call() checks them and returns (L, call)),
    the targets and `valid`, the zeroed ScoreResult, the call."""
    B, A = _context_batch(eng), eng.spec.act_dim
    want = (want,) if isinstance(want, str) else tuple(want)
    for w in want:
        if w not in ("actions", "tokens", "logp"):
            raise ValueError(f'want: unknown output {w!r} (choose among "actions", "tokens", "logp")')
    L, call = context_call()
    if actions is not None:
        _chk_dev(actions, torch.float32, (B, L, A), eng.device, "actions")
    if tokens is not None:
        _chk_dev(tokens, torch.int32, (B, L, A), eng.device, "tokens")
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        _chk_dev(valid, torch.uint8, (B, L), eng.device, "valid")
    # zeroed: the entries the call leaves alone (the logits of masked timesteps) must not depend on the allocator

    def zeros(asked, dtype, *tail):
        return torch.zeros(B, L, A, *tail, dtype=dtype, device=eng.device) if asked else None
    res = ScoreResult(actions=zeros("actions" in want, torch.float32), tokens=zeros("tokens" in want, torch.int32),
                      logp=zeros("logp" in want, torch.float32), logits=zeros(logits, torch.float32, eng.spec.n_vocab))
    call(_head_mode(discrete), _ptr(actions), _ptr(tokens), _ptr(valid), _over_mode(over), float(temperature), _ptr(res.actions),
         _ptr(res.tokens), _ptr(res.logp), _ptr(res.logits))
    return res


class Engine:
    """One engine per GPU: weights + per-env recurrent state resident in HBM, one batched env-step per call.

    Mirrors what the reference keeps on the agent (`policy`, `past_key_values` / `inference_params`,
    src/algos/decision_transformer_sb3.py:86-104, src/algos/decision_mamba.py:29-38) for B envs at once."""

    def __init__(self, spec: ModelSpec, state_dict: Dict[str, torch.Tensor], batch: int, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("lram_amd.Engine needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = load_library()
        self.spec = spec
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.batch = 0
        self._h = ctypes.c_void_p()
        cfg = make_config(spec)
        _check(self.lib, self.lib.lram_create(ctypes.byref(cfg), self.device.index, ctypes.byref(self._h)))
        self.load_weights(state_dict)
        self.alloc(batch)

    # -- lifetime --------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.lram_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights / state -------------------------------------------------------------------------
    def load_weights(self, state_dict: Dict[str, torch.Tensor]):
        packed = engine_layout(self.spec, state_dict)
        for name, t in packed.items():
            t = t.contiguous()
            _check(self.lib, self.lib.lram_set_weight(self._h, name.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()))
        _check(self.lib, self.lib.lram_finalize(self._h))

    def alloc(self, batch: int):
        _check(self.lib, self.lib.lram_state_alloc(self._h, int(batch)))
        self.batch = int(batch)
        self._live = self.batch
        self._context_rows = "all"   # (lram_state_alloc sets the mode back)
        self._slot_image = None      # host copy of the slot table's image column (a new allocation drops the table)
        self._mask_words = None      # keeps the packed words of set_action_mask alive during the call (the engine copies them)
        self._n_img_live = 0         # image slots below `live`: the frames step_slots is handed
        self._window_K = 0           # (lram_state_alloc frees the window ring)
        self._window_slots = "shared"
        B, A = self.batch, self.spec.act_dim
        # zeroed: a discrete head writes column 0 only, and the columns it leaves alone must not depend on what the allocator
        # hands out (two runs on the same inputs return the same tensors)
        self._actions = torch.zeros(B, A, dtype=torch.float32, device=self.device)
        self._tokens = torch.zeros(B, A, dtype=torch.int32, device=self.device)

    def state_bytes_per_env(self) -> int:
        return int(self.lib.lram_state_bytes_per_env(self._h))

    def reset(self, env_mask: Optional[torch.Tensor] = None):
        """Zero recurrent state of masked env slots (all when None): `past_key_values = None`."""
        if env_mask is not None:
            env_mask = env_mask.to(device=self.device, dtype=torch.uint8).contiguous()
            _chk_dev(env_mask, torch.uint8, (self.batch,), self.device, "env_mask")
        _check(self.lib, self.lib.lram_reset(self._h, _ptr(env_mask), _stream_ptr(self.device)))

    # -- the hot path ----------------------------------------------------------------------------
    def _step_io(self, rtg, reward, reset_mask, out_actions, out_tokens):
        """What step(), step_images() and step_slots() share: checks rtg, reward and the reset mask of the live rows and
        returns the checked output buffers (actions, tokens) -- the engine's own unless the caller handed some in."""
        B, A = self._live, self.spec.act_dim
        _chk_dev(rtg, torch.float32, (B,), self.device, "rtg")
        _chk_dev(reward, torch.float32, (B,), self.device, "reward")
        if reset_mask is not None:
            _chk_dev(reset_mask, torch.uint8, (B,), self.device, "reset_mask")
        actions = self._live_rows(self._actions) if out_actions is None else out_actions
        tokens = self._live_rows(self._tokens) if out_tokens is None else out_tokens
        _chk_dev(actions, torch.float32, (B, A), self.device, "out_actions")
        _chk_dev(tokens, torch.int32, (B, A), self.device, "out_tokens")
        return actions, tokens

    def step(self, obs: torch.Tensor, rtg: torch.Tensor, reward: torch.Tensor,
             reset_mask: Optional[torch.Tensor] = None, discrete=False, obs_is_embedding: bool = False,
             out_actions: Optional[torch.Tensor] = None, out_tokens: Optional[torch.Tensor] = None):
        """One env-step for all live slots (B = `live`: the whole batch unless set_live parked some).  Inputs are device
        tensors (already resident in HBM).
        Returns (actions float32 [B, act_dim], tokens int32 [B, act_dim]); valid once the current
        stream has executed.  discrete=True: column 0 holds the action index; discrete="per_slot": the head mode of
        every slot comes from the slot table (set_slot_table)."""
        B, spec = self._live, self.spec
        _chk_dev(obs, torch.float32, (B, spec.d_model if obs_is_embedding else spec.state_dim), self.device, "obs")
        actions, tokens = self._step_io(rtg, reward, reset_mask, out_actions, out_tokens)
        _check(self.lib, self.lib.lram_step(self._h, _ptr(obs), int(obs_is_embedding), _ptr(rtg), _ptr(reward),
                                            _ptr(reset_mask), _head_mode(discrete), _ptr(actions), _ptr(tokens),
                                            _stream_ptr(self.device)))
        return actions, tokens

    # -- mixed-domain batches --------------------------------------------------------------------
    def set_slot_table(self, discrete=None, act_dim=None, image=None):
        """Per env slot: head mode (bool), action dims in use (int, 1 .. spec.act_dim; 1 for a discrete slot) and observation
        kind (bool: uint8 frame) -- arrays of length `batch` (lram_set_slot_table).  set_slot_table(None) clears the table.
        Synchronises and drops a captured graph: not a hot-path call."""
        if discrete is None and act_dim is None and image is None:
            _check(self.lib, self.lib.lram_set_slot_table(self._h, None, None))
            self._slot_image, self._n_img_live = None, 0
            return
        B = self.batch
        d = torch.as_tensor(discrete).reshape(-1).to("cpu")
        a = torch.as_tensor(act_dim).reshape(-1).to("cpu")
        i = torch.zeros(B, dtype=torch.bool) if image is None else torch.as_tensor(image).reshape(-1).to("cpu")
        for name, t in (("discrete", d), ("act_dim", a), ("image", i)):
            if t.numel() != B:
                raise ValueError(f"{name}: expected {B} entries (one per env slot), got {t.numel()}")
            if t.dtype.is_floating_point or t.dtype.is_complex:
                raise ValueError(f"{name}: expected a bool / integer array, got {t.dtype}")
        if bool(((a < 0) | (a > 255)).any()):
            raise ValueError("act_dim: entries must be in 1 .. spec.act_dim")
        flags = (d.bool().to(torch.uint8) * LRAM_SLOT_DISCRETE + i.bool().to(torch.uint8) * LRAM_SLOT_IMAGE).contiguous()
        acts = a.to(torch.uint8).contiguous()
        _check(self.lib, self.lib.lram_set_slot_table(self._h, ctypes.c_void_p(flags.data_ptr()),
                                                      ctypes.c_void_p(acts.data_ptr())))
        self._slot_image = i.bool().clone()
        self._n_img_live = int(self._slot_image[:self._live].sum())

    def set_action_mask(self, allowed):
        """Allowed-action sets (lram_set_action_mask): bool [batch, n_vocab] (tensor or array), allowed[b, t] = env slot b may
        take vocabulary token t; None clears the mask.  Every head kernel then works on the slot's sub-row: the argmax, a
        draw, its log-probability and over="selectable" scores; over="vocab" and raw logits are unchanged.  The sets stay
        with the slot index.  Synchronises and drops a captured graph: not a hot-path call."""
        if allowed is None:
            _check(self.lib, self.lib.lram_set_action_mask(self._h, None, 0))
            return
        spec = self.spec
        table = self.slot_table()
        m = check_action_mask(allowed, self.batch, spec.n_vocab, spec.n_discrete, None if table is None else table["discrete"])
        self._mask_words = pack_action_mask(m)
        _check(self.lib, self.lib.lram_set_action_mask(self._h, ctypes.c_void_p(self._mask_words.data_ptr()),
                                                       int(self._mask_words.shape[1])))

    @property
    def action_mask(self) -> Optional[torch.Tensor]:
        """The mask in effect (lram_get_action_mask): bool [batch, n_vocab] on the CPU, or None."""
        on = ctypes.c_int32(0)
        words = torch.zeros(self.batch, (self.spec.n_vocab + 31) // 32, dtype=torch.int32)
        _check(self.lib, self.lib.lram_get_action_mask(self._h, ctypes.c_void_p(words.data_ptr()), int(words.shape[1]),
                                                       ctypes.byref(on)))
        return unpack_action_mask(words, self.spec.n_vocab) if on.value else None

    def slot_table(self) -> Optional[dict]:
        """The table in effect (lram_get_slot_table): {"discrete": bool [B], "act_dim": int64 [B], "image": bool [B],
        "n_image": int} as CPU tensors, or None when no table is set."""
        try:
            n = self.n_image_slots
        except LramError:
            return None
        flags = torch.empty(self.batch, dtype=torch.uint8)
        acts = torch.empty(self.batch, dtype=torch.uint8)
        _check(self.lib, self.lib.lram_get_slot_table(self._h, ctypes.c_void_p(flags.data_ptr()),
                                                      ctypes.c_void_p(acts.data_ptr()), None))
        return {"discrete": (flags & LRAM_SLOT_DISCRETE) != 0, "act_dim": acts.to(torch.int64),
                "image": (flags & LRAM_SLOT_IMAGE) != 0, "n_image": n}

    @property
    def n_image_slots(self) -> int:
        n = ctypes.c_int32(0)
        _check(self.lib, self.lib.lram_get_slot_table(self._h, None, None, ctypes.byref(n)))
        return int(n.value)

    def step_slots(self, obs: Optional[torch.Tensor], images: Optional[torch.Tensor], rtg: torch.Tensor,
                   reward: torch.Tensor, reset_mask: Optional[torch.Tensor] = None,
                   out_actions: Optional[torch.Tensor] = None, out_tokens: Optional[torch.Tensor] = None):
        """One env-step of a mixed batch (lram_step_slots): obs float32 [B, state_dim] (rows of image slots are never read),
        images uint8 [n_image, C, H, W] -- frame k belongs to the k-th image slot in ascending slot order; None when the table
        holds no image slot.  Head mode per slot: a continuous slot fills columns < its act_dim, a discrete slot column 0 (the
        action index); every other column holds 0.0 / token -1.  Returns (actions, tokens) as step()."""
        B, spec = self._live, self.spec
        n_img = self.n_image_slots   # raises when no table is set
        if B < self.batch:           # parked slots hand in no frame: the image slots of the live prefix (counted by
            n_img = self._n_img_live  # set_slot_table / set_live, not per step)
        if obs is None:
            if n_img != B:
                raise ValueError("obs: None is allowed only when every slot is an image slot")
        else:
            _chk_dev(obs, torch.float32, (B, spec.state_dim), self.device, "obs")
        c = h = w = 0
        if n_img > 0:
            if images is None or images.dim() != 4:
                raise ValueError("images must be [n_image, C, H, W]")
            _chk_dev(images, torch.uint8, (n_img, *images.shape[1:]), self.device, "images")
            c, h, w = (int(x) for x in images.shape[1:])
        elif images is not None and images.shape[0] != 0:
            raise ValueError(f"images: the slot table holds no image slot, got {images.shape[0]} frames")
        actions, tokens = self._step_io(rtg, reward, reset_mask, out_actions, out_tokens)
        _check(self.lib, self.lib.lram_step_slots(self._h, _ptr(obs), _ptr(images) if n_img > 0 else None, c, h, w, _ptr(rtg),
                                                  _ptr(reward), _ptr(reset_mask), _ptr(actions), _ptr(tokens),
                                                  _stream_ptr(self.device)))
        return actions, tokens

    def _stored_context_call(self, kind: str, obs_seq, rtg_seq, reward_seq, reset_mask, obs_is_embedding, lengths, append):
        """What prefill() and score() share: checks the [B, L, .] inputs and the reset mask, and returns (L, call).  call(*tail)
        checks and normalises `lengths`, picks the C entry -- dense without lengths, else the append or the ragged (replace)
        one -- and runs it: the arguments up to the reset mask from here, `tail` (from the head mode on) behind them."""
        B, spec = _context_batch(self), self.spec
        L = obs_seq.shape[1]
        _chk_dev(obs_seq, torch.float32, (B, L, spec.d_model if obs_is_embedding else spec.state_dim), self.device,
                 "obs_seq")
        _chk_dev(rtg_seq, torch.float32, (B, L), self.device, "rtg_seq")
        _chk_dev(reward_seq, torch.float32, (B, L), self.device, "reward_seq")
        if reset_mask is not None:
            _chk_dev(reset_mask, torch.uint8, (B,), self.device, "reset_mask")
        lib = self.lib

        def call(*tail):
            head = (self._h, _ptr(obs_seq), int(obs_is_embedding), _ptr(rtg_seq), _ptr(reward_seq), int(L))
            tail = (_ptr(reset_mask), *tail, _stream_ptr(self.device))
            if lengths is None:
                _check(lib, lib.lram_prefill(*head, *tail) if kind == "prefill" else lib.lram_score(*head, *tail))
                return
            fn = {("prefill", False): lib.lram_prefill_ragged, ("prefill", True): lib.lram_prefill_append,
                  ("score", False): lib.lram_score_ragged, ("score", True): lib.lram_score_append}[kind, bool(append)]
            _check(lib, fn(*head, _i32_array(check_context_lengths(lengths, B, L)), *tail))
        return L, call

    def _frames_context_call(self, kind: str, frames, obs_seq, rtg_seq, reward_seq, reset_mask, lengths, append):
        """_stored_context_call for frames: checks the inputs (check_frame_contexts) and returns (L, call); call(*tail) runs
        lram_prefill_frames / lram_score_frames with `tail` (from the head mode on) behind the reset mask."""
        B = _context_batch(self)   # (the image slots among the rows of the call hand in frames)
        n_img = int(self._slot_image[:B].sum()) if self._slot_image is not None else None   # (None: no slot table)
        L, C, H, W = check_frame_contexts(frames, obs_seq, B, n_img, self.spec.state_dim)
        _chk_dev(frames, torch.uint8, tuple(frames.shape), self.device, "frames")
        if n_img is None or n_img == B:
            obs_seq = None   # (every slot takes frames: nobody reads it)
        if obs_seq is not None:
            _chk_dev(obs_seq, torch.float32, (B, L, self.spec.state_dim), self.device, "obs_seq")
        _chk_dev(rtg_seq, torch.float32, (B, L), self.device, "rtg_seq")
        _chk_dev(reward_seq, torch.float32, (B, L), self.device, "reward_seq")
        if reset_mask is not None:
            _chk_dev(reset_mask, torch.uint8, (B,), self.device, "reset_mask")
        host = None if lengths is None else _i32_array(check_context_lengths(lengths, B, L))
        fn = self.lib.lram_prefill_frames if kind == "prefill" else self.lib.lram_score_frames

        def call(*tail):
            _check(self.lib, fn(self._h, _ptr(frames), C, H, W, _ptr(obs_seq), _ptr(rtg_seq), _ptr(reward_seq), L, host,
                                int(bool(append)), _ptr(reset_mask), *tail, _stream_ptr(self.device)))
        return L, call

    def prefill_frames(self, frames: torch.Tensor, rtg_seq: torch.Tensor, reward_seq: torch.Tensor,
                       obs_seq: Optional[torch.Tensor] = None, lengths=None, append=False,
                       reset_mask: Optional[torch.Tensor] = None, discrete=False, want_action: bool = True):
        """prefill() from uint8 frames [n, L, C, H, W] (lram_prefill_frames): the IMPALA CNN embeds the frames inside the call,
        and with `lengths` only the frames [b, l] with l < lengths[b] -- padded frames are never read or convolved.  Without a
        slot table n = batch; with one, n = its image slots in ascending slot order (as step_slots takes frames) and `obs_seq`
        float32 [B, L, state_dim] carries the vector slots' observations (rows of image slots are computed and overwritten:
        anything, NaN included, may stand there).  `lengths`, `append`, `reset_mask`, `discrete`, `want_action` and the
        result as in prefill().  Bit-identical to prefill(embed_frames(frames), obs_is_embedding=True) for a dense call."""
        self._need_all_live("prefill_frames")
        _, call = self._frames_context_call("prefill", frames, obs_seq, rtg_seq, reward_seq, reset_mask, lengths, append)
        return _prefill_tail(self, call, discrete, want_action)

    def score_frames(self, frames: torch.Tensor, rtg_seq: torch.Tensor, reward_seq: torch.Tensor, *,
                     obs_seq: Optional[torch.Tensor] = None, lengths=None, append=False,
                     actions: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None,
                     valid: Optional[torch.Tensor] = None, reset_mask: Optional[torch.Tensor] = None, discrete=False,
                     over: str = "vocab", temperature: float = 1.0, want=("actions", "tokens", "logp"),
                     logits: bool = False) -> ScoreResult:
        """score() from uint8 frames (lram_score_frames): `frames` / `obs_seq` as in prefill_frames(), everything else as in
        score()."""
        self._need_all_live("score_frames")
        return _score_tail(self, lambda: self._frames_context_call("score", frames, obs_seq, rtg_seq, reward_seq, reset_mask, lengths,
                                                                  append),
                                actions, tokens, valid, discrete, over, temperature, want, logits)

    def prefill(self, obs_seq: torch.Tensor, rtg_seq: torch.Tensor, reward_seq: torch.Tensor,
                reset_mask: Optional[torch.Tensor] = None, discrete=False, obs_is_embedding: bool = False,
                want_action: bool = True, lengths=None, append: bool = False):
        """L stored timesteps in one call ([B, L, state_dim], [B, L], [B, L]); == L sequential step() calls.
        Returns (actions, tokens) of the last timestep (None when want_action is False).
        `lengths` (list / array / integer tensor of B entries, moved to the host; lram_prefill_ragged): env b's context is rows
        [b, :lengths[b]] (left-aligned; the rows behind it are ignored), its state afterwards is that of its own context and its
        action the one at its own last timestep.  A length below L replaces the slot's state (the slot is reset first whatever
        `reset_mask` says); length L behaves as without lengths; length 0 leaves the slot alone (action 0, token -1).
        `append=True` with lengths (lram_prefill_append): env b's lengths[b] timesteps are APPENDED to the state the slot holds;
        `reset_mask[b]` alone decides whether it restarts before its first timestep (no mask: nobody does), and a slot of
        length 0 is held -- no kernel writes its state.  Without lengths, append changes nothing: the dense call."""
        self._need_all_live("prefill")
        L, call = self._stored_context_call("prefill", obs_seq, rtg_seq, reward_seq, reset_mask, obs_is_embedding, lengths, append)
        return _prefill_tail(self, call, discrete, want_action)

    def score(self, obs_seq: torch.Tensor, rtg_seq: torch.Tensor, reward_seq: torch.Tensor, *,
              actions: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None,
              valid: Optional[torch.Tensor] = None, reset_mask: Optional[torch.Tensor] = None, discrete=False,
              over: str = "vocab", temperature: float = 1.0, want=("actions", "tokens", "logp"), logits: bool = False,
              obs_is_embedding: bool = False, lengths=None, append: bool = False) -> ScoreResult:
        """Score L stored timesteps in one call (lram_score): prefill() with the action head at EVERY timestep -- the
        reference's no-cache forward plus the loss it takes from the logits (universal_decision_transformer_sb3.py:398-434).
        `actions` float32 [B, L, act_dim] (recorded actions, tokenised on the device) or `tokens` int32 [B, L, act_dim] are the
        targets of `logp`; `valid` uint8 / bool [B, L] masks outputs only (the state advances through every timestep);
        over="vocab" normalises over all n_vocab logits (the reference's cross-entropy), "selectable" over the range the head
        picks from; `temperature` multiplies the logits.  `want` names the outputs among "actions", "tokens", "logp";
        logits=True adds the raw logits.  The state afterwards equals prefill()'s; nothing is drawn in sampling mode.
        `lengths` as in prefill() (lram_score_ragged): rows [b, l] with l >= lengths[b] are masked, and the state afterwards is
        that of every env's own context.  `append=True` with lengths (lram_score_append): as in prefill() -- the contexts
        continue the slots' states, which is how a trajectory longer than one call is scored window by window."""
        self._need_all_live("score")
        if obs_seq.dim() != 3:
            raise ValueError("obs_seq must be [B, L, state_dim]")
        return _score_tail(self, lambda: self._stored_context_call("score", obs_seq, rtg_seq, reward_seq, reset_mask, obs_is_embedding,
                                                                  lengths, append),
                                actions, tokens, valid, discrete, over, temperature, want, logits)

    def last_logp(self, tokens: torch.Tensor, over: str = "selectable", temperature: float = 1.0) -> torch.Tensor:
        """Log-probabilities float32 [B, act_dim] of `tokens` (int32 [B, act_dim]: what step / prefill just returned) under the
        logits of the last action-producing call (lram_score_last).  over="selectable" with the armed temperature is the
        distribution an unfiltered sampling head draws from; top-k / top-p are not applied.
        over="sampled" (lram_score_last_sampled): under the distribution the armed head draws from -- the per-slot settings
        where set_sampling_slots set a table, those of set_sampling otherwise, top-k / top-p applied (a token outside the
        support scores -inf, a greedy slot's argmax token 0).  `temperature` must then be left at its default: the armed one
        is used."""
        B, A = self._live, self.spec.act_dim   # (the live rows: what the last step returned)
        _chk_dev(tokens, torch.int32, (B, A), self.device, "tokens")
        out = torch.zeros(B, A, dtype=torch.float32, device=self.device)
        if over == "sampled":
            if float(temperature) != 1.0:
                raise ValueError('last_logp(over="sampled") scores under the armed settings: leave `temperature` at its default')
            _check(self.lib, self.lib.lram_score_last_sampled(self._h, _ptr(tokens), _ptr(out), _stream_ptr(self.device)))
            return out
        _check(self.lib, self.lib.lram_score_last(self._h, _ptr(tokens), _over_mode(over), float(temperature), _ptr(out),
                                                  _stream_ptr(self.device)))
        return out

    def embed_images(self, images: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 frames [B, C, H, W] -> state-token embeddings [B, d_model] through the IMPALA CNN kernels
        (`self.embed_image(state / 255)`, online_decision_transformer_model.py:523-526); feed the result to
        step(..., obs_is_embedding=True).  Needs the embed_image.* weights in the state dict."""
        B, D = self.batch, self.spec.d_model
        if images.dim() != 4:
            raise ValueError("images must be [B, C, H, W]")
        _chk_dev(images, torch.uint8, (B, *images.shape[1:]), self.device, "images")
        if out is None:
            out = torch.empty(B, D, dtype=torch.float32, device=self.device)
        _chk_dev(out, torch.float32, (B, D), self.device, "out")
        _check(self.lib, self.lib.lram_embed_images(self._h, _ptr(images), int(images.shape[1]), int(images.shape[2]),
                                                    int(images.shape[3]), _ptr(out), _stream_ptr(self.device)))
        return out

    def embed_frames(self, frames: torch.Tensor) -> torch.Tensor:
        """uint8 frames [..., C, H, W], any number of them -> [..., d_model] (lram_embed_frames): embed_images' arithmetic
        through the tiled frame-list path of prefill_frames; the result does not depend on LRAM_IMG_TILE."""
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() < 4:
            raise ValueError("frames: expected a uint8 tensor [..., C, H, W]")
        lead, (C, H, W) = tuple(frames.shape[:-3]), (int(x) for x in frames.shape[-3:])
        n = 1
        for x in lead:
            n *= int(x)
        if n < 1 or min(C, H, W) < 1:
            raise ValueError(f"frames: no frame in a tensor of shape {tuple(frames.shape)}")
        _chk_dev(frames, torch.uint8, tuple(frames.shape), self.device, "frames")
        out = torch.empty(*lead, self.spec.d_model, dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.lram_embed_frames(self._h, _ptr(frames), n, C, H, W, _ptr(out), _stream_ptr(self.device)))
        return out

    def image_counts(self, reset: bool = False) -> dict:
        """What the frame-list front end has done since the last reset (lram_image_counts): "frames" convolved, "tiles"
        launched, "linear" launches.  Padded frames are not among the frames."""
        buf = (ctypes.c_int64 * 3)()
        _check(self.lib, self.lib.lram_image_counts(self._h, buf, 1 if reset else 0))
        return {"frames": int(buf[0]), "tiles": int(buf[1]), "linear": int(buf[2])}

    def step_images(self, images: torch.Tensor, rtg: torch.Tensor, reward: torch.Tensor,
                    reset_mask: Optional[torch.Tensor] = None, discrete=False,
                    out_actions: Optional[torch.Tensor] = None, out_tokens: Optional[torch.Tensor] = None):
        """One env-step from uint8 frames [B, C, H, W]: embed_images + step(obs_is_embedding=True) as one call (the reference's
        forward embeds image states inside `compute_inputs`, online_decision_transformer_model.py:463-530).  Same results as the two
        calls; the CNN runs per env slice beside the step's observation-independent state-pass work."""
        if images.dim() != 4:
            raise ValueError("images must be [B, C, H, W]")
        _chk_dev(images, torch.uint8, (self._live, *images.shape[1:]), self.device, "images")
        actions, tokens = self._step_io(rtg, reward, reset_mask, out_actions, out_tokens)
        _check(self.lib, self.lib.lram_step_images(self._h, _ptr(images), int(images.shape[1]), int(images.shape[2]),
                                                   int(images.shape[3]), _ptr(rtg), _ptr(reward), _ptr(reset_mask),
                                                   _head_mode(discrete), _ptr(actions), _ptr(tokens), _stream_ptr(self.device)))
        return actions, tokens

    def encoder_step(self, inputs_embeds: torch.Tensor, reset_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`self.encoder(inputs_embeds=[B,T,D], use_cache=True)` plug point (decision_xlstm.py:138-169)."""
        self._need_all_live("encoder_step")
        B, D = _context_batch(self), self.spec.d_model
        T = inputs_embeds.shape[1]
        _chk_dev(inputs_embeds, torch.float32, (B, T, D), self.device, "inputs_embeds")
        if reset_mask is not None:
            _chk_dev(reset_mask, torch.uint8, (B,), self.device, "reset_mask")
        out = torch.empty_like(inputs_embeds)
        _check(self.lib, self.lib.lram_encoder_step(self._h, _ptr(inputs_embeds), int(T), _ptr(reset_mask), _ptr(out),
                                                    _stream_ptr(self.device)))
        return out

    def taps(self):
        """(embed_ln tokens [B,T,D], encoder hidden [B,T,D], logits [B, act_dim*n_vocab]) of the last step (B = `live`)."""
        B, s = self._live, self.spec
        hid = torch.empty(B, s.tokens_per_step, s.d_model, dtype=torch.float32, device=self.device)
        tok = torch.empty_like(hid) if self.batch <= 1024 else None   # the token tap is kept for small batches only
        logits = torch.empty(B, s.act_dim * s.n_vocab, dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.lram_get_taps(self._h, _ptr(tok), _ptr(hid), _ptr(logits), _stream_ptr(self.device)))
        return tok, hid, logits

    # -- past_key_values-compatible state access -------------------------------------------------
    def _state_shape(self, block: int, which: int):
        s, B = self.spec, self.batch
        if s.backbone == "mamba":
            return {0: (B, s.d_inner, s.d_state), 3: (B, s.d_inner, s.d_conv)}.get(which)
        if block in s.slstm_at:
            return {0: (4, B, s.d_model), 3: (B, s.conv_k, s.d_model)}.get(which)
        dh = s.head_dim
        return {0: (B, s.n_heads, dh, dh), 1: (B, s.n_heads, dh, 1), 2: (B, s.n_heads, 1, 1),
                3: (B, s.conv_k, s.inner)}.get(which)

    def export_state_tensor(self, block: int, which: int) -> torch.Tensor:
        shape = self._state_shape(block, which)
        n = int(self.lib.lram_state_numel(self._h, block, which))
        if shape is None or n == 0:
            raise KeyError(f"no state tensor (block={block}, which={which})")
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        assert out.numel() == n
        _check(self.lib, self.lib.lram_state_export(self._h, block, which, _ptr(out), _stream_ptr(self.device)))
        return out

    def import_state_tensor(self, block: int, which: int, t: torch.Tensor):
        shape = self._state_shape(block, which)
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if shape is None or tuple(t.shape) != tuple(shape):
            raise ValueError(f"state tensor (block={block}, which={which}) must have shape {shape}, got {tuple(t.shape)}")
        _check(self.lib, self.lib.lram_state_import(self._h, block, which, _ptr(t), _stream_ptr(self.device)))

    def export_past_key_values(self):
        """State in the reference's layout: xLSTM nested dict of tuples, Mamba
        {layer_idx: (conv_state, ssm_state)} (src/algos/decision_mamba.py:9-25)."""
        s = self.spec
        if s.backbone == "mamba":
            return {i: (self.export_state_tensor(i, 3), self.export_state_tensor(i, 0)) for i in range(s.n_blocks)}
        out = {}
        for i in range(s.n_blocks):
            if i in s.slstm_at:
                out[f"block_{i}"] = {"slstm_state": self.export_state_tensor(i, 0),
                                     "conv_state": (self.export_state_tensor(i, 3),)}
            else:
                out[f"block_{i}"] = {"mlstm_state": tuple(self.export_state_tensor(i, w) for w in (0, 1, 2)),
                                     "conv_state": (self.export_state_tensor(i, 3),)}
        return out

    def import_past_key_values(self, pkv):
        s = self.spec
        if s.backbone == "mamba":
            for i, (conv, ssm) in pkv.items():
                self.import_state_tensor(int(i), 3, conv)
                self.import_state_tensor(int(i), 0, ssm)
            return
        for i in range(s.n_blocks):
            blk = pkv[f"block_{i}"]
            if i in s.slstm_at:
                self.import_state_tensor(i, 0, blk["slstm_state"])
            else:
                for w, t in enumerate(blk["mlstm_state"]):
                    self.import_state_tensor(i, w, t)
            self.import_state_tensor(i, 3, blk["conv_state"][0])

    # -- live prefix: step only the slots that have something to do --------------------------------
    @property
    def live(self) -> int:
        """Slots [0, live) are live, [live, batch) parked (lram_get_live)."""
        return self._live

    def set_live(self, n: int):
        """The first `n` slots (1 .. batch) are live from now on; the others are parked: they keep their recurrent state and
        no row of them is computed (lram_set_live; lazy mode still carries their bookkeeping over each step).  step / step_images / step_slots / last_logp / taps then take and return `n` rows;
        prefill / score / encoder_step raise until every slot is live again, unless set_context_rows says otherwise.  Cheap: no synchronisation, no allocation."""
        _check(self.lib, self.lib.lram_set_live(self._h, int(n), _stream_ptr(self.device)))
        self._live = int(self.lib.lram_get_live(self._h))
        if self._slot_image is not None:
            self._n_img_live = int(self._slot_image[:self._live].sum())

    def swap_slots(self, a, b):
        """Exchange the recurrent state of slots a[i] and b[i], live or parked, in one launch (lram_state_swap_slots).  All
        indices distinct and in range.  Slot-table entries, per-slot sampling settings and the sampling stream stay with the
        slot index."""
        a, b = check_swap_lists(a, b, self.batch)
        _check(self.lib, self.lib.lram_state_swap_slots(self._h, _i32_array(a), _i32_array(b), len(a),
                                                        _stream_ptr(self.device)))

    # -- context rows: stored contexts and encoder calls on the live prefix -------------------------
    @property
    def context_rows(self) -> str:
        """Which slots prefill / score / their frames forms / encoder_step run on (lram_get_context_rows): "all", "live" or
        "started"."""
        return self._context_rows

    def set_context_rows(self, mode: str):
        """"all" (the default; alloc() sets it back): every allocated slot, and the calls raise while slots are parked.
        "live": the live prefix -- inputs, lengths, reset mask and results have `live` rows, parked slots are left alone.
        "started": "live", and a call with `lengths` -- which must then not increase in slot order -- runs in every chunk only
        the envs that have started by it: no held rows, no rows on zero tokens, no record saved for a slot of length 0.
        Cheap: host bookkeeping only (lram_set_context_rows)."""
        if mode not in CONTEXT_ROWS:
            raise ValueError(f'context rows: unknown mode {mode!r} (choose among "all", "live", "started")')
        _check(self.lib, self.lib.lram_set_context_rows(self._h, CONTEXT_ROWS.index(mode)))
        self._context_rows = mode

    def context_counts(self, reset: bool = False) -> dict:
        """What the stored-context entries have done since the last reset (lram_context_counts): "calls", "chunks" run,
        "env_timesteps" computed (the sum over chunks of rows x timesteps), "kept" slot records saved and restored."""
        buf = (ctypes.c_int64 * 4)()
        _check(self.lib, self.lib.lram_context_counts(self._h, buf, 1 if reset else 0))
        return {"calls": int(buf[0]), "chunks": int(buf[1]), "env_timesteps": int(buf[2]), "kept": int(buf[3])}

    # -- context-window inference: the reference's cache-off evaluation ---------------------------------
    @property
    def window_timesteps(self) -> int:
        """K of the ring alloc_window() made; 0: none (alloc() frees it)."""
        return getattr(self, "_window_K", 0)

    def alloc_window(self, K: int):
        """The device ring of every env slot's last K timesteps (lram_window_alloc): all counts 0, no pad entry, slots mode
        "shared".  K = 0 frees it.  Synchronises: not a hot-path call."""
        K = check_window_timesteps(K, self.batch, self.spec.d_model)
        _check(self.lib, self.lib.lram_window_alloc(self._h, K))
        self._window_K = K
        self._window_slots = "shared"

    def set_window_pad(self, vec: torch.Tensor, is_embedding: bool = False):
        """The pad entry of pad="reference" (lram_window_set_pad): a normalised observation float32 [state_dim], which goes
        through the state Linear, or with is_embedding a state-token embedding float32 [d_model].  The reference pads with
        zero observations before it normalises them: the vector is (0 - state_mean) / state_std."""
        vec = vec.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        _chk_dev(vec, torch.float32, (self.spec.d_model if is_embedding else self.spec.state_dim,), self.device, "vec")
        _check(self.lib, self.lib.lram_window_set_pad(self._h, _ptr(vec), int(bool(is_embedding)), _stream_ptr(self.device)))

    @property
    def window_slots(self) -> str:
        """Which slots step_window runs (lram_window_get_slots): "shared" or "own"."""
        return getattr(self, "_window_slots", "shared")

    def set_window_slots(self, mode: str):
        """"shared" (the default; alloc() and alloc_window() set it back): step_window runs every slot and raises while slots
        are parked.  "own": it runs the live prefix (set_live) -- inputs, control arrays and results have `live` rows, and a
        parked slot keeps its window, count and recurrent state bit for bit.  Cheap: host bookkeeping only
        (lram_window_set_slots)."""
        if mode not in WINDOW_SLOTS:
            raise ValueError(f'window slots: unknown mode {mode!r} (choose "shared" or "own")')
        _check(self.lib, self.lib.lram_window_set_slots(self._h, WINDOW_SLOTS.index(mode)))
        self._window_slots = mode

    def step_window(self, obs: torch.Tensor, rtg: torch.Tensor, prev_reward: torch.Tensor, reset=None, relabel=None, keep=None,
                    pad: str = "reference", discrete=False, obs_is_embedding: bool = False):
        """One env-step of the cache-off evaluation for all slots (lram_step_window): the ring takes the new timestep and the
        model runs from an empty state over every env's last K timesteps.  `obs` float32 [B, state_dim] (or [B, d_model]),
        `rtg` and `prev_reward` float32 [B] on the device; `reset` (bools), `relabel`, `keep` (ints >= 0) are HOST arrays of B
        entries or None.  Per env, in this order: reset empties the window; otherwise prev_reward becomes the reward of the
        newest entry; relabel = m rewrites the rtg of the newest m entries to the suffix sums of their rewards; keep = k
        prunes the window to its newest k entries; then (obs, rtg, reward 0) is pushed.  pad="reference": shorter windows
        are left-padded with the pad entry (set_window_pad), rtg 0 and reward 0, as the reference's pad_inputs does;
        pad="none": only the real timesteps count.  Returns (actions, tokens) as step().  The recurrent state afterwards is
        the stored-context call's: step_window and step on one engine overwrite each other's state.
        With set_window_slots("own") B is `live`: the call takes and returns `live` rows and runs slots [0, live) alone."""
        if pad not in WINDOW_PAD:
            raise ValueError(f'pad: unknown mode {pad!r} (choose "reference" or "none")')
        B, spec = (self._live if self.window_slots == "own" else self.batch), self.spec
        _chk_dev(obs, torch.float32, (B, spec.d_model if obs_is_embedding else spec.state_dim), self.device, "obs")
        _chk_dev(rtg, torch.float32, (B,), self.device, "rtg")
        _chk_dev(prev_reward, torch.float32, (B,), self.device, "prev_reward")
        reset, relabel, keep = check_window_controls(reset, relabel, keep, B)
        host_reset = None if reset is None else (ctypes.c_uint8 * B)(*reset)
        _check(self.lib, self.lib.lram_step_window(
            self._h, _ptr(obs), int(obs_is_embedding), _ptr(rtg), _ptr(prev_reward), host_reset,
            None if relabel is None else _i32_array(relabel), None if keep is None else _i32_array(keep),
            WINDOW_PAD.index(pad), _head_mode(discrete), _ptr(self._actions), _ptr(self._tokens), _stream_ptr(self.device)))
        if B != self.batch:
            return self._actions[:B], self._tokens[:B]
        return self._actions, self._tokens

    def window(self) -> WindowResult:
        """The windows as the ring holds them (lram_window_peek), of every slot, live or parked: see WindowResult."""
        B, K, D = self.batch, self.window_timesteps, self.spec.d_model
        if K < 1:
            raise LramError("window: no window ring is allocated (alloc_window)")
        emb = torch.empty(B, K, D, dtype=torch.float32, device=self.device)
        rtg = torch.empty(B, K, dtype=torch.float32, device=self.device)
        rew = torch.empty(B, K, dtype=torch.float32, device=self.device)
        counts = (ctypes.c_int32 * B)()
        _check(self.lib, self.lib.lram_window_peek(self._h, _ptr(emb), _ptr(rtg), _ptr(rew), counts, _stream_ptr(self.device)))
        return WindowResult(emb, rtg, rew, list(counts))

    # -- windows of individual env slots: they move as the recurrent state does (copy_slots / swap_slots / save_slots / load_slots)
    @property
    def window_slot_numel(self) -> int:
        """Floats in one slot's window record (lram_window_slot_numel): K * (d_model + 2) + 1."""
        if self.window_timesteps < 1:
            raise LramError("window: no window ring is allocated (alloc_window)")
        return int(self.lib.lram_window_slot_numel(self._h))

    def copy_window_slots(self, src, dst):
        """Slot dst[i]'s window -- entries and count -- becomes slot src[i]'s (lram_window_copy_slots), in one launch; `src` may
        repeat.  No other slot's window and no recurrent state is touched."""
        src, dst = check_slot_lists(src, dst, self.batch)
        _check(self.lib, self.lib.lram_window_copy_slots(self._h, _i32_array(src), _i32_array(dst), len(src),
                                                         _stream_ptr(self.device)))

    def swap_window_slots(self, a, b):
        """Exchange the windows of slots a[i] and b[i], live or parked, in one launch (lram_window_swap_slots).  All indices
        distinct and in range."""
        a, b = check_swap_lists(a, b, self.batch)
        _check(self.lib, self.lib.lram_window_swap_slots(self._h, _i32_array(a), _i32_array(b), len(a),
                                                         _stream_ptr(self.device)))

    def save_window_slots(self, slots, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Records of the listed slots' windows, float32 [n, window_slot_numel] on the device (lram_window_save_slots): per
        record the window as window() lays it out -- [K, d_model] embeddings, [K] rtg, [K] rewards, end-aligned with zeros
        ahead of the count -- then the count as one float.  Position-free: it loads into any engine of the same K and d_model."""
        slots = _slot_list(slots, "slots")
        n, numel = len(slots), self.window_slot_numel
        if out is None:
            out = torch.empty(n, numel, dtype=torch.float32, device=self.device)
        _chk_dev(out, torch.float32, (n, numel), self.device, "out")
        _check(self.lib, self.lib.lram_window_save_slots(self._h, _i32_array(slots), n, _ptr(out), _stream_ptr(self.device)))
        return out

    def load_window_slots(self, slots, records: torch.Tensor):
        """Write records [n, window_slot_numel] (as save_window_slots returns) into the listed slots' windows
        (lram_window_load_slots).  Reads the n counts back: synchronises the stream."""
        slots, _ = check_slot_lists(slots, None, self.batch)
        records = records.to(device=self.device, dtype=torch.float32).contiguous()
        _chk_dev(records, torch.float32, (len(slots), self.window_slot_numel), self.device, "records")
        _check(self.lib, self.lib.lram_window_load_slots(self._h, _i32_array(slots), len(slots), _ptr(records),
                                                         _stream_ptr(self.device)))

    def _live_rows(self, buf: torch.Tensor) -> torch.Tensor:
        return buf if self._live == self.batch else buf[:self._live]

    def _need_all_live(self, what: str):
        if self._context_rows == "all" and self._live != self.batch:
            raise LramError(f"{what}: {self.batch - self._live} of {self.batch} env slots are parked (set_live): stored "
                            f"contexts and encoder calls need every slot live -- call set_live(batch) first")

    # -- state of individual env slots: fork / snapshot / restore ---------------------------------
    @property
    def slot_state_numel(self) -> int:
        """Floats in one env slot's state record (lram_slot_state_numel) = state_bytes_per_env() / 4."""
        return int(self.lib.lram_slot_state_numel(self._h))

    def copy_slots(self, src, dst):
        """Slot dst[i] becomes an exact copy of slot src[i] (lram_state_copy_slots): no other slot is touched, nothing is
        folded.  `src` may repeat (fork one context into many slots); slot-table entries and the sampling stream stay with the
        slot index, so forked slots draw independent continuations."""
        src, dst = _slot_list(src, "src"), _slot_list(dst, "dst")
        if len(src) != len(dst):
            raise ValueError(f"src and dst must have the same length, got {len(src)} and {len(dst)}")
        _check(self.lib, self.lib.lram_state_copy_slots(self._h, _i32_array(src), _i32_array(dst), len(src),
                                                        _stream_ptr(self.device)))

    def save_slots(self, slots, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Records of the listed slots, float32 [n, slot_state_numel] on the device (lram_state_save_slots): the portable
        per-env format (blocks in order, tensors in `which` order, reference layout).  Read-only for the engine."""
        slots = _slot_list(slots, "slots")
        n, numel = len(slots), self.slot_state_numel
        if out is None:
            out = torch.empty(n, numel, dtype=torch.float32, device=self.device)
        _chk_dev(out, torch.float32, (n, numel), self.device, "out")
        _check(self.lib, self.lib.lram_state_save_slots(self._h, _i32_array(slots), n, _ptr(out), _stream_ptr(self.device)))
        return out

    def load_slots(self, slots, records: torch.Tensor):
        """Write records [n, slot_state_numel] (as save_slots returns, from this or another engine of the same model) into the
        listed slots (lram_state_load_slots)."""
        slots = _slot_list(slots, "slots")
        records = records.to(device=self.device, dtype=torch.float32).contiguous()
        _chk_dev(records, torch.float32, (len(slots), self.slot_state_numel), self.device, "records")
        _check(self.lib, self.lib.lram_state_load_slots(self._h, _i32_array(slots), len(slots), _ptr(records),
                                                        _stream_ptr(self.device)))

    # -- launch-latency removal / measurement ----------------------------------------------------
    def set_graph_mode(self, enable: bool):
        _check(self.lib, self.lib.lram_set_graph_mode(self._h, int(enable)))

    def set_state_mode(self, mode, fold_period: int = 0):
        """mode: False / 0 / "eager" = materialised C (the reference's representation); True / 1 / "lazy" = read-once
        matrix memory with a pending-token window folded every `fold_period` steps; 2 / "auto" (default) = lazy where
        the state pass dominates (lram_set_state_mode)."""
        names = {"eager": 0, "materialised": 0, "lazy": 1, "auto": 2}
        m = names[mode] if isinstance(mode, str) else int(mode)
        _check(self.lib, self.lib.lram_set_state_mode(self._h, m, int(fold_period)))

    @property
    def state_mode(self) -> str:
        return "lazy" if self.lib.lram_get_state_mode(self._h) else "materialised"

    def lazy_peek(self, block: int, which: str) -> torch.Tensor:
        """Lazy representation looked at without folding: 'g' [B, NH] (scale of C_base since the last fold), 'm' [B, NH]
        (stabiliser state), 'pending' [B] (window tokens) -- lram_lazy_peek."""
        w = {"g": 0, "m": 1, "pending": 2}[which]
        shape = (self.batch,) if w == 2 else (self.batch, self.spec.n_heads)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.lram_lazy_peek(self._h, block, w, _ptr(out), _stream_ptr(self.device)))
        return out

    def set_micro_batches(self, n: int):
        """Env slices pipelined on separate HIP streams (0 = auto, 1 = off); results are independent of n."""
        _check(self.lib, self.lib.lram_set_micro_batches(self._h, int(n)))

    def set_compat_mode(self, mamba_repeat: int = 1, stale_state: bool = False):
        """Reference-trajectory modes of the Mamba agent (lram_set_compat_mode):
        `mamba_repeat` forwards per env-step with action dim i read from forward i
        (src/algos/decision_mamba.py:107-122), `stale_state`: a reset re-initialises layer 0 only (:20-25)."""
        _check(self.lib, self.lib.lram_set_compat_mode(self._h, int(mamba_repeat), int(bool(stale_state))))

    @property
    def compat_mode(self):
        r, st = ctypes.c_int32(1), ctypes.c_int32(0)
        self.lib.lram_get_compat_mode(self._h, ctypes.byref(r), ctypes.byref(st))
        return {"mamba_repeat": int(r.value), "stale_state": bool(st.value)}

    def set_sampling(self, temperature: Optional[float] = 1.0, top_k: int = 0, top_p: float = 0.0, seed: int = 0,
                     slot_base: int = 0):
        """Arm the sampling mode of the action head (lram_set_sampling): step / step_images / prefill then draw every
        (env, action dim) token from its logits row -- quantile filter `top_p` (a quantile of the logit values, as the
        reference's sample_from_logits, not nucleus sampling), the `top_k` largest, softmax(temperature * logits): the
        temperature MULTIPLIES -- with Philox uniforms keyed by `seed` and counted per (slot_base + slot, action dim, draw).
        Arming zeroes the draw count.  set_sampling(None) restores the argmax head."""
        if temperature is None:
            _check(self.lib, self.lib.lram_set_sampling(self._h, 0, 1.0, 0, 0.0, 0, 0))
            return
        _check(self.lib, self.lib.lram_set_sampling(self._h, 1, float(temperature), int(top_k), float(top_p),
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(slot_base) & 0xFFFFFFFFFFFFFFFF))

    @property
    def sampling(self) -> Optional[dict]:
        """None while the head takes the argmax; else the armed settings and `draws`, the action-producing calls since
        arming (reads a device counter: synchronises)."""
        on, k = ctypes.c_int32(0), ctypes.c_int32(0)
        t, p = ctypes.c_double(0.0), ctypes.c_double(0.0)
        seed, base, draws = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.lib, self.lib.lram_get_sampling(self._h, ctypes.byref(on), ctypes.byref(t), ctypes.byref(k), ctypes.byref(p),
                                                    ctypes.byref(seed), ctypes.byref(base), ctypes.byref(draws)))
        if not on.value:
            return None
        return {"temperature": t.value, "top_k": int(k.value), "top_p": p.value, "seed": int(seed.value),
                "slot_base": int(base.value), "draws": int(draws.value)}

    def set_sampling_slots(self, temperature=1.0, top_k=0, top_p=0.0, greedy=False):
        """Per-slot settings of the armed sampling head (lram_set_sampling_slots): each argument a scalar (every slot) or an
        array of length `batch`; `greedy` slots take the argmax of their row.  Seed, slot_base and the draw count stay those
        of set_sampling, which must be armed.  set_sampling_slots(None) clears the table (the settings of set_sampling apply
        again); set_sampling itself clears it too.  Synchronises and drops a captured graph: not a hot-path call."""
        if temperature is None:
            _check(self.lib, self.lib.lram_set_sampling_slots(self._h, None, None, None, None))
            return
        cols = slot_setting_arrays(self.batch, temperature, top_k, top_p, greedy)
        mode = (~cols["greedy"]).to(torch.uint8).contiguous()
        t, k, p = cols["temperature"].contiguous(), cols["top_k"].contiguous(), cols["top_p"].contiguous()
        _check(self.lib, self.lib.lram_set_sampling_slots(self._h, ctypes.c_void_p(mode.data_ptr()), ctypes.c_void_p(t.data_ptr()),
                                                          ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(p.data_ptr())))

    @property
    def sampling_slots(self) -> Optional[dict]:
        """The per-slot table in effect (lram_get_sampling_slots): {"temperature": float64 [B], "top_k": int32 [B],
        "top_p": float64 [B], "greedy": bool [B]} as CPU tensors, or None when none is set."""
        B = self.batch
        mode = torch.zeros(B, dtype=torch.uint8)
        t, p = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
        k = torch.zeros(B, dtype=torch.int32)
        on = ctypes.c_int32(0)
        _check(self.lib, self.lib.lram_get_sampling_slots(self._h, ctypes.c_void_p(mode.data_ptr()), ctypes.c_void_p(t.data_ptr()),
                                                          ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(p.data_ptr()),
                                                          ctypes.byref(on)))
        if not on.value:
            return None
        return {"temperature": t, "top_k": k, "top_p": p, "greedy": mode == 0}

    def profile_begin_sampled(self, every_n_steps: int):
        """Time every n-th step only (lram_profile_begin_sampled): 1/n of the event bookkeeping on the state-pass queue."""
        _check(self.lib, self.lib.lram_profile_begin_sampled(self._h, int(every_n_steps)))

    def profile_begin(self):
        _check(self.lib, self.lib.lram_profile_begin(self._h))

    def profile_end(self):
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        _check(self.lib, self.lib.lram_profile_end(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value


    def gemm_counts(self, reset: bool = False) -> dict:
        """Projection launches and fp32-equivalent FLOPs per kernel family of the dispatcher since the last reset
        (lram_gemm_counts): what the engine actually ran, whatever LRAM_GEMM says."""
        buf = (ctypes.c_double * 8)()
        _check(self.lib, self.lib.lram_gemm_counts(self._h, buf, 1 if reset else 0))
        names = ("f16x2", "bf16x3", "f32", "few_row_f32")
        return {n: {"launches": int(buf[i]), "flop": float(buf[4 + i])} for i, n in enumerate(names)}

    def slstm_counts(self, reset: bool = False) -> dict:
        """Launches of each form of the sLSTM recurrence since the last reset (lram_slstm_counts): "token" (one launch per
        token), "step" (one launch per pass) and "gemm" (pointwise launches behind a recurrent GEMM, one per token)."""
        buf = (ctypes.c_int64 * 3)()
        _check(self.lib, self.lib.lram_slstm_counts(self._h, buf, 1 if reset else 0))
        return {"token": int(buf[0]), "step": int(buf[1]), "gemm": int(buf[2])}

    def profile_end_split(self):
        """(state-pass ms, state-pass launches, fold ms, fold launches) -- lram_profile_end_split."""
        m, a = ctypes.c_double(0.0), ctypes.c_double(0.0)
        nm, na = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self.lib, self.lib.lram_profile_end_split(self._h, ctypes.byref(m), ctypes.byref(nm), ctypes.byref(a),
                                                         ctypes.byref(na)))
        return m.value, nm.value, a.value, na.value


def gemm_f32(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, accumulate: bool = False, kernel: str = "f32") -> torch.Tensor:
    """out[M,N] = a[M,K] @ w[N,K]^T (+ bias) (+ out) through the library's fp32-MFMA kernel (kernel="f32") or the
    bf16x3 kernel (kernel="bf16x3") the engine uses for its projections."""
    lib = load_library()
    fn = {"f32": lib.lram_gemm_f32, "bf16x3": lib.lram_gemm_bf16x3,
          "f16x2": lib.lram_gemm_f16x2, "f16x2p": lib.lram_gemm_f16x2_presplit, "f16x2p8": lib.lram_gemm_f16x2_presplit_8p,
          "skinny": lib.lram_gemm_skinny,
          "narrow": lib.lram_gemm_narrow, "narrow16": lib.lram_gemm_narrow_f16x2}[kernel]
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    _check(lib, fn(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(out), out.stride(0), _ptr(bias),
                                  int(accumulate), M, N, K, _stream_ptr(a.device)))
    return out


def sample_tokens(logits: torch.Tensor, uniform: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0,
                  rows: Optional[int] = None) -> torch.Tensor:
    """The sampling head's device code on caller data (lram_sample_tokens): logits float32 [R, n] (row stride free) or, with
    `rows` given, one row [n] shared by all `rows` draws; uniform float64 [R] in [0, 1) -> tokens int32 [R]."""
    lib = load_library()
    if rows is None:
        R, n = logits.shape
        ld = logits.stride(0)
        if logits.stride(1) != 1:
            raise ValueError("logits rows must be contiguous")
    else:
        R, n, ld = int(rows), logits.shape[-1], 0
        logits = logits.reshape(-1).contiguous()
    _chk_dev(uniform, torch.float64, (R,), logits.device, "uniform")
    if logits.dtype != torch.float32:
        raise ValueError("logits must be float32")
    out = torch.empty(R, dtype=torch.int32, device=logits.device)
    _check(lib, lib.lram_sample_tokens(_ptr(logits), R, int(n), int(ld), float(temperature), int(top_k), float(top_p),
                                       _ptr(uniform), _ptr(out), _stream_ptr(logits.device)))
    return out


def slot_setting_arrays(n: int, temperature=1.0, top_k=0, top_p=0.0, greedy=False) -> dict:
    """Scalars or arrays of length n -> {"temperature": float64 [n], "top_k": int32 [n], "top_p": float64 [n], "greedy": bool [n]}
    on the CPU (the host arrays of lram_set_sampling_slots / the rows of lram_sample_rows)."""
    out = {}
    for name, v, dt in (("temperature", temperature, torch.float64), ("top_k", top_k, torch.int32),
                        ("top_p", top_p, torch.float64), ("greedy", greedy, torch.bool)):
        t = torch.as_tensor(v).to("cpu").reshape(-1)
        if name == "top_k" and (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool):
            raise ValueError(f"top_k: expected integers, got {t.dtype}")
        if t.numel() == 1:
            t = t.expand(n)
        if t.numel() != n:
            raise ValueError(f"{name}: expected a scalar or {n} entries (one per slot / row), got {t.numel()}")
        out[name] = t.to(dt).contiguous()
    return out


def _mask_words_dev(mask, rows: int, n: int, device) -> torch.Tensor:
    """bool [rows, n] with no empty row -> its packed words on `device` (the dev_mask of the *_masked row entries)."""
    m = check_action_mask(mask, rows, n, 0)
    return pack_action_mask(m).to(device)


def sample_rows(logits: torch.Tensor, *, temperature=1.0, top_k=0, top_p=0.0, greedy=False,
                uniform: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, mask=None):
    """The sampling head's row code with per-row settings on caller data (lram_sample_rows): logits float32 [R, n]; the
    settings scalars or arrays of length R.  uniform float64 [R] -> the drawn tokens int32 [R]; tokens int32 [R] -> their
    log-probabilities float32 [R] under the row's filtered distribution.  Returns (drawn, logp), None where not asked for.
    mask bool [R, n]: row r works on its allowed sub-row (lram_sample_rows_masked; every row must allow something)."""
    lib = load_library()
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError("logits must be float32 [rows, n] with contiguous rows")
    if uniform is None and tokens is None:
        raise ValueError("sample_rows: give `uniform` (draw), `tokens` (score) or both")
    R, n = logits.shape
    dev = logits.device
    cols = slot_setting_arrays(R, temperature, top_k, top_p, greedy)
    t, k, p = cols["temperature"], cols["top_k"], cols["top_p"]
    if not bool((torch.isfinite(t) & (t > 0)).all()):
        raise ValueError("temperature must be finite and > 0")
    if not bool(((p >= 0) & (p <= 1)).all()):
        raise ValueError("top_p must be in [0, 1]")
    if not bool(((k >= 0) & (k <= n)).all()):
        raise ValueError("top_k must be in 0 .. n")
    mode = (~cols["greedy"]).to(torch.uint8).to(dev)
    t, k, p = t.to(dev), k.to(dev), p.to(dev)
    drawn = logp = None
    if uniform is not None:
        _chk_dev(uniform, torch.float64, (R,), dev, "uniform")
        drawn = torch.empty(R, dtype=torch.int32, device=dev)
    if tokens is not None:
        _chk_dev(tokens, torch.int32, (R,), dev, "tokens")
        logp = torch.empty(R, dtype=torch.float32, device=dev)
    if mask is not None:
        words = _mask_words_dev(mask, R, n, dev)
        _check(lib, lib.lram_sample_rows_masked(_ptr(logits), R, int(n), int(logits.stride(0)), _ptr(mode), _ptr(t), _ptr(k),
                                                _ptr(p), _ptr(uniform), _ptr(tokens), _ptr(drawn), _ptr(logp), _ptr(words),
                                                int(words.shape[1]), _stream_ptr(dev)))
        return drawn, logp
    _check(lib, lib.lram_sample_rows(_ptr(logits), R, int(n), int(logits.stride(0)), _ptr(mode), _ptr(t), _ptr(k), _ptr(p),
                                     _ptr(uniform), _ptr(tokens), _ptr(drawn), _ptr(logp), _stream_ptr(dev)))
    return drawn, logp


def score_tokens(logits: torch.Tensor, spec_or_dims, *, actions: Optional[torch.Tensor] = None,
                 tokens: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None, discrete: bool = False,
                 over: str = "vocab", temperature: float = 1.0, want=("actions", "tokens", "logp"), mask=None) -> ScoreResult:
    """The scoring head's device code on caller logits (lram_score_tokens): logits float32 [R, act_dim, n_vocab];
    `spec_or_dims` a ModelSpec or (n_discrete, action_channels); targets / valid / outputs per row as Engine.score.
    mask bool [R, n_vocab]: row r's allowed set (lram_score_tokens_masked); it must allow something inside the row's
    selectable range."""
    lib = load_library()
    if logits.dim() != 3 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("logits must be a contiguous float32 tensor [rows, act_dim, n_vocab]")
    R, A, V = logits.shape
    if isinstance(spec_or_dims, ModelSpec):
        n_discrete, channels = spec_or_dims.n_discrete, spec_or_dims.action_channels
    else:
        n_discrete, channels = (int(x) for x in spec_or_dims)
    dev = logits.device
    if actions is not None:
        _chk_dev(actions, torch.float32, (R, A), dev, "actions")
    if tokens is not None:
        _chk_dev(tokens, torch.int32, (R, A), dev, "tokens")
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        _chk_dev(valid, torch.uint8, (R,), dev, "valid")
    want = (want,) if isinstance(want, str) else tuple(want)
    res = ScoreResult(actions=torch.zeros(R, A, dtype=torch.float32, device=dev) if "actions" in want else None,
                      tokens=torch.zeros(R, A, dtype=torch.int32, device=dev) if "tokens" in want else None,
                      logp=torch.zeros(R, A, dtype=torch.float32, device=dev) if "logp" in want else None)
    if mask is not None:
        m = check_action_mask(mask, R, V, n_discrete, torch.full((R,), bool(discrete)))
        words = pack_action_mask(m).to(dev)
        _check(lib, lib.lram_score_tokens_masked(_ptr(logits), R, A, V, n_discrete, channels, -1.0, 1.0, int(bool(discrete)),
                                                 _ptr(actions), _ptr(tokens), _ptr(valid), _over_mode(over), float(temperature),
                                                 _ptr(res.actions), _ptr(res.tokens), _ptr(res.logp), _ptr(words),
                                                 int(words.shape[1]), _stream_ptr(dev)))
        return res
    _check(lib, lib.lram_score_tokens(_ptr(logits), R, A, V, n_discrete, channels, -1.0, 1.0, int(bool(discrete)),
                                      _ptr(actions), _ptr(tokens), _ptr(valid), _over_mode(over), float(temperature),
                                      _ptr(res.actions), _ptr(res.tokens), _ptr(res.logp), _stream_ptr(dev)))
    return res


def sample_uniforms(seed: int, slot_base: int, n_slots: int, act_dim: int, draw: int, device=None) -> torch.Tensor:
    """The uniforms an armed step uses at draw `draw` (lram_sample_uniforms): float64 [n_slots, act_dim]."""
    lib = load_library()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(int(n_slots), int(act_dim), dtype=torch.float64, device=device)
    _check(lib, lib.lram_sample_uniforms(int(seed) & 0xFFFFFFFFFFFFFFFF, int(slot_base) & 0xFFFFFFFFFFFFFFFF, int(n_slots),
                                         int(act_dim), int(draw) & 0xFFFFFFFFFFFFFFFF, _ptr(out), _stream_ptr(device)))
    return out


def pad_obs(native: torch.Tensor, state_dim: int, inv_index: Optional[torch.Tensor] = None,
            mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device-side observation front end (lram_pad_obs): scatter / zero-pad to `state_dim` (+ normalise)."""
    lib = load_library()
    B, n = native.shape
    if out is None:
        out = torch.empty(B, state_dim, dtype=torch.float32, device=native.device)
    _check(lib, lib.lram_pad_obs(_ptr(native), n, _ptr(inv_index), _ptr(mean), _ptr(std), _ptr(out), B, state_dim,
                                 _stream_ptr(native.device)))
    return out


def pad_obs_slots(native: torch.Tensor, state_dim: int, slot_row: torch.Tensor, inv_index: Optional[torch.Tensor] = None,
                  mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pad_obs with one index / mean / std row per slot (lram_pad_obs_slots): slot_row int32 [B] picks the row of the
    [n_rows, state_dim] tables (inv_index int32, mean / std float32) that slot b uses; inv_index None zero-pads."""
    lib = load_library()
    B, n = native.shape
    dev = native.device
    tables = [t for t in (inv_index, mean, std) if t is not None]
    n_rows = int(tables[0].reshape(-1, state_dim).shape[0]) if tables else 1
    _chk_dev(native, torch.float32, (B, n), dev, "native")
    _chk_dev(slot_row, torch.int32, (B,), dev, "slot_row")
    if inv_index is not None:
        _chk_dev(inv_index, torch.int32, (n_rows, state_dim), dev, "inv_index")
    for name, t in (("mean", mean), ("std", std)):
        if t is not None:
            _chk_dev(t, torch.float32, (n_rows, state_dim), dev, name)
    if out is None:
        out = torch.empty(B, state_dim, dtype=torch.float32, device=dev)
    _chk_dev(out, torch.float32, (B, state_dim), dev, "out")
    _check(lib, lib.lram_pad_obs_slots(_ptr(native), n, _ptr(slot_row), _ptr(inv_index), _ptr(mean), _ptr(std), n_rows,
                                       _ptr(out), B, state_dim, _stream_ptr(dev)))
    return out


def stream_copy(dst: torch.Tensor, src: torch.Tensor):
    lib = load_library()
    _check(lib, lib.lram_stream_copy(_ptr(dst), _ptr(src), src.numel(), _stream_ptr(src.device)))


def stream_read(buf: torch.Tensor, sink: torch.Tensor):
    """Read-only stream with the lazy read pass's access shape (lram_stream_read): the practical HBM ceiling for reading
    the recurrent state once.  `sink`: 1024 floats on the same device."""
    lib = load_library()
    _check(lib, lib.lram_stream_read(_ptr(buf), buf.numel(), _ptr(sink), _stream_ptr(buf.device)))


def stream_rmw(buf: torch.Tensor):
    """In-place x *= 1 stream with the cell kernel's access pattern (lram_stream_rmw): the practical HBM ceiling for
    reading the recurrent state once and writing it once."""
    lib = load_library()
    _check(lib, lib.lram_stream_rmw(_ptr(buf), buf.numel(), _stream_ptr(buf.device)))
