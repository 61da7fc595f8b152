"""ctypes face of librcn_hipx.so (include/rcn_hipx.h): the Track-X trainable convolution network.  No reference
counterpart (see the header); torch tensors are used only as HBM buffers."""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
LIBX_PATH = os.path.join(HERE, "librcn_hipx.so")
KIND = {"conv": 0, "pool": 1, "dense_relu": 2, "dense": 3, "conv_linear": 4, "bn_relu": 5, "bn_add_relu": 6, "global_avgpool": 7,
        "conv_linear_s2": 8, "bn_add_relu_down": 9, "conv1x1_linear": 10, "dwconv_linear": 11,
        "bn": 12, "bn_add": 13, "dwconv_linear_s2": 14}


class XLayer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("out", C.c_int32)]


class AugmentStruct(C.Structure):
    """rcn_hipx_augment"""
    _fields_ = [("pad", C.c_int32), ("hflip", C.c_int32), ("seed", C.c_uint64), ("epoch", C.c_uint64)]


@dataclass(frozen=True)
class Augment:
    """Random crop with zero padding (dy, dx in [-pad, pad]) and a horizontal flip with probability 1/2, drawn per sample from
    (seed, epoch, position in the epoch): include/rcn_hipx.h, rcn_hipx_augment.  A new `epoch` value gives new draws."""
    pad: int = 4
    hflip: bool = True
    seed: int = 0
    epoch: int = 0

    def struct(self) -> AugmentStruct:
        return AugmentStruct(int(self.pad), int(bool(self.hflip)), int(self.seed) & (2 ** 64 - 1), int(self.epoch) & (2 ** 64 - 1))


class MixStep(C.Structure):
    """rcn_hipx_mix_step: one training step's mixing record (24 bytes)"""
    _fields_ = [("blend", C.c_float), ("weight", C.c_float), ("y0", C.c_int32), ("y1", C.c_int32), ("x0", C.c_int32), ("x1", C.c_int32)]


EVAL_MAX_TOPK = 8                                        # RCN_HIPX_EVAL_MAX_TOPK


class EvalOut(C.Structure):
    """rcn_hipx_eval_out: the device buffers rcn_hipx_evaluate_metrics_dev fills (a NULL asks for nothing)"""
    _fields_ = [("loss_sum", C.c_void_p), ("correct", C.c_void_p), ("pred", C.c_void_p), ("n_topk", C.c_int32), ("topk", C.c_int32 * EVAL_MAX_TOPK),
                ("topk_correct", C.c_void_p), ("confusion", C.c_void_p), ("loss_each", C.c_void_p), ("rank", C.c_void_p), ("logits", C.c_void_p)]


STATE_MAX_LAYERS, STATE_SECTIONS = 32, 6               # RCN_HIPX_STATE_MAX_LAYERS, RCN_HIPX_STATE_SECTIONS
STATE_MAGIC, STATE_VERSION = 0x54535852, 1               # RCN_HIPX_STATE_MAGIC, RCN_HIPX_STATE_VERSION
SECTIONS = {"params": 1, "velocity": 2, "adam_m": 4, "adam_v": 8, "ema": 16, "accum": 32}      # RCN_HIPX_STATE_*: section s is bit s
STATE_HAS = {"adam_tick": 1, "dropout_tick": 2, "clip_state": 4, "recipe": 8}                 # RCN_HIPX_STATE_HAS_*: the descriptor's flags
STATE_SCALARS_BYTES = 256                                # the scalars block in front of a body: Adam tick at 0, dropout ordinal at 32, clip state at 40


class StateDesc(C.Structure):
    """rcn_hipx_state_desc: what describes a body and everything a snapshot carries outside it (include/rcn_hipx.h)"""
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint32),
                ("in_h", C.c_int32), ("in_w", C.c_int32), ("in_c", C.c_int32), ("n_layers", C.c_int32),
                ("layers", XLayer * STATE_MAX_LAYERS),
                ("classes", C.c_int32), ("precision", C.c_int32), ("tiling", C.c_int32), ("sections", C.c_int32),
                ("flags", C.c_int32), ("accum_pos", C.c_int32),
                ("n_log", C.c_int64),
                ("layer_off", C.c_int64 * STATE_MAX_LAYERS),
                ("section_off", C.c_int64 * STATE_SECTIONS),
                ("body_bytes", C.c_int64),
                ("optim", C.c_int32), ("sgd_nesterov", C.c_int32),
                ("sgd_momentum", C.c_float), ("sgd_weight_decay", C.c_float),
                ("adam_beta1", C.c_float), ("adam_beta2", C.c_float), ("adam_eps", C.c_float), ("adam_weight_decay", C.c_float),
                ("adam_decoupled", C.c_int32),
                ("loss_eps", C.c_float), ("ema_decay", C.c_float), ("clip_max_norm", C.c_float),
                ("accum_k", C.c_int32),
                ("dropout_p", C.c_float),
                ("dropout_seed", C.c_uint64)]

    def shape_and_layers(self):
        """(in_shape, layers) as ConvNet takes them; ("bn_add_relu", d), ("bn_add_relu_down", d) and ("bn_add", d) come back with their
        distance and ("conv_linear_s2", Cout) with its width (a depthwise layer of either stride: its resolved width C): the descriptor
        stores either as `out`"""
        names = {v: k for k, v in KIND.items()}
        layers = [(names[self.layers[i].kind],) if self.layers[i].kind in (KIND["pool"], KIND["bn_relu"], KIND["bn"], KIND["global_avgpool"]) else (names[self.layers[i].kind], int(self.layers[i].out))
                  for i in range(self.n_layers)]
        return (int(self.in_h), int(self.in_w), int(self.in_c)), layers

    def section(self, body: np.ndarray, name: str) -> np.ndarray:
        """section `name` (a key of SECTIONS) of a body's bytes as n_log float32 values, in the logical layout of get_params"""
        s = SECTIONS[name].bit_length() - 1
        if not self.sections >> s & 1:
            raise KeyError(f"the snapshot carries no {name!r} section")
        return np.frombuffer(body, dtype=np.float32, count=int(self.n_log), offset=int(self.section_off[s]))

    def scalars(self, body: np.ndarray) -> dict:
        """the scalars block of a body's bytes: {"adam_step", "dropout_state", "clip_count", "grad_norm", "clip_coef"}, None where the
        snapshot carries no such copy"""
        b = bytes(body[:STATE_SCALARS_BYTES])
        step, = struct.unpack_from("<q", b, 0)
        drop, = struct.unpack_from("<q", b, 32)
        count, norm, coef = struct.unpack_from("<Qff", b, 40)
        tick, dt, clip = (bool(self.flags & STATE_HAS[k]) for k in ("adam_tick", "dropout_tick", "clip_state"))
        return {"adam_step": step if tick else None, "dropout_state": drop if dt else None, "clip_count": count if clip else None,
                "grad_norm": norm if clip else None, "clip_coef": coef if clip else None}


# the same record as a NumPy structured dtype: an array of it, moved to the device as bytes, is train_epoch's `mix`
MIX_DTYPE = np.dtype([("blend", np.float32), ("weight", np.float32), ("y0", np.int32), ("y1", np.int32), ("x0", np.int32), ("x1", np.int32)])


def mix_plan(n_steps: int, H: int, W: int, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, switch_prob: float = 0.5, seed: int = 0) -> np.ndarray:
    """n_steps mixing records (MIX_DTYPE) for images of H x W, drawn with np.random.default_rng(seed); pure NumPy.  Per step: CutMix with
    probability switch_prob when both alphas are positive, else whichever is positive; lam ~ Beta(alpha, alpha).  mixup: blend = weight =
    float32(lam), empty box.  CutMix (the paper's box): cut = int(dim * sqrt(1 - lam)) per dimension around a centre uniform in the image,
    corners clipped to the image; blend = 1, weight = float32(1 - area / (H W))."""
    n_steps, H, W = int(n_steps), int(H), int(W)
    mixup_alpha, cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
    if n_steps < 1:
        raise ValueError("mix_plan: n_steps >= 1")
    if mixup_alpha < 0 or cutmix_alpha < 0 or (mixup_alpha == 0 and cutmix_alpha == 0):
        raise ValueError("mix_plan: alphas >= 0, at least one of them positive")
    rng = np.random.default_rng(seed)
    out = np.zeros(n_steps, dtype=MIX_DTYPE)
    for i in range(n_steps):
        cut = rng.random() < switch_prob if (mixup_alpha > 0 and cutmix_alpha > 0) else cutmix_alpha > 0
        lam = float(rng.beta(cutmix_alpha, cutmix_alpha) if cut else rng.beta(mixup_alpha, mixup_alpha))
        if not cut:
            out[i] = (lam, lam, 0, 0, 0, 0)
            continue
        ch, cw = int(H * np.sqrt(1.0 - lam)), int(W * np.sqrt(1.0 - lam))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        y0, y1 = int(np.clip(cy - ch // 2, 0, H)), int(np.clip(cy + ch // 2, 0, H))
        x0, x1 = int(np.clip(cx - cw // 2, 0, W)), int(np.clip(cx + cw // 2, 0, W))
        out[i] = (1.0, np.float32(1.0 - (y1 - y0) * (x1 - x0) / (H * W)), y0, y1, x0, x1)
    return out


def _aug_ref(augment: Optional[Augment]):
    """(ctypes struct kept alive by the caller, pointer or None)"""
    if augment is None:
        return None, None
    a = augment.struct()
    return a, C.byref(a)


_vp, _i = C.c_void_p, C.c_int
SIGNATURES = {
    "rcn_hipx_create": (_i, [_i, _i, _i, _i, C.POINTER(XLayer), _i, _i, _vp, C.POINTER(_vp)]),
    "rcn_hipx_destroy": (None, [_vp]),
    "rcn_hipx_last_error": (C.c_char_p, [_vp]),
    "rcn_hipx_synchronize": (_i, [_vp]),
    "rcn_hipx_param_count": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rcn_hipx_classes": (_i, [_vp]),
    "rcn_hipx_set_params": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_get_params": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_init_params": (_i, [_vp, C.c_uint64]),
    "rcn_hipx_forward_dev": (_i, [_vp, _vp, _i, _vp]),
    "rcn_hipx_train_step_dev": (_i, [_vp, _vp, _vp, _i, C.c_float, _vp]),
    "rcn_hipx_gradients_dev": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "rcn_hipx_apply_dev": (_i, [_vp, _vp, C.c_float]),
    "rcn_hipx_unpad_host": (_i, [_vp, _vp, C.POINTER(C.c_float)]),
    "rcn_hipx_set_precision": (_i, [_vp, _i]),
    "rcn_hipx_set_tiling": (_i, [_vp, _i]),
    "rcn_hipx_set_overlap": (_i, [_vp, _i]),
    "rcn_hipx_gradients_begin_dev": (_i, [_vp, _vp, _vp, _i, _vp, _vp, C.c_int64, C.POINTER(C.c_int)]),
    "rcn_hipx_gradients_bucket_dev": (_i, [_vp, _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rcn_hipx_plan_buckets": (_i, [_i, _i, _i, C.POINTER(XLayer), _i, _i, _i, _i, C.c_int64, C.c_char_p, _i]),
    "rcn_hipx_set_option": (_i, [_vp, C.c_char_p, _i]),
    "rcn_hipx_get_option": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int)]),
    "rcn_hipx_plan_net": (_i, [_vp, _i, C.c_char_p, _i]),
    "rcn_hipx_step_flops": (_i, [_vp, _i, C.POINTER(C.c_double)]),
    "rcn_hipx_plan": (_i, [_i, _i, _i, C.POINTER(XLayer), _i, _i, _i, _i, C.c_char_p, _i]),
    "rcn_hipx_set_sgd": (_i, [_vp, C.c_float, C.c_float, _i]),
    "rcn_hipx_get_sgd": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "rcn_hipx_get_velocity": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_set_velocity": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_reset_velocity": (_i, [_vp]),
    "rcn_hipx_apply_sgd_dev": (_i, [_vp, _vp, C.c_float, C.c_float]),
    "rcn_hipx_set_adam": (_i, [_vp, C.c_float, C.c_float, C.c_float, C.c_float, _i]),
    "rcn_hipx_get_adam": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rcn_hipx_get_adam_state": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "rcn_hipx_set_adam_state": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64]),
    "rcn_hipx_reset_adam": (_i, [_vp]),
    "rcn_hipx_train_epoch_dev": (_i, [_vp, _vp, _i, C.c_float, C.c_float, _vp, C.c_int64, _vp, _i, C.c_int64, C.c_int64, C.c_float, _vp]),
    "rcn_hipx_train_epoch_ex_dev": (_i, [_vp, _vp, _i, C.c_float, C.c_float, _vp, C.c_int64, _vp, _i, C.c_int64, C.c_int64, C.c_float, _vp, C.POINTER(AugmentStruct), _vp]),
    "rcn_hipx_gather_batch_dev": (_i, [_vp, _vp, _i, C.c_float, C.c_float, _vp, C.c_int64, _vp, C.c_int64, _i, C.POINTER(AugmentStruct), C.c_uint64, _vp, _vp]),
    "rcn_hipx_augment_draw": (_i, [C.POINTER(AugmentStruct), C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rcn_hipx_plan_epoch_net": (_i, [_vp, _i, _i, _i, C.POINTER(AugmentStruct), C.c_char_p, _i]),
    "rcn_hipx_set_loss": (_i, [_vp, C.c_float]),
    "rcn_hipx_get_loss": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_train_step_pair_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _i, C.c_float, _vp]),
    "rcn_hipx_gather_mix_dev": (_i, [_vp, _vp, _i, C.c_float, C.c_float, _vp, C.c_int64, _vp, C.c_int64, _i, C.POINTER(AugmentStruct), C.c_uint64, _vp, _vp, _vp, _vp]),
    "rcn_hipx_train_epoch_mix_dev": (_i, [_vp, _vp, _i, C.c_float, C.c_float, _vp, C.c_int64, _vp, _i, C.c_int64, C.c_int64, C.c_float, _vp, C.POINTER(AugmentStruct), _vp, _vp]),
    "rcn_hipx_plan_epoch_mix_net": (_i, [_vp, _i, _i, _i, C.POINTER(AugmentStruct), _i, C.c_char_p, _i]),
    "rcn_hipx_evaluate_dev": (_i, [_vp, _vp, _i, C.c_float, C.c_float, _vp, C.c_int64, _vp, _vp, _vp]),
    "rcn_hipx_graphs_instantiated": (_i, [_vp, C.POINTER(C.c_int64)]),
    "rcn_hipx_plan_eval": (_i, [_i, _i, _i, C.POINTER(XLayer), _i, _i, _i, _i, C.c_char_p, _i]),
    "rcn_hipx_plan_eval_net": (_i, [_vp, _i, C.c_char_p, _i]),
    "rcn_hipx_set_ema": (_i, [_vp, C.c_float]),
    "rcn_hipx_get_ema": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_get_ema_params": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_set_ema_params": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_reset_ema": (_i, [_vp]),
    "rcn_hipx_evaluate_ex_dev": (_i, [_vp, _vp, _i, C.c_float, C.c_float, _vp, C.c_int64, _i, _vp, _vp, _vp]),
    "rcn_hipx_set_clip": (_i, [_vp, C.c_float]),
    "rcn_hipx_get_clip": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_get_grad_norm": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "rcn_hipx_set_grad_norm_log": (_i, [_vp, _vp, C.c_int64]),
    "rcn_hipx_get_grad_norm_count": (_i, [_vp, C.POINTER(C.c_int64)]),
    "rcn_hipx_grad_norm_dev": (_i, [_vp, _vp, C.c_int64, C.c_float, _vp]),
    "rcn_hipx_set_accumulate": (_i, [_vp, _i]),
    "rcn_hipx_get_accumulate": (_i, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rcn_hipx_reset_accumulation": (_i, [_vp]),
    "rcn_hipx_get_accumulated": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_plan_micro_net": (_i, [_vp, _i, _i, C.c_char_p, _i]),
    "rcn_hipx_set_dropout": (_i, [_vp, C.c_float, C.c_uint64]),
    "rcn_hipx_get_dropout": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "rcn_hipx_get_dropout_state": (_i, [_vp, C.POINTER(C.c_int64)]),
    "rcn_hipx_set_dropout_state": (_i, [_vp, C.c_int64]),
    "rcn_hipx_dropout_draw": (_i, [C.c_float, C.c_uint64, C.c_uint64, _i, C.c_uint64, C.POINTER(C.c_int)]),
    "rcn_hipx_dropout_apply_dev": (_i, [_vp, _i, C.c_int64, _vp, _i]),
    "rcn_hipx_state_desc_size": (_i, []),
    "rcn_hipx_state_layout": (_i, [_i, _i, _i, C.POINTER(XLayer), _i, _i, C.POINTER(StateDesc)]),
    "rcn_hipx_snapshot_dev": (_i, [_vp, _i, _vp, C.c_int64, C.POINTER(StateDesc)]),
    "rcn_hipx_restore_dev": (_i, [_vp, C.POINTER(StateDesc), _vp, C.c_int64]),
    "rcn_hipx_set_accumulated": (_i, [_vp, C.POINTER(C.c_float), _i]),
    "rcn_hipx_evaluate_metrics_dev": (_i, [_vp, _vp, _i, C.c_float, C.c_float, _vp, C.c_int64, _i, C.POINTER(EvalOut)]),
    "rcn_hipx_label_rank": (_i, [C.POINTER(C.c_float), _i, _i, C.POINTER(C.c_int)]),
    "rcn_hipx_plan_eval_metrics_net": (_i, [_vp, _i, _i, _i, _i, _i, C.c_char_p, _i]),
    "rcn_hipx_last_logits_dev": (_i, [_vp, _i, _vp]),
    "rcn_hipx_set_bn": (_i, [_vp, C.c_float, C.c_float]),
    "rcn_hipx_get_bn": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "rcn_hipx_bn_stats_count": (_i, [_vp, C.POINTER(C.c_int64)]),
    "rcn_hipx_get_bn_stats": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_set_bn_stats": (_i, [_vp, C.POINTER(C.c_float)]),
    "rcn_hipx_reset_bn_stats": (_i, [_vp]),
    "rcn_hipx_bn_partials": (_i, [C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}
_libx = None


def load():
    global _libx
    if _libx is None:
        if not os.path.exists(LIBX_PATH):
            raise ImportError(f"{LIBX_PATH} not found: build it with `python -m mercer_research_amd.build`; there is no CPU fallback")
        _lib.preload_hip_runtime()
        lib = C.CDLL(LIBX_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _libx = lib
    return _libx


class ConvNetError(RuntimeError):
    pass


DEFAULT_BUCKET_BYTES = 1 << 20      # gradient buckets of the data-parallel step: at least 1 MiB each (a ring all-reduce below that is latency)


PRECISIONS = {"fp32": 0, "bf16": 1, "bf16_stored": 2}
TILINGS = {"gemm": 0, "auto": 1, "lds": 2}      # RCN_HIPX_TILING_*
WEIGHTS = {"live": 0, "ema": 1}     # RCN_HIPX_WEIGHTS_*: which parameters an evaluation scores
MICRO_KINDS = {"first": 0, "middle": 1, "last": 2}      # rcn_hipx_plan_micro_net's kinds of micro-step


def _layer_array(layers: Sequence[tuple]):
    """a net's description as the rcn_hipx_layer array the library takes"""
    arr = (XLayer * len(layers))()
    for i, l in enumerate(layers):
        arr[i].kind, arr[i].out = KIND[l[0]], int(l[1]) if len(l) > 1 else 0
    return arr


def _ptr(t):
    """a tensor's device pointer (None: NULL)"""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _plan_text(name: str, fn, *args) -> str:
    """The text a plan entry `fn` writes for `args` (its buffer and capacity come last); its refusal as a ConvNetError under `name`."""
    buf = C.create_string_buffer(1 << 16)
    st = fn(*args, buf, len(buf))
    if st != 0:
        raise ConvNetError(f"{name}: {st}: {buf.value.decode()}")
    return buf.value.decode()


def plan(in_shape: Tuple[int, int, int], layers: Sequence[tuple], batch: int, precision: str = "fp32", tiling: str = "auto", buckets: Optional[int] = None) -> str:
    """Which kernels a training step of this net would launch, one line per launch (rcn_hipx_plan): the library's own dispatch code run
    with its launches replaced by notes.  Needs no GPU.  buckets = N: the bucketed GRADIENT step of a data-parallel rank instead
    (rcn_hipx_plan_buckets, buckets of at least N bytes): per bucket its launches and the slice of the flat gradient that becomes final."""
    lib = load()
    args = (in_shape[0], in_shape[1], in_shape[2], _layer_array(layers), len(layers), batch, PRECISIONS[precision], TILINGS[tiling])
    if buckets is not None:
        return _plan_text("rcn_hipx_plan_buckets", lib.rcn_hipx_plan_buckets, *args, int(buckets))
    return _plan_text("rcn_hipx_plan", lib.rcn_hipx_plan, *args)


def plan_eval(in_shape: Tuple[int, int, int], layers: Sequence[tuple], batch: int, precision: str = "fp32", tiling: str = "auto") -> str:
    """Which kernels ONE evaluation chunk of `batch` rows would launch (rcn_hipx_plan_eval): the forward launches of `plan` and the
    evaluation kernel, one line per launch.  Needs no GPU."""
    return _plan_text("rcn_hipx_plan_eval", load().rcn_hipx_plan_eval, in_shape[0], in_shape[1], in_shape[2], _layer_array(layers), len(layers), batch,
                      PRECISIONS[precision], TILINGS[tiling])


def bn_partials(rows: int) -> Tuple[int, int]:
    """(parts, capacity) of rcn_hipx_bn_partials: the partial sums per channel of a map of `rows` rows, and what a layer whose largest map
    has `rows` rows makes room for.  Needs no GPU."""
    parts, cap = C.c_int(), C.c_int()
    if load().rcn_hipx_bn_partials(int(rows), C.byref(parts), C.byref(cap)) != 0:
        raise ConvNetError("rcn_hipx_bn_partials: rows must be at least 1")
    return int(parts.value), int(cap.value)


def label_rank(row, label: int) -> int:
    """How many classes BEAT `label` on the logits `row` (rcn_hipx_label_rank, the function k_eval_metrics runs, on the host): class c beats y
    when row[c] > row[y], or row[c] == row[y] and c < y.  0 .. classes - 1; -1 for a label outside [0, classes).  Needs no GPU."""
    r = np.ascontiguousarray(row, dtype=np.float32).reshape(-1)
    out = C.c_int()
    if load().rcn_hipx_label_rank(_fptr(r), int(r.size), int(label), C.byref(out)) != 0:
        raise ValueError("label_rank: a row of at least one logit")
    return int(out.value)


@dataclass
class EvalReport:
    """What ConvNet.evaluate_metrics found over a resident set, on the host.  loss: the mean loss; correct: rows whose arg-max is the label;
    topk: {k: rows whose label is among the k best}; confusion: int64 [classes, classes], row = label, column = prediction (None: not asked
    for); loss_each, rank, logits, pred: one entry per row, or None."""
    n: int
    loss: float
    correct: int
    topk: dict
    confusion: Optional[np.ndarray] = None
    loss_each: Optional[np.ndarray] = None
    rank: Optional[np.ndarray] = None
    logits: Optional[np.ndarray] = None
    pred: Optional[np.ndarray] = None

    def _confusion(self) -> np.ndarray:
        if self.confusion is None:
            raise ValueError("this report carries no confusion matrix (evaluate_metrics(confusion=True))")
        return self.confusion.astype(np.float64)

    def accuracy(self) -> float:
        """rows on the diagonal over rows in the matrix (a row whose label is out of range is in neither); NaN for an empty matrix"""
        m = self._confusion()
        return float(np.trace(m) / m.sum()) if m.sum() > 0 else float("nan")

    def recall(self) -> np.ndarray:
        """per class: rows of the class predicted as it, over rows of the class; NaN for a class without rows"""
        m = self._confusion()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(m) / m.sum(axis=1)

    def precision(self) -> np.ndarray:
        """per class: rows of the class predicted as it, over rows predicted as it; NaN for a class that is never predicted"""
        m = self._confusion()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(m) / m.sum(axis=0)


def state_layout(in_shape: Tuple[int, int, int], layers: Sequence[tuple], sections: Sequence[str] = ("params",)) -> StateDesc:
    """The descriptor of a body with these sections (keys of SECTIONS) for a net of this description (rcn_hipx_state_layout): shape, layer
    offsets, section offsets and body_bytes; the recipe at its defaults.  Needs no GPU."""
    d = StateDesc()
    mask = 0
    for name in sections:
        mask |= SECTIONS[name]
    st = load().rcn_hipx_state_layout(in_shape[0], in_shape[1], in_shape[2], _layer_array(layers), len(layers), mask, C.byref(d))
    if st != 0:
        raise ConvNetError(f"rcn_hipx_state_layout: {st}")
    return d


# ---- the state file: [8: magic][u32: descriptor bytes][u64: body bytes][u64: extra bytes][descriptor][body][extra][u32: CRC-32 of all before]
STATE_FILE_MAGIC = b"RCNXSTA1"
_STATE_HEAD = struct.Struct("<8sIQQ")


def write_state_file(desc: StateDesc, body, extra: Optional[bytes] = None) -> bytes:
    """One state file as bytes: the descriptor, the body (desc.body_bytes bytes: a bytes-like object or a uint8 array) and the caller's
    `extra` blob (its loop state: epoch, next batch, permutation seed), closed by a CRC-32 (zlib) of everything before it.  Needs no GPU."""
    body = bytes(memoryview(np.ascontiguousarray(body)).cast("B")) if isinstance(body, np.ndarray) else bytes(body)
    extra = b"" if extra is None else bytes(extra)
    if len(body) != int(desc.body_bytes):
        raise ConvNetError(f"write_state_file: the descriptor describes a body of {int(desc.body_bytes)} bytes, not {len(body)}")
    out = _STATE_HEAD.pack(STATE_FILE_MAGIC, C.sizeof(StateDesc), len(body), len(extra)) + bytes(desc) + body + extra
    return out + struct.pack("<I", zlib.crc32(out) & 0xffffffff)


def read_state_file(data: bytes) -> Tuple[StateDesc, np.ndarray, Optional[bytes]]:
    """(descriptor, body as a uint8 array, extra or None) of write_state_file's bytes.  A short file, a wrong magic, sizes that do not add up
    or a wrong CRC raise ConvNetError: nothing of such a file reaches the library.  Needs no GPU."""
    data = bytes(data)
    if len(data) < _STATE_HEAD.size + 4:
        raise ConvNetError("state file: truncated (shorter than its header)")
    magic, dsize, nbody, nextra = _STATE_HEAD.unpack_from(data, 0)
    if magic != STATE_FILE_MAGIC:
        raise ConvNetError("state file: wrong magic (not a Track X state file of this version)")
    if dsize != C.sizeof(StateDesc):
        raise ConvNetError(f"state file: a descriptor of {dsize} bytes; this library's has {C.sizeof(StateDesc)}")
    if len(data) != _STATE_HEAD.size + dsize + nbody + nextra + 4:
        raise ConvNetError("state file: truncated, or its sizes do not add up")
    crc, = struct.unpack_from("<I", data, len(data) - 4)
    if crc != zlib.crc32(data[:-4]) & 0xffffffff:
        raise ConvNetError("state file: CRC mismatch (the file is damaged)")
    at = _STATE_HEAD.size
    desc = StateDesc.from_buffer_copy(data, at)
    at += dsize
    if nbody != int(desc.body_bytes):
        raise ConvNetError("state file: the body's size is not the descriptor's")
    body = np.frombuffer(data, dtype=np.uint8, count=nbody, offset=at).copy()
    at += nbody
    return desc, body, (data[at:at + nextra] if nextra else None)


class Snapshot:
    """The state of a ConvNet at one point of its stream (ConvNet.snapshot): the device body, its descriptor and an event recorded on the
    net's stream behind the pack launch.  The body is valid once that event has happened; to_bytes and save wait for it alone."""

    def __init__(self, net: "ConvNet", desc: StateDesc, body, event):
        self.net, self.desc, self.body, self.event = net, desc, body, event
        self._host = None

    def body_bytes(self) -> np.ndarray:
        """The body as a uint8 host array: waits for the snapshot's event only -- not for work enqueued on the net's stream later -- and
        copies on a side stream of its own."""
        if self._host is None:
            t = self.net.torch
            side = self.net._state_side_stream()
            side.wait_event(self.event)
            with t.cuda.stream(side):
                host = t.empty(self.body.numel(), dtype=t.uint8, pin_memory=True)
                host.copy_(self.body, non_blocking=True)
            self.body.record_stream(side)
            side.synchronize()
            self._host = host.numpy().copy()
        return self._host

    def to_bytes(self, extra: Optional[bytes] = None) -> bytes:
        return write_state_file(self.desc, self.body_bytes(), extra)

    def save(self, path, extra: Optional[bytes] = None):
        data = self.to_bytes(extra)
        with open(path, "wb") as f:
            f.write(data)
        return len(data)


# the convolution kinds as step_hbm_floor_bytes sees them: (filter taps, stride, depthwise: C -> C with one input channel per filter)
_CONV_GEOMETRY = {"conv": (9, 1, False), "conv_linear": (9, 1, False), "conv_linear_s2": (9, 2, False), "conv1x1_linear": (1, 1, False), "dwconv_linear": (9, 1, True),
                  "dwconv_linear_s2": (9, 2, True)}
X_KIND = {"float32": 0, "uint8": 1}      # RCN_HIPX_X_F32 / RCN_HIPX_X_U8, by the set's torch dtype


def augment_draws(aug: Augment, q0: int, count: int) -> np.ndarray:
    """The (dy, dx, flip) draws of positions q0 .. q0 + count - 1 as an int array [count, 3], from rcn_hipx_augment_draw: the host side
    of the one function the gather kernel runs.  Needs no GPU."""
    lib = load()
    a = aug.struct()
    out = np.zeros((int(count), 3), dtype=np.int64)
    dy, dx, fl = C.c_int(), C.c_int(), C.c_int()
    for k in range(int(count)):
        if lib.rcn_hipx_augment_draw(C.byref(a), (int(q0) + k) & (2 ** 64 - 1), C.byref(dy), C.byref(dx), C.byref(fl)) != 0:
            raise ConvNetError(f"rcn_hipx_augment_draw refuses {aug}")
        out[k] = (dy.value, dx.value, fl.value)
    return out


def dropout_keep(p: float, seed: int, t: int, site: int, count: int) -> np.ndarray:
    """The keep / drop draws of elements 0 .. count - 1 of dropout site `site` in the training forward with ordinal t, as a bool array
    (True: kept), from rcn_hipx_dropout_draw: the host side of the one function k_dropout_fwd runs.  Needs no GPU."""
    lib = load()
    out = np.zeros(int(count), dtype=bool)
    k = C.c_int()
    for i in range(int(count)):
        if lib.rcn_hipx_dropout_draw(float(p), int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1), int(site), i, C.byref(k)) != 0:
            raise ConvNetError(f"rcn_hipx_dropout_draw refuses p = {p}, site = {site}")
        out[i] = bool(k.value)
    return out


def warmup_cosine(n_steps: int, peak: float, warmup_steps: int, floor: float = 0.0) -> np.ndarray:
    """A learning-rate schedule of n_steps float32 values, computed in float64: linear from peak / warmup_steps to peak over the first
    warmup_steps steps, then floor + (peak - floor) * 0.5 * (1 + cos(pi * t)) with t running from 0 to 1 over the remaining steps."""
    n_steps, warmup_steps = int(n_steps), int(warmup_steps)
    if n_steps < 1 or not 0 <= warmup_steps <= n_steps:
        raise ValueError("warmup_cosine: n_steps >= 1 and 0 <= warmup_steps <= n_steps")
    lr = np.empty(n_steps, dtype=np.float64)
    lr[:warmup_steps] = float(peak) * np.arange(1, warmup_steps + 1, dtype=np.float64) / max(warmup_steps, 1)
    rest = n_steps - warmup_steps
    t = np.arange(rest, dtype=np.float64) / max(rest - 1, 1)
    lr[warmup_steps:] = float(floor) + (float(peak) - float(floor)) * 0.5 * (1.0 + np.cos(np.pi * t))
    return lr.astype(np.float32)


class ConvNet:
    """layers: sequence of ("conv", Cout) | ("pool",) | ("dense_relu", units) | ("dense", classes) | ("conv_linear", Cout) | ("bn_relu",) |
    ("bn_add_relu", d) | ("global_avgpool",): torch's Conv2d -> BatchNorm2d -> ReLU is ("conv_linear", Cout), ("bn_relu",).  ("bn_add_relu", d) is
    relu(BatchNorm2d(z) + s) with s the output of the layer d places in front of it (d >= 2): torchvision's BasicBlock with an identity
    shortcut is ("conv_linear", C), ("bn_relu",), ("conv_linear", C), ("bn_add_relu", 4) behind the layer that made the block's input.
    ("global_avgpool",) is AdaptiveAvgPool2d(1) -> flatten(1) behind the last map (a "conv", "bn_relu", "bn_add_relu" or "pool" layer): the
    dense layer behind it has K = C inputs at any input resolution, and only dense layers may follow.
    ("conv_linear_s2", Cout) is Conv2d(Cin, Cout, 3, stride=2, padding=1) on an even map of Cin % 32 == 0 channels, followed by a bn layer
    like "conv_linear".  ("bn_add_relu_down", d) is relu(BatchNorm2d(z) + s') with s' the parameter-free option-A shortcut of the output s
    (Cs <= C channels, twice this layer's height and width) of the layer d places in front:
    F.pad(s[:, :, ::2, ::2], (0, 0, 0, 0, lo, C - Cs - lo)), lo = (C - Cs) / 2.  The down block of the CIFAR ResNet behind a layer of C
    channels is ("conv_linear_s2", 2C), ("bn_relu",), ("conv_linear", 2C), ("bn_add_relu_down", 4).
    ("conv1x1_linear", Cout) is Conv2d(Cin, Cout, 1) on a map of Cin % 32 == 0 channels, followed by a bn layer like "conv_linear"; a
    bottleneck block behind a layer of C channels is ("conv1x1_linear", C/4), ("bn_relu",), ("conv_linear", C/4), ("bn_relu",),
    ("conv1x1_linear", C), ("bn_add_relu", 6); the option "pw" (set_option) chooses between the implicit GEMM (0, the default) and its streaming kernel (1).
    ("dwconv_linear",) is Conv2d(C, C, 3, padding=1, groups=C), the depthwise 3x3 convolution, on a map of C % 32 == 0 channels, followed by a
    bn layer like "conv_linear" (("dwconv_linear", C) says the same; any other width is refused); fp32 arithmetic in either precision mode.
    A separable layer is ("dwconv_linear",), ("bn_relu",), ("conv1x1_linear", C'), ("bn_relu",); a residual separable block behind a layer
    of C channels is ("dwconv_linear",), ("bn_relu",), ("conv1x1_linear", C), ("bn_add_relu", 4).
    ("dwconv_linear_s2",) is Conv2d(C, C, 3, stride=2, padding=1, groups=C) on an even map, under "dwconv_linear"'s rules otherwise.  ("bn",) is
    BatchNorm2d(C) with no activation and ("bn_add", d) is BatchNorm2d(z) + s with none, s as for "bn_add_relu": MobileNetV2's linear
    bottleneck.  Either may be a skip's source, and a convolution of any kind must follow directly (not "pool", "global_avgpool" or a dense
    layer).  An inverted residual block of expansion t behind a layer of C channels is ("conv1x1_linear", tC), ("bn_relu",), ("dwconv_linear",),
    ("bn_relu",), ("conv1x1_linear", C), ("bn_add", 6); one that changes the width or halves the map ends in ("dwconv_linear_s2",), ("bn_relu",),
    ("conv1x1_linear", C'), ("bn",)."""

    def __init__(self, in_shape: Tuple[int, int, int], layers: Sequence[tuple], max_batch: int, device: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("ConvNet needs a GPU; there is no CPU fallback")
        self.lib = load()
        self.torch = torch
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.in_shape, self.layers, self.max_batch = tuple(in_shape), [tuple(l) for l in layers], max_batch
        self.net = C.c_void_p()
        st = self.lib.rcn_hipx_create(device, in_shape[0], in_shape[1], in_shape[2], _layer_array(layers), len(layers), max_batch, C.c_void_p(self.stream.cuda_stream),
                                      C.byref(self.net))
        if st != 0:
            msg = self.lib.rcn_hipx_last_error(self.net).decode() if self.net.value else f"status {st}"
            if self.net.value:
                self.lib.rcn_hipx_destroy(self.net)
            self.net = C.c_void_p()
            raise ConvNetError(f"rcn_hipx_create: {st}: {msg}")
        a, b = C.c_int64(), C.c_int64()
        self.lib.rcn_hipx_param_count(self.net, C.byref(a), C.byref(b))
        self.n_logical, self.n_padded = int(a.value), int(b.value)
        self.classes = self.lib.rcn_hipx_classes(self.net)

    def _ck(self, st):
        if st != 0:
            raise ConvNetError(f"rcn_hipx status {st}: {self.lib.rcn_hipx_last_error(self.net).decode()}")

    def close(self):
        if getattr(self, "net", None) is not None and self.net.value:
            self.lib.rcn_hipx_destroy(self.net)
            self.net = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._ck(self.lib.rcn_hipx_synchronize(self.net))

    def set_precision(self, mode: str):
        """"fp32" (fp32 MFMA, default), "bf16" (bf16 MFMA operands, fp32 accumulate / storage / update) or "bf16_stored" (bf16 operands
        AND the convolutional stage's activations / gradients kept in HBM as bf16: include/rcn_hipx.h, RCN_HIPX_BF16_STORED)."""
        self._ck(self.lib.rcn_hipx_set_precision(self.net, PRECISIONS[mode]))

    def set_tiling(self, mode: str):
        """fp32 3x3 kernels: "gemm" (implicit GEMM only), "auto" (by shape, the default) or "lds" (LDS-tiled wherever they apply)."""
        self._ck(self.lib.rcn_hipx_set_tiling(self.net, TILINGS[mode]))

    def set_overlap(self, mode):
        """Backward pass: weight gradients on a second stream beside the input-gradient chain: 0 / False = no (default: measured no
        gain), 1 / True = every layer's, 2 = the dense layers' only."""
        self._ck(self.lib.rcn_hipx_set_overlap(self.net, int(mode)))

    def set_option(self, name: str, value: int):
        """A kernel-selection knob of THIS net (rcn_hipx_set_option; the environment only seeds the defaults at creation)."""
        self._ck(self.lib.rcn_hipx_set_option(self.net, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int()
        if self.lib.rcn_hipx_get_option(self.net, name.encode(), C.byref(v)) != 0:
            raise ConvNetError(f"unknown option {name!r}")
        return int(v.value)

    def plan_of_this_net(self, batch: int) -> str:
        """The launches a training step of THIS net would make, with its own precision, tiling and options (rcn_hipx_plan_net)."""
        return _plan_text("rcn_hipx_plan_net", self.lib.rcn_hipx_plan_net, self.net, int(batch))

    def _set_flat(self, fn, flat: np.ndarray):
        f = np.ascontiguousarray(flat, dtype=np.float32)
        assert f.size == self.n_logical
        self._ck(fn(self.net, _fptr(f)))

    def _get_flat(self, fn) -> np.ndarray:
        f = np.zeros(self.n_logical, dtype=np.float32)
        self._ck(fn(self.net, _fptr(f)))
        return f

    def set_params(self, flat: np.ndarray):
        self._set_flat(self.lib.rcn_hipx_set_params, flat)

    def get_params(self) -> np.ndarray:
        return self._get_flat(self.lib.rcn_hipx_get_params)

    def init_params(self, seed: int = 1):
        self._ck(self.lib.rcn_hipx_init_params(self.net, seed))

    def to_device(self, a: np.ndarray):
        with self.torch.cuda.stream(self.stream):
            return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def forward(self, x):
        out = self.torch.empty(x.shape[0], self.classes, dtype=self.torch.float32, device=self.device)
        self._ck(self.lib.rcn_hipx_forward_dev(self.net, _ptr(x), x.shape[0], _ptr(out)))
        return out

    def last_logits(self, B: int):
        """[B, classes]: the logits the LAST forward pass left -- after train_step or gradients, those of its TRAINING forward (batch
        statistics, dropout), which forward never runs (rcn_hipx_last_logits_dev)"""
        out = self.torch.empty(int(B), self.classes, dtype=self.torch.float32, device=self.device)
        self._ck(self.lib.rcn_hipx_last_logits_dev(self.net, int(B), _ptr(out)))
        return out

    def train_step(self, x, labels, lr: float, loss=None):
        self._ck(self.lib.rcn_hipx_train_step_dev(self.net, _ptr(x), _ptr(labels), x.shape[0], lr, _ptr(loss)))

    def train_step_pair(self, x, labels_a, labels_b, weight, lr: float, loss=None):
        """train_step on pair labels (rcn_hipx_train_step_pair_dev): sample s has the target w * onehot(labels_a[s]) + (1 - w) *
        onehot(labels_b[s]), smoothed by set_loss's label_smoothing.  weight: a one-element float32 device tensor holding w, read by the
        loss launch (None: w = 1)."""
        self._ck(self.lib.rcn_hipx_train_step_pair_dev(self.net, _ptr(x), _ptr(labels_a), _ptr(labels_b), _ptr(weight), x.shape[0], lr, _ptr(loss)))

    def _mix_records(self, mix, count: int):
        """the pointer of `count` rcn_hipx_mix_step records in a contiguous device tensor (any dtype: the bytes of a MIX_DTYPE array)"""
        if not self.torch.is_tensor(mix) or mix.device != self.device or not mix.is_contiguous() or mix.numel() * mix.element_size() < count * MIX_DTYPE.itemsize:
            raise ValueError(f"mix: a contiguous tensor on the net's device holding at least {count} records of {MIX_DTYPE.itemsize} bytes (MIX_DTYPE)")
        if mix.data_ptr() % 4:
            raise ValueError("mix: the records must be 4-byte aligned")
        return _ptr(mix)

    def mix_to_device(self, records: np.ndarray):
        """a MIX_DTYPE array (mix_plan's) as a device tensor of its bytes: train_epoch's and gather_mix's `mix`"""
        rec = np.ascontiguousarray(records, dtype=MIX_DTYPE).reshape(-1)
        return self.to_device(rec.view(np.uint8).reshape(rec.size, MIX_DTYPE.itemsize))

    def _resident_set(self, X, labels):
        """(x_kind, rows) of a device-resident set after checking its dtype, shape, device and contiguity (labels: int32, one per row)."""
        t = self.torch
        kind = X_KIND.get(str(X.dtype).replace("torch.", ""))
        if kind is None:
            raise ValueError(f"a resident set is torch.float32 or torch.uint8, not {X.dtype}")
        if tuple(X.shape[1:]) != self.in_shape or X.shape[0] < 1:
            raise ValueError(f"a resident set is [n, {self.in_shape[0]}, {self.in_shape[1]}, {self.in_shape[2]}] with n >= 1, not {tuple(X.shape)}")
        if X.device != self.device or not X.is_contiguous():
            raise ValueError("a resident set is a contiguous tensor on the net's device")
        if labels is not None:
            if labels.dtype != t.int32 or tuple(labels.shape) != (X.shape[0],) or labels.device != self.device or not labels.is_contiguous():
                raise ValueError("labels: a contiguous int32 tensor on the net's device, one per row of the set")
        return kind, int(X.shape[0])

    def train_epoch(self, X, labels, perm, B: int, lr, n_batches: Optional[int] = None, first_batch: int = 0, losses=None,
                    x_scale: float = 1.0 / 255.0, x_shift: float = 0.0, augment: Optional[Augment] = None, mix=None):
        """n_batches training steps over a device-resident set (rcn_hipx_train_epoch_dev): batch s is rows perm[s*B : (s+1)*B] (perm None:
        rows in order), gathered on the device into the net's own batch buffer, then the step of train_step -- bit-identical to it, and ONE
        captured graph per (B, lr) whatever X, perm, first_batch and losses are.  X: torch.float32 or torch.uint8 [n, H, W, C] (uint8 rows
        become fl(fl(u8 * x_scale) + x_shift); both are ignored for float32); perm: int32 device tensor with entries in [0, n) (checked here,
        once per call: one device reduction, which synchronises) or None; n_batches defaults to n // B - first_batch; losses (optional):
        float32 device tensor of at least n_batches elements, losses[i] = mean loss of the call's i-th step before its update.
        lr: a float, or a contiguous float32 device tensor of at least n_batches elements -- lr[i] is the rate of the call's i-th step
        (rcn_hipx_train_epoch_ex_dev: ONE graph per B whatever the schedule; checked finite here, once per call, which synchronises).
        augment: an Augment -- every batch is gathered through its random crop and flip, drawn from (seed, epoch, s*B + r).
        mix: a contiguous device tensor holding at least n_batches records of MIX_DTYPE (mix_plan's array through mix_to_device) -- the
        call's i-th step is mixed by record i (rcn_hipx_train_epoch_mix_dev: mixup / CutMix with the mirrored row of the same batch, ONE
        more graph whatever the records are).
        On an accumulating net (set_accumulate(k), k > 1) B is the micro-batch and lr, mix and losses are all per micro-batch: every k-th
        step applies an update, at ITS entry of lr (the other entries are ignored), so a schedule of U updates is np.repeat(schedule, k).
        Pick n_batches % k == 0, or the tail stays pending (get_accumulate) and the next call's first steps complete its cycle."""
        t = self.torch
        kind, n = self._resident_set(X, labels)
        if labels is None:
            raise ValueError("train_epoch needs labels")
        B, first_batch = int(B), int(first_batch)
        n_batches = (n // B - first_batch if B >= 1 else 0) if n_batches is None else int(n_batches)
        if perm is not None:
            if perm.dtype != t.int32 or perm.dim() != 1 or perm.device != self.device or not perm.is_contiguous():
                raise ValueError("perm: a contiguous one-dimensional int32 tensor on the net's device")
            if perm.numel() < (first_batch + n_batches) * B <= n:        # (batches beyond the set itself: the library's refusal below)
                raise ValueError(f"perm has {perm.numel()} entries; batches {first_batch} .. {first_batch + n_batches - 1} of {B} rows need {(first_batch + n_batches) * B}")
            if perm.numel():
                lo, hi = t.aminmax(perm)
                if int(lo) < 0 or int(hi) >= n:
                    raise ValueError(f"perm entries must lie in [0, {n}); found {int(lo)} .. {int(hi)}")
        if losses is not None:
            if losses.dtype != t.float32 or losses.device != self.device or not losses.is_contiguous() or losses.numel() < n_batches:
                raise ValueError("losses: a contiguous float32 tensor on the net's device with at least n_batches elements")
        lr_dev = None
        if t.is_tensor(lr):
            if lr.dtype != t.float32 or lr.dim() != 1 or lr.device != self.device or not lr.is_contiguous() or lr.numel() < n_batches:
                raise ValueError("lr: a float, or a contiguous one-dimensional float32 tensor on the net's device with at least n_batches elements")
            if n_batches > 0 and not bool(t.isfinite(lr[:n_batches]).all()):
                raise ValueError("lr: the schedule holds a value that is not finite")
            lr_dev, lr = _ptr(lr), 0.0
        recs = self._mix_records(mix, n_batches) if mix is not None else None
        keep, aug = _aug_ref(augment)
        # (rcn_hipx_train_epoch_dev and _ex_dev are this entry with NULLs)
        self._ck(self.lib.rcn_hipx_train_epoch_mix_dev(self.net, _ptr(X), kind, float(x_scale), float(x_shift), _ptr(labels), n, _ptr(perm), B, first_batch, n_batches, float(lr),
                                                       lr_dev, aug, recs, _ptr(losses)))

    def _index_row(self, idx, B: int):
        """gather_batch's and gather_mix's idx: None, or B row numbers"""
        if idx is not None and (idx.dtype != self.torch.int32 or idx.dim() != 1 or idx.device != self.device or not idx.is_contiguous() or idx.numel() < B):
            raise ValueError("idx: a contiguous one-dimensional int32 tensor on the net's device with at least B entries")

    def gather_batch(self, X, labels, idx, B: int, base: int = 0, augment: Optional[Augment] = None, q0: int = 0,
                     x_scale: float = 1.0 / 255.0, x_shift: float = 0.0):
        """One batch as train_epoch gathers it (rcn_hipx_gather_batch_dev): rows idx[0 : B] (idx None: rows base .. base + B - 1) of a
        resident set as a float32 [B, H, W, C] tensor, and their labels (None without labels), enqueued on the net's stream.  augment: row r
        draws with position q0 + r (train_epoch's batch s has q0 = s * B)."""
        t = self.torch
        kind, n = self._resident_set(X, labels)
        B = int(B)
        self._index_row(idx, B)
        with t.cuda.stream(self.stream):
            x = t.empty((max(B, 0),) + self.in_shape, dtype=t.float32, device=self.device)
            y = t.empty(max(B, 0), dtype=t.int32, device=self.device) if labels is not None else None
        keep, aug = _aug_ref(augment)
        self._ck(self.lib.rcn_hipx_gather_batch_dev(self.net, _ptr(X), kind, float(x_scale), float(x_shift), _ptr(labels), n, _ptr(idx), int(base), B, aug,
                                                    int(q0) & (2 ** 64 - 1), _ptr(x), _ptr(y)))
        return x, y

    def gather_mix(self, X, labels, idx, B: int, mix, base: int = 0, augment: Optional[Augment] = None, q0: int = 0,
                   x_scale: float = 1.0 / 255.0, x_shift: float = 0.0):
        """One batch as train_epoch(mix=...) gathers it (rcn_hipx_gather_mix_dev): gather_batch's rows, row r mixed with row B - 1 - r by the
        ONE record `mix` holds (a device tensor, as train_epoch's).  Returns (x, labels of the rows, labels of their partners); the two
        labels are None without labels."""
        t = self.torch
        kind, n = self._resident_set(X, labels)
        B = int(B)
        self._index_row(idx, B)
        rec = self._mix_records(mix, 1)
        with t.cuda.stream(self.stream):
            x = t.empty((max(B, 0),) + self.in_shape, dtype=t.float32, device=self.device)
            ya = t.empty(max(B, 0), dtype=t.int32, device=self.device) if labels is not None else None
            yb = t.empty(max(B, 0), dtype=t.int32, device=self.device) if labels is not None else None
        keep, aug = _aug_ref(augment)
        self._ck(self.lib.rcn_hipx_gather_mix_dev(self.net, _ptr(X), kind, float(x_scale), float(x_shift), _ptr(labels), n, _ptr(idx), int(base), B, aug,
                                                  int(q0) & (2 ** 64 - 1), rec, _ptr(x), _ptr(ya), _ptr(yb)))
        return x, ya, yb

    def plan_epoch_of_this_net(self, batch: int, x_dtype: str = "uint8", lr_from_device: bool = False, augment: Optional[Augment] = None, mix: bool = False) -> str:
        """What one step of train_epoch launches for THIS net (rcn_hipx_plan_epoch_net / _mix_net): the gather, the copy of a scheduled rate
        (and, mix: of the step's target weight), the graph's key, then plan_of_this_net's text.  x_dtype: "uint8" or "float32", the set's storage."""
        keep, aug = _aug_ref(augment)
        # (rcn_hipx_plan_epoch_net is this entry with mix = 0)
        return _plan_text("rcn_hipx_plan_epoch_net", self.lib.rcn_hipx_plan_epoch_mix_net, self.net, int(batch), X_KIND[x_dtype], int(bool(lr_from_device)), aug, int(bool(mix)))

    def evaluate_async(self, X, labels=None, x_scale: float = 1.0 / 255.0, x_shift: float = 0.0, want_pred: bool = True, weights: str = "live"):
        """Forward pass, loss and arg-max over ALL rows of a resident set (rcn_hipx_evaluate_ex_dev), enqueued on the net's stream: returns the
        device tensors (loss_sum: float64[1], correct: int64[1], pred: int32[n] or None), valid once the net's stream has got there
        (`synchronize`).  labels None: prediction only (loss_sum and correct stay zero).  weights: "live" (the parameters of the last step)
        or "ema" (set_ema's average of them; the live parameters are back in place when the call's work is done)."""
        t = self.torch
        if weights not in WEIGHTS:
            raise ValueError(f"weights must be one of {sorted(WEIGHTS)}, not {weights!r}")
        kind, n = self._resident_set(X, labels)
        with t.cuda.stream(self.stream):
            loss_sum = t.zeros(1, dtype=t.float64, device=self.device)
            correct = t.zeros(1, dtype=t.int64, device=self.device)
            pred = t.empty(n, dtype=t.int32, device=self.device) if (want_pred or labels is None) else None
        self._ck(self.lib.rcn_hipx_evaluate_ex_dev(self.net, _ptr(X), kind, float(x_scale), float(x_shift), _ptr(labels), n, WEIGHTS[weights], _ptr(loss_sum), _ptr(correct),
                                                   _ptr(pred)))
        return loss_sum, correct, pred

    def evaluate(self, X, labels, x_scale: float = 1.0 / 255.0, x_shift: float = 0.0, weights: str = "live") -> Tuple[float, int]:
        """(mean loss, number of rows whose arg-max equals the label) over all rows of a resident set; synchronises."""
        if labels is None:
            raise ValueError("evaluate needs labels (predict: arg-max only)")
        loss_sum, correct, _ = self.evaluate_async(X, labels, x_scale, x_shift, want_pred=False, weights=weights)
        self.synchronize()
        return float(loss_sum.item()) / X.shape[0], int(correct.item())

    def predict(self, X, x_scale: float = 1.0 / 255.0, x_shift: float = 0.0, weights: str = "live"):
        """The arg-max class of every row (the FIRST maximum, as torch.argmax): an int32 device tensor, valid on the net's stream."""
        return self.evaluate_async(X, None, x_scale, x_shift, weights=weights)[2]

    def graphs_instantiated(self) -> int:
        """hipGraphs this net has instantiated since it was created (an epoch with a (B, lr) seen before adds none)."""
        c = C.c_int64()
        self._ck(self.lib.rcn_hipx_graphs_instantiated(self.net, C.byref(c)))
        return int(c.value)

    def plan_eval_of_this_net(self, batch: int) -> str:
        """The launches one evaluation chunk of THIS net would make, with its own precision, tiling and options (rcn_hipx_plan_eval_net)."""
        return _plan_text("rcn_hipx_plan_eval_net", self.lib.rcn_hipx_plan_eval_net, self.net, int(batch))

    def _topk_list(self, topk) -> Tuple[int, ...]:
        """`topk` as the strictly increasing tuple of 1 <= k <= classes the library takes; anything else is a ValueError (nothing is clamped)"""
        ks = tuple(int(k) for k in topk)
        if len(ks) > EVAL_MAX_TOPK:
            raise ValueError(f"topk: at most {EVAL_MAX_TOPK} values, not {len(ks)}")
        if any(k < 1 or k > self.classes for k in ks):
            raise ValueError(f"topk: every k must lie in 1 .. {self.classes} (the net's classes), not {ks}")
        if any(b <= a for a, b in zip(ks, ks[1:])):
            raise ValueError(f"topk must be strictly increasing, not {ks}")
        return ks

    def evaluate_metrics_async(self, X, labels=None, topk=(1, 5), confusion: bool = True, per_row: bool = False, logits: bool = False,
                               x_scale: float = 1.0 / 255.0, x_shift: float = 0.0, weights: str = "live") -> dict:
        """evaluate_async with more to tell (rcn_hipx_evaluate_metrics_dev), enqueued on the net's stream: a dict of device tensors, valid once
        the net's stream has got there -- loss_sum float64[1], correct int64[1] and pred int32[n] as evaluate_async gives them, bit for bit;
        topk (the ks) and topk_correct int64[len(topk)] (rows whose label is among the k best; None for an empty topk); confusion int64
        [classes, classes] (row = label, column = prediction) or None; per_row: loss_each float32[n] and rank int32[n] (classes that beat
        the label, -1 for a label out of range), else None; logits: float32[n, classes], forward()'s bits, else None.  topk: strictly
        increasing, 1 <= k <= classes (the default asks for top-5: a ValueError on a net with fewer classes).  labels None: pred and
        logits only (topk=(), confusion=False, per_row=False)."""
        t = self.torch
        if weights not in WEIGHTS:
            raise ValueError(f"weights must be one of {sorted(WEIGHTS)}, not {weights!r}")
        ks = self._topk_list(topk)
        if labels is None and (ks or confusion or per_row):
            raise ValueError("without labels there are only pred and logits: topk=(), confusion=False, per_row=False")
        kind, n = self._resident_set(X, labels)
        with t.cuda.stream(self.stream):
            new = lambda shape, dtype: t.empty(shape, dtype=dtype, device=self.device)
            out = dict(loss_sum=t.zeros(1, dtype=t.float64, device=self.device), correct=t.zeros(1, dtype=t.int64, device=self.device), pred=new(n, t.int32), topk=ks,
                       topk_correct=new(len(ks), t.int64) if ks else None, confusion=new((self.classes, self.classes), t.int64) if confusion else None,
                       loss_each=new(n, t.float32) if per_row else None, rank=new(n, t.int32) if per_row else None,
                       logits=new((n, self.classes), t.float32) if logits else None)
        addr = lambda name: out[name].data_ptr() if out[name] is not None else None
        eo = EvalOut(addr("loss_sum"), addr("correct"), addr("pred"), len(ks), (C.c_int32 * EVAL_MAX_TOPK)(*ks), addr("topk_correct"), addr("confusion"), addr("loss_each"),
                     addr("rank"), addr("logits"))
        self._ck(self.lib.rcn_hipx_evaluate_metrics_dev(self.net, _ptr(X), kind, float(x_scale), float(x_shift), _ptr(labels), n, WEIGHTS[weights], C.byref(eo)))
        return out

    def evaluate_metrics(self, X, labels, topk=(1, 5), confusion: bool = True, per_row: bool = False, logits: bool = False,
                         x_scale: float = 1.0 / 255.0, x_shift: float = 0.0, weights: str = "live") -> EvalReport:
        """evaluate_metrics_async, synchronised and brought to the host as an EvalReport."""
        if labels is None:
            raise ValueError("evaluate_metrics needs labels (predict / predict_logits: without)")
        out = self.evaluate_metrics_async(X, labels, topk, confusion, per_row, logits, x_scale, x_shift, weights)
        self.synchronize()
        host = lambda name: out[name].cpu().numpy() if out[name] is not None else None
        counts = host("topk_correct")
        return EvalReport(n=int(X.shape[0]), loss=float(out["loss_sum"].item()) / X.shape[0], correct=int(out["correct"].item()),
                          topk={k: int(c) for k, c in zip(out["topk"], counts)} if counts is not None else {}, confusion=host("confusion"),
                          loss_each=host("loss_each"), rank=host("rank"), logits=host("logits"), pred=host("pred"))

    def predict_logits(self, X, x_scale: float = 1.0 / 255.0, x_shift: float = 0.0, weights: str = "live"):
        """The logits of every row of a resident set, [n, classes] float32 on the device (forward()'s bits, chunk by chunk), valid on the net's stream."""
        return self.evaluate_metrics_async(X, None, (), False, False, True, x_scale, x_shift, weights)["logits"]

    def plan_eval_metrics_of_this_net(self, batch: int, n_topk: int = 2, confusion: bool = True, per_row: bool = False, logits: bool = False) -> str:
        """plan_eval_of_this_net for one chunk of an evaluate_metrics call (rcn_hipx_plan_eval_metrics_net): the `eval:` line names
        k_eval_metrics and what it was asked for; every other line is plan_eval_of_this_net's."""
        return _plan_text("rcn_hipx_plan_eval_metrics_net", self.lib.rcn_hipx_plan_eval_metrics_net, self.net, int(batch), int(n_topk), int(bool(confusion)),
                          int(bool(per_row)), int(bool(logits)))

    def gradients(self, x, labels, grad=None, loss=None):
        grad = grad if grad is not None else self.torch.empty(self.n_padded, dtype=self.torch.float32, device=self.device)
        self._ck(self.lib.rcn_hipx_gradients_dev(self.net, _ptr(x), _ptr(labels), x.shape[0], _ptr(grad), _ptr(loss)))
        return grad

    def gradients_bucketed(self, x, labels, grad, loss=None, min_bucket_bytes: int = DEFAULT_BUCKET_BYTES, on_bucket=None):
        """The gradients of `gradients`, bucket by bucket (rcn_hipx_gradients_begin_dev / _bucket_dev): after every bucket's launches are
        enqueued, on_bucket(slice_of_grad, k, n) is called -- a data-parallel step starts that slice's all-reduce there, on another stream,
        behind an event of this net's stream.  Bit-identical to `gradients`."""
        nb = C.c_int()
        self._ck(self.lib.rcn_hipx_gradients_begin_dev(self.net, _ptr(x), _ptr(labels), x.shape[0], _ptr(grad), _ptr(loss), int(min_bucket_bytes),
                                                       C.byref(nb)))
        off, ln = C.c_int64(), C.c_int64()
        for k in range(nb.value):
            self._ck(self.lib.rcn_hipx_gradients_bucket_dev(self.net, k, C.byref(off), C.byref(ln)))
            if on_bucket is not None:
                on_bucket(grad[off.value:off.value + ln.value], k, nb.value)
        return grad

    def apply(self, grad, scale: float):
        self._ck(self.lib.rcn_hipx_apply_dev(self.net, _ptr(grad), scale))

    def set_sgd(self, momentum: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False):
        """The optimiser of train_step / apply_sgd: SGD with momentum, weight decay and Nesterov, as torch.optim.SGD with dampening 0
        (include/rcn_hipx.h, rcn_hipx_set_sgd).  (0, 0, False) is plain SGD, the default."""
        self._ck(self.lib.rcn_hipx_set_sgd(self.net, float(momentum), float(weight_decay), int(bool(nesterov))))

    def set_adam(self, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, decoupled: bool = False):
        """Adam as the optimiser of train_step / apply_sgd, as torch.optim.Adam(betas, eps, weight_decay); decoupled: torch.optim.AdamW
        (include/rcn_hipx.h, rcn_hipx_set_adam).  The update count lives on the device and advances inside the step's graph.  set_sgd
        selects SGD again; both optimisers' state survives the switch."""
        self._ck(self.lib.rcn_hipx_set_adam(self.net, float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(decoupled)))

    def get_adam(self) -> dict:
        """{"betas", "eps", "weight_decay", "decoupled", "selected"}: the values of the last set_adam (its defaults before), and whether
        Adam is the optimiser now."""
        b1, b2, eps, wd, dec, sel = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_int(), C.c_int()
        self._ck(self.lib.rcn_hipx_get_adam(self.net, C.byref(b1), C.byref(b2), C.byref(eps), C.byref(wd), C.byref(dec), C.byref(sel)))
        return {"betas": (float(b1.value), float(b2.value)), "eps": float(eps.value), "weight_decay": float(wd.value), "decoupled": bool(dec.value),
                "selected": bool(sel.value)}

    def get_adam_state(self) -> Tuple[np.ndarray, np.ndarray, int]:
        """(m, v, step): the moments in the logical layout of get_params and the number of updates so far."""
        m, v, step = np.zeros(self.n_logical, dtype=np.float32), np.zeros(self.n_logical, dtype=np.float32), C.c_int64()
        self._ck(self.lib.rcn_hipx_get_adam_state(self.net, _fptr(m), _fptr(v), C.byref(step)))
        return m, v, int(step.value)

    def set_adam_state(self, m: np.ndarray, v: np.ndarray, step: int):
        m, v = np.ascontiguousarray(m, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)
        assert m.size == self.n_logical and v.size == self.n_logical
        self._ck(self.lib.rcn_hipx_set_adam_state(self.net, _fptr(m), _fptr(v), int(step)))

    def reset_adam(self):
        self._ck(self.lib.rcn_hipx_reset_adam(self.net))

    def set_loss(self, label_smoothing: float = 0.0):
        """The training loss: cross-entropy against the target smoothed by label_smoothing, as torch.nn.CrossEntropyLoss(label_smoothing=)
        (include/rcn_hipx.h, rcn_hipx_set_loss).  0 is the default: the hard loss kernels.  evaluate stays the plain cross-entropy."""
        self._ck(self.lib.rcn_hipx_set_loss(self.net, float(label_smoothing)))

    def get_loss(self) -> float:
        eps = C.c_float()
        self._ck(self.lib.rcn_hipx_get_loss(self.net, C.byref(eps)))
        return float(eps.value)

    def get_sgd(self) -> Tuple[float, float, bool]:
        mu, wd, nest = C.c_float(), C.c_float(), C.c_int()
        self._ck(self.lib.rcn_hipx_get_sgd(self.net, C.byref(mu), C.byref(wd), C.byref(nest)))
        return float(mu.value), float(wd.value), bool(nest.value)

    def get_velocity(self) -> np.ndarray:
        """The momentum buffer in the logical layout of get_params (zeros while the net has none)."""
        return self._get_flat(self.lib.rcn_hipx_get_velocity)

    def set_velocity(self, flat: np.ndarray):
        self._set_flat(self.lib.rcn_hipx_set_velocity, flat)

    def reset_velocity(self):
        self._ck(self.lib.rcn_hipx_reset_velocity(self.net))

    def set_ema(self, decay: float = 0.0):
        """An exponential moving average of the parameters, e <- e + (1 - decay) * (p_new - e), kept by the launch that updates them
        (include/rcn_hipx.h, rcn_hipx_set_ema).  The first decay > 0 starts it as a copy of the live parameters.  0 is the default: off; an
        average that exists is kept but no longer updated.  evaluate / predict score it with weights="ema"."""
        self._ck(self.lib.rcn_hipx_set_ema(self.net, float(decay)))

    def get_ema_decay(self) -> float:
        d = C.c_float()
        self._ck(self.lib.rcn_hipx_get_ema(self.net, C.byref(d)))
        return float(d.value)

    def get_ema(self) -> np.ndarray:
        """The average in the logical layout of get_params (ConvNetError, status -6, while the net has none)."""
        return self._get_flat(self.lib.rcn_hipx_get_ema_params)

    def set_ema_params(self, flat: np.ndarray):
        self._set_flat(self.lib.rcn_hipx_set_ema_params, flat)

    def reset_ema(self):
        """The average becomes a copy of the live parameters (a no-op while the net has none)."""
        self._ck(self.lib.rcn_hipx_reset_ema(self.net))

    def set_clip(self, max_norm: float = 0.0):
        """Gradient clipping by global L2 norm in front of the update, as torch.nn.utils.clip_grad_norm_(params, max_norm) over all
        parameters (include/rcn_hipx.h, rcn_hipx_set_clip): three launches in the step's graph instead of one.  0 is the default: off.
        float("inf") measures only: grad_norm() and the log are filled, the parameters are those of an unclipped step bit for bit."""
        self._ck(self.lib.rcn_hipx_set_clip(self.net, float(max_norm)))

    def get_clip(self) -> float:
        m = C.c_float()
        self._ck(self.lib.rcn_hipx_get_clip(self.net, C.byref(m)))
        return float(m.value)

    def grad_norm(self) -> Tuple[float, float]:
        """(norm, coef) of the last clipped update as float32 values; synchronises.  ConvNetError, status -6, while clipping was never on."""
        norm, coef = C.c_float(), C.c_float()
        self._ck(self.lib.rcn_hipx_get_grad_norm(self.net, C.byref(norm), C.byref(coef)))
        return float(norm.value), float(coef.value)

    def set_grad_norm_log(self, log):
        """A ring of norms on the device (rcn_hipx_set_grad_norm_log): the k-th clipped update since this call writes log[k % log.numel()].
        log: a contiguous float32 tensor on the net's device with at least one element (the net keeps a reference), or None: off."""
        t = self.torch
        if log is not None and (not t.is_tensor(log) or log.dtype != t.float32 or log.device != self.device or not log.is_contiguous()):
            raise ValueError("log: a contiguous float32 tensor on the net's device, or None")
        if log is not None and log.numel() < 1:          # (an empty tensor's pointer is NULL, which the library reads as "off")
            raise ValueError("log: at least one element")
        self._ck(self.lib.rcn_hipx_set_grad_norm_log(self.net, _ptr(log), int(log.numel()) if log is not None else 0))
        self._grad_norm_log = log

    def grad_norm_count(self) -> int:
        """Clipped updates since set_grad_norm_log (or since clipping was first switched on); synchronises."""
        c = C.c_int64()
        self._ck(self.lib.rcn_hipx_get_grad_norm_count(self.net, C.byref(c)))
        return int(c.value)

    def grad_norm_of(self, g, scale: float = 1.0):
        """The clip's norm of any float32 device tensor, (float)sqrt(sum of fl(scale * g)^2 in double), as a one-element device tensor valid
        on the net's stream (rcn_hipx_grad_norm_dev): numel % 4 == 0 and 16-byte aligned, else ConvNetError (status -1)."""
        t = self.torch
        if not t.is_tensor(g) or g.dtype != t.float32 or g.device != self.device or not g.is_contiguous():
            raise ValueError("grad_norm_of: a contiguous float32 tensor on the net's device")
        with t.cuda.stream(self.stream):
            out = t.empty(1, dtype=t.float32, device=self.device)
        self._ck(self.lib.rcn_hipx_grad_norm_dev(self.net, _ptr(g), int(g.numel()), float(scale), _ptr(out)))
        return out

    def set_accumulate(self, k: int = 1):
        """Gradient accumulation: every k consecutive training micro-steps (train_step, train_step_pair, the steps of train_epoch) form one
        update on the mean of their gradients, as (loss / k).backward() k times, then clipping, opt.step() and zero_grad()
        (include/rcn_hipx.h, rcn_hipx_set_accumulate).  1 is the default: off.  A changed k discards a pending cycle."""
        self._ck(self.lib.rcn_hipx_set_accumulate(self.net, int(k)))

    def get_accumulate(self) -> Tuple[int, int]:
        """(k, pending): pending is the number of micro-steps already accumulated in the open cycle, 0 .. k - 1."""
        k, pending = C.c_int(), C.c_int()
        self._ck(self.lib.rcn_hipx_get_accumulate(self.net, C.byref(k), C.byref(pending)))
        return int(k.value), int(pending.value)

    def reset_accumulation(self):
        """Drops a pending cycle, as zero_grad would: the next micro-step starts a new one (a no-op when nothing is pending)."""
        self._ck(self.lib.rcn_hipx_reset_accumulation(self.net))

    def get_accumulated(self) -> np.ndarray:
        """The accumulator in the logical layout of get_params; synchronises.  ConvNetError, status -6, while accumulation was never on."""
        return self._get_flat(self.lib.rcn_hipx_get_accumulated)

    def set_accumulated(self, flat: np.ndarray, pending: int):
        """The accumulator from the logical layout of get_params and the position in the open cycle, 0 .. k - 1
        (rcn_hipx_set_accumulated); synchronises.  ConvNetError, status -6, while the net does not accumulate."""
        f = np.ascontiguousarray(flat, dtype=np.float32)
        assert f.size == self.n_logical
        self._ck(self.lib.rcn_hipx_set_accumulated(self.net, _fptr(f), int(pending)))

    # ---- save and resume (include/rcn_hipx.h: rcn_hipx_snapshot_dev / rcn_hipx_restore_dev) ----
    def _state_side_stream(self):
        if getattr(self, "_state_side", None) is None:
            self._state_side = self.torch.cuda.Stream(device=self.device)
        return self._state_side

    def snapshot(self, sections="all", body=None) -> Snapshot:
        """The net's state at this point of its stream, packed into one device buffer by ONE launch (rcn_hipx_snapshot_dev): nothing blocks,
        nothing of the net is written, no graph is captured or dropped, and steps enqueued afterwards do not show in it.  sections: "all"
        (every section whose buffer exists, the scalars block and the recipe), "model" (the parameters alone: a restore leaves the
        target's recipe as it is), or a sequence of SECTIONS keys.  body: a contiguous uint8 tensor on the net's device to pack into
        (an earlier snapshot's, which it then overwrites) instead of a new one."""
        t = self.torch
        if sections == "all":
            mask = 0
        elif sections == "model":
            mask = SECTIONS["params"]
        else:
            mask = SECTIONS["params"]
            for name in sections:
                mask |= SECTIONS[name]
        if body is not None and (not t.is_tensor(body) or body.dtype != t.uint8 or body.device != self.device or not body.is_contiguous()):
            raise ValueError("snapshot: body is a contiguous uint8 tensor on the net's device")
        desc = StateDesc()
        with t.cuda.stream(self.stream):
            if body is None:
                room = state_layout(self.in_shape, self.layers, tuple(SECTIONS)).body_bytes
                body = t.empty(int(room), dtype=t.uint8, device=self.device)              # (room for every section; trimmed to the snapshot's own below)
            self._ck(self.lib.rcn_hipx_snapshot_dev(self.net, mask, _ptr(body), body.numel(), C.byref(desc)))
            event = t.cuda.Event()
            event.record(self.stream)
        if sections == "model":
            desc.flags = 0
        return Snapshot(self, desc, body[:int(desc.body_bytes)], event)

    def save(self, path, extra: Optional[bytes] = None, sections="all") -> int:
        """snapshot(sections).save(path, extra): one file holding the descriptor, the body, the caller's `extra` blob and a CRC-32.
        Returns the file's size."""
        snap = self.snapshot(sections)
        return snap.save(path, self._bn_pack_extra(extra))

    # ---- batch normalisation (include/rcn_hipx.h: rcn_hipx_set_bn; csrc/convnet_bn.hpp) ----
    def set_bn(self, momentum: float = 0.1, eps: float = 1e-5):
        """momentum and eps of every bn_relu layer, torch.nn.BatchNorm2d's meaning and defaults.  A changed value drops the net's graphs."""
        self._ck(self.lib.rcn_hipx_set_bn(self.net, float(momentum), float(eps)))

    def get_bn(self) -> Tuple[float, float, int]:
        """(momentum, eps, number of bn_relu layers)"""
        m, e, k = C.c_float(), C.c_float(), C.c_int()
        self._ck(self.lib.rcn_hipx_get_bn(self.net, C.byref(m), C.byref(e), C.byref(k)))
        return float(m.value), float(e.value), int(k.value)

    def _bn_count(self) -> int:
        c = C.c_int64()
        self._ck(self.lib.rcn_hipx_bn_stats_count(self.net, C.byref(c)))
        return int(c.value)

    def get_bn_stats(self) -> np.ndarray:
        """The running statistics, all bn_relu layers back to back: mean[C] then var[C] per layer (float32); synchronises."""
        f = np.zeros(self._bn_count(), dtype=np.float32)
        if f.size:
            self._ck(self.lib.rcn_hipx_get_bn_stats(self.net, _fptr(f)))
        return f

    def set_bn_stats(self, stats: np.ndarray):
        f = np.ascontiguousarray(stats, dtype=np.float32).ravel()
        if f.size != self._bn_count():
            raise ValueError(f"set_bn_stats: {self._bn_count()} values (mean[C] then var[C] per bn_relu layer), not {f.size}")
        if f.size:
            self._ck(self.lib.rcn_hipx_set_bn_stats(self.net, _fptr(f)))

    def reset_bn_stats(self):
        """running mean 0, running variance 1: the state of a new net"""
        self._ck(self.lib.rcn_hipx_reset_bn_stats(self.net))

    # The state file's body has no room for the running statistics (its format is the descriptor's), so save puts them, with momentum and
    # eps, in FRONT of the caller's extra blob behind a tag, and load / load_state take them off again.  A net without a bn_relu layer
    # writes the caller's blob as it is: its files are what they always were.
    _BN_TAG = struct.Struct("<8sIffI")                       # tag, number of floats, momentum, eps, 1 if a caller's blob follows the floats

    def _bn_pack_extra(self, extra: Optional[bytes]) -> Optional[bytes]:
        stats = self.get_bn_stats()
        if not stats.size:
            return extra
        m, e, _ = self.get_bn()
        return self._BN_TAG.pack(b"RCNXBNS1", stats.size, m, e, 0 if extra is None else 1) + stats.tobytes() + (b"" if extra is None else bytes(extra))

    def _bn_unpack_extra(self, extra: Optional[bytes]) -> Optional[bytes]:
        count = self._bn_count()
        if not count or extra is None or len(extra) < self._BN_TAG.size or extra[:8] != b"RCNXBNS1":
            return extra
        _, n, m, e, has = self._BN_TAG.unpack_from(extra, 0)
        at = self._BN_TAG.size
        if n != count or len(extra) < at + 4 * n:
            raise ConvNetError("state file: the running statistics in front of the extra blob are not this net's")
        self.set_bn(m, e)
        self.set_bn_stats(np.frombuffer(extra, dtype=np.float32, count=n, offset=at))
        return extra[at + 4 * n:] if has else None

    def _restore(self, desc: StateDesc, body):
        self._ck(self.lib.rcn_hipx_restore_dev(self.net, C.byref(desc), _ptr(body), int(body.numel())))
        self.synchronize()                                  # (the unpack launch has read the body: the caller may let go of it)

    def load_state(self, source) -> Optional[bytes]:
        """Restores a Snapshot (of any net of this description on this device) or a state file (a path) into THIS net
        (rcn_hipx_restore_dev): precision, tiling, the recipe and every carried section; what the snapshot does not carry is left alone.
        Everything is checked before anything changes: a refusal (ConvNetError) leaves the net bit for bit what it was.  Synchronises.
        Returns the file's `extra` blob (None for a Snapshot).  A file written by save carries a bn_relu net's running statistics, momentum and
        eps in front of that blob: they are restored too and taken off it.  A Snapshot carries gamma and beta, not the running statistics."""
        if isinstance(source, Snapshot):
            if source.body.device != self.device:
                raise ValueError("load_state: the snapshot's body lives on another device (save it and load the file)")
            self.stream.wait_event(source.event)
            self._restore(source.desc, source.body)
            return None
        with open(source, "rb") as f:
            desc, body, extra = read_state_file(f.read())
        self._restore(desc, self.to_device(body))
        return self._bn_unpack_extra(extra)

    @classmethod
    def load(cls, path, max_batch: int, device: int = 0):
        """(net, extra): a new net built from the file's descriptor -- input shape and layers -- and restored from it; `extra` is the blob
        save was given (None without one)."""
        with open(path, "rb") as f:
            desc, body, extra = read_state_file(f.read())
        in_shape, layers = desc.shape_and_layers()
        net = cls(in_shape, layers, int(max_batch), device)
        try:
            net._restore(desc, net.to_device(body))
            extra = net._bn_unpack_extra(extra)
        except Exception:
            net.close()
            raise
        return net, extra

    def plan_micro_of_this_net(self, batch: int, kind: str) -> str:
        """The launches of one kind of micro-step of THIS accumulating net (rcn_hipx_plan_micro_net): kind "first", "middle" or "last".
        plan_of_this_net describes the last one."""
        if kind not in MICRO_KINDS:
            raise ValueError(f"kind must be one of {sorted(MICRO_KINDS)}, not {kind!r}")
        return _plan_text("rcn_hipx_plan_micro_net", self.lib.rcn_hipx_plan_micro_net, self.net, int(batch), MICRO_KINDS[kind])

    def set_dropout(self, p: float = 0.0, seed: int = 0):
        """Inverted dropout behind every dense_relu layer, as torch.nn.Dropout(p) in training mode, the masks drawn inside the step's graph
        from (seed, ordinal of the training forward, site, element) (include/rcn_hipx.h, rcn_hipx_set_dropout).  0 is the default: off.
        forward, evaluate and predict never drop.  Data-parallel ranks give different seeds."""
        self._ck(self.lib.rcn_hipx_set_dropout(self.net, float(p), int(seed) & (2 ** 64 - 1)))

    def get_dropout(self) -> Tuple[float, int, int]:
        """(p, seed, sites): sites is the number of dense_relu layers."""
        p, seed, sites = C.c_float(), C.c_uint64(), C.c_int()
        self._ck(self.lib.rcn_hipx_get_dropout(self.net, C.byref(p), C.byref(seed), C.byref(sites)))
        return float(p.value), int(seed.value), int(sites.value)

    def dropout_state(self) -> int:
        """The training forwards dropout has counted so far (the ordinal of the last one); synchronises."""
        t = C.c_int64()
        self._ck(self.lib.rcn_hipx_get_dropout_state(self.net, C.byref(t)))
        return int(t.value)

    def set_dropout_state(self, t: int):
        """The next training forward draws with ordinal t + 1."""
        self._ck(self.lib.rcn_hipx_set_dropout_state(self.net, int(t)))

    def dropout_apply(self, site: int, t: int, a):
        """The forward launch of dropout site `site` with the net's p and seed and an explicit ordinal t, IN PLACE on a: a contiguous float32
        [B, units of the site] tensor on the net's device (rcn_hipx_dropout_apply_dev), enqueued on the net's stream.  The net's own ordinal
        is not touched.  Returns a."""
        tt = self.torch
        if not tt.is_tensor(a) or a.dtype != tt.float32 or a.device != self.device or not a.is_contiguous() or a.dim() != 2:
            raise ValueError("dropout_apply: a contiguous two-dimensional float32 tensor on the net's device")
        units = [l[1] for l in self.layers if l[0] == "dense_relu"]
        if not 0 <= int(site) < len(units) or a.shape[1] != units[int(site)]:
            raise ValueError(f"dropout_apply: site in 0 .. {len(units) - 1} and a of [B, units of that site]")
        self._ck(self.lib.rcn_hipx_dropout_apply_dev(self.net, int(site), int(t), _ptr(a), int(a.shape[0])))
        return a

    def apply_sgd(self, grad, grad_scale: float, lr: float):
        """The data-parallel half of the configured optimiser (set_sgd's or set_adam's): the same update from a padded gradient buffer,
        scaled by grad_scale first."""
        self._ck(self.lib.rcn_hipx_apply_sgd_dev(self.net, _ptr(grad), grad_scale, lr))

    def unpad(self, padded) -> np.ndarray:
        f = np.zeros(self.n_logical, dtype=np.float32)
        self._ck(self.lib.rcn_hipx_unpad_host(self.net, _ptr(padded), _fptr(f)))
        return f

    def step_hbm_floor_bytes(self, B: int, stored16: bool = False) -> float:
        """HBM floor of one training step with activations stored as they are (fp32; stored16: the convolutional stage's maps and their
        gradients as bf16, "bf16_stored"): every layer's input read and output written once in the forward
        pass; in the backward pass dZ read and dX written once by the input-gradient GEMM (not for the first layer) and the input and dZ
        read once more by the weight-gradient GEMM; parameters read twice and written once.  Fusion (pool in the epilogue, ReLU masks in
        the consumer) can go below it only by not materialising a tensor at all."""
        H, W, Cc = self.in_shape
        total, first = 0.0, True
        es_in = 4                                            # bytes per element of the current layer's input tensor
        es_stage = 2 if stored16 else 4
        maps = []                                            # every layer's output (H, W, C): a down shortcut reads its source's
        for l in self.layers:
            maps.append(None)
            if l[0] in _CONV_GEOMETRY:
                # input read and output written by the forward pass; dZ read and dX written by the input gradient (not for the first layer);
                # input and dZ read by the weight gradient; [W | b] read twice and written once
                taps, stride, depthwise = _CONV_GEOMETRY[l[0]]
                oH, oW, Co = H // stride, W // stride, Cc if depthwise else l[1]
                es_out = es_stage if l[0] == "conv" else 4       # only the ReLU convolution's map is stored as the stage's
                params = (taps if depthwise else taps * Cc) * Co + Co
                i, o = H * W * Cc * es_in, oH * oW * Co * es_out
                total += B * ((i + o) + (0 if first else (i + o)) + (i + o)) + 3 * params * 4
                H, W, Cc, first, es_in = oH, oW, Co, False, es_out
            elif l[0] == "bn_add_relu_down":
                # as bn_relu, and the shortcut: a quarter of the source's map (its Cs channels at every second pixel) read by the apply pass;
                # the add pass of the backward reads that quarter of the source's gradient and this layer's window and writes the quarter
                m = H * W * Cc * 4
                sm = H * W * maps[len(maps) - 1 - l[1]][2] * 4
                total += B * (3 * m + 4 * m + sm + 3 * sm)
            elif l[0] in ("bn_relu", "bn"):
                # forward: the map read twice (statistics, apply) and written once; backward: three maps read over its two passes (x and dy
                # by the sums, then one more pass's worth -- a re-read that hits the cache, the gate map -- is not counted) and one written
                m = H * W * Cc * 4
                total += B * (3 * m + 4 * m)
            elif l[0] in ("bn_add_relu", "bn_add"):
                # as bn_relu, and the skip: its map read once more by the apply pass; the add pass of the backward reads the source's
                # gradient and this layer's and writes the source's (the gate maps are not counted, as above)
                m = H * W * Cc * 4
                total += B * (3 * m + 4 * m + m + 3 * m)
            elif l[0] == "global_avgpool":
                # forward: the map read once and [B][C] written; backward: the map's gradient written once ([B][C] read; the gate map is
                # not counted, as above)
                m, o = H * W * Cc * 4, Cc * 4
                total += B * ((m + o) + (o + m))
                H, W, es_in = 1, 1, 4
            elif l[0] == "pool":
                i, o = H * W * Cc * es_stage, (H // 2) * (W // 2) * Cc * es_stage
                total += B * 2 * (i + o)
                H, W = H // 2, W // 2
            else:
                i, o = H * W * Cc * es_in, l[1] * 4
                total += B * ((i + o) + (0 if first else (i + o)) + (i + o)) + 3 * (H * W * Cc * l[1] + l[1]) * 4
                H, W, Cc, first, es_in = 1, 1, l[1], False, 4
            maps[-1] = (H, W, Cc)
        return total

    def step_flops(self, B: int) -> float:
        f = C.c_double()
        self._ck(self.lib.rcn_hipx_step_flops(self.net, B, C.byref(f)))
        return f.value
