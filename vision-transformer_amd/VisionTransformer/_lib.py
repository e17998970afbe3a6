"""ctypes binding of libvit_hip.so (include/vit_hip.h).

The library is built in-tree by `make -C vision-transformer_amd/csrc` (or `__graft_entry__.build()`).  It is loaded
AFTER `import torch`, so its DT_NEEDED libamdhip64.so.7 resolves to the HIP runtime torch already mapped.
There is deliberately no fallback: if the library is missing, every HIP-path call raises.
"""
import ctypes
import os

import torch  # noqa: F401  (must be imported first: provides the HIP runtime the library binds to)

LIB_PATH = os.environ.get("VIT_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvit_hip.so")
ABI_VERSION = 18

F32, BF16, MASK4 = 0, 1, 2
FLAG_SHARED_CUS = 1          # VIT_FLAG_SHARED_CUS (vit_hip.h)
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


class GemmDesc(ctypes.Structure):
    _fields_ = [
        ("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("c", ctypes.c_void_p),
        ("lda", ctypes.c_int64), ("ldb", ctypes.c_int64), ("ldc", ctypes.c_int64),
        ("m", ctypes.c_int64), ("n", ctypes.c_int64), ("k", ctypes.c_int64),
        ("a_kcontig", ctypes.c_int32), ("b_kcontig", ctypes.c_int32),
        ("in_dtype", ctypes.c_int32), ("out_dtype", ctypes.c_int32),
        ("alpha", ctypes.c_float), ("beta", ctypes.c_float),
        ("bias", ctypes.c_void_p),
        ("act", ctypes.c_int32), ("aux_dtype", ctypes.c_int32),
        ("aux", ctypes.c_void_p), ("ldaux", ctypes.c_int64),
        ("res", ctypes.c_void_p), ("ldres", ctypes.c_int64), ("res_rowmod", ctypes.c_int64),
        ("res_dtype", ctypes.c_int32),
        ("dropout_p", ctypes.c_float), ("dropout_seed", ctypes.c_uint32),
        ("split_k", ctypes.c_int32),
        ("out_group_rows", ctypes.c_int64), ("out_group_stride", ctypes.c_int64),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
        ("colsum_part", ctypes.c_void_p),
        ("mask_out", ctypes.c_void_p),
        ("dropout_row_stride", ctypes.c_int64),
        ("flags", ctypes.c_int32),
        ("dropout_row0", ctypes.c_int64),
    ]


class ColsumJob(ctypes.Structure):
    _fields_ = [("part", ctypes.c_void_p), ("nparts", ctypes.c_int64), ("cols", ctypes.c_int64),
                ("nsets", ctypes.c_int32), ("out", ctypes.c_void_p * 3), ("beta", ctypes.c_float)]


class TensorChunk(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("shadow", ctypes.c_void_p), ("n", ctypes.c_int64)]


class MixItem(ctypes.Structure):      # vit_mix_item, 24 bytes
    _fields_ = [("src", ctypes.c_int32), ("w", ctypes.c_float), ("y0", ctypes.c_int32), ("y1", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("x1", ctypes.c_int32)]


class AugItem(ctypes.Structure):      # vit_aug_item, 36 bytes
    _fields_ = [(n, ctypes.c_int32) for n in ("x0", "y0", "cw", "ch", "flip", "ey0", "ey1", "ex0", "ex1")]


class RaLayer(ctypes.Structure):      # vit_ra_layer, 72 bytes
    _fields_ = [("coef", ctypes.c_double * 6), ("kind", ctypes.c_int32), ("iarg0", ctypes.c_int32),
                ("iarg1", ctypes.c_int32), ("farg", ctypes.c_float), ("fill", ctypes.c_uint8 * 4),
                ("pad_", ctypes.c_int32)]


RA_MAX_LAYERS = 4                     # VIT_RA_MAX_LAYERS (vit_hip.h)


class RaItem(ctypes.Structure):       # vit_ra_item, 288 bytes
    _fields_ = [("layer", RaLayer * RA_MAX_LAYERS)]


# VIT_RA_* kinds (vit_hip.h)
(RA_NONE, RA_AUTOCONTRAST, RA_EQUALIZE, RA_INVERT, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_COLOR, RA_CONTRAST,
 RA_BRIGHTNESS, RA_SHARPNESS, RA_AFFINE, RA_KINDS) = range(13)


class OptGroup(ctypes.Structure):     # vit_opt_group, 32 bytes, host memory
    _fields_ = [(n, ctypes.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "bias_corr1",
                                              "bias_corr2")] + [("flags", ctypes.c_int32)]


OPT_MAX_GROUPS, OPT_ADAPT, OPT_TRUST_CLIP = 64, 1, 2      # VIT_OPT_* (vit_hip.h)

# the tiled form of vit_augment_to_tensor (vit_hip.h VIT_AUG_TILE_*): tile rows x columns, most source rows of a tile
AUG_TILE_ROWS, AUG_TILE_COLS, AUG_TILE_MAX_SPAN = 16, 64, 80

_P, _I64, _I32, _F, _U32 =ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_uint32

# name: (restype, argtypes)
_SIGS = {
    "vit_abi_version": (ctypes.c_int, []),
    "vit_last_error": (ctypes.c_char_p, []),
    "vit_set_option": (ctypes.c_int, [ctypes.c_char_p, _I64]),
    "vit_get_option": (_I64, [ctypes.c_char_p]),
    "vit_gemm_workspace_bytes": (_I64, [ctypes.POINTER(GemmDesc)]),
    "vit_gemm": (ctypes.c_int, [ctypes.POINTER(GemmDesc), _P]),
    "vit_gemm_split_k_hint": (ctypes.c_int, [_I64, _I64, _I64, _I32]),
    "vit_im2col": (ctypes.c_int, [_P, _I32, _P, _I32, _I64, _I64, _I64, _I64, _I64, _P]),
    "vit_col2im": (ctypes.c_int, [_P, _I32, _P, _I32, _I64, _I64, _I64, _I64, _I64, _P]),
    "vit_embed_cls": (ctypes.c_int, [_P, _P, _P, _I32, _I64, _I64, _I64, _P]),
    "vit_layernorm_fwd": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _P, _I64, _I64, _F, _I32, _P]),
    "vit_layernorm_bwd_parts": (_I64, [_I64, _I64]),
    "vit_layernorm_bwd": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _F, _U32, _P, _P, _I32, _I64,
                                         _I64, _I32, _P]),
    "vit_attn_fwd": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _F, _I32, _I64, _P]),
    "vit_attn_bwd_uses_o32": (ctypes.c_int, [_I64, _I64, _I64, _I64, _I32]),
    "vit_attn_bwd_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64, _I32]),
    "vit_attn_bwd": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _F, _I32, _P, _I32, _P]),
    "vit_attn_fwd_row0": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _F, _I32, _P]),
    "vit_attn_bwd_row0": (ctypes.c_int, [_P, _P, _I64, _P, _I64, _I64, _I64, _I64, _F, _I32, _P]),
    "vit_colsum_workspace_bytes": (_I64, [_I64, _I64]),
    "vit_colsum": (ctypes.c_int, [_P, _I64, _I32, _I64, _I64, _P, _F, _F, _P, _P]),
    "vit_colsum_finish": (ctypes.c_int, [_P, _I64, _I64, _I32, _P, _P, _P, _F, _P]),
    "vit_colsum_finish_batch": (ctypes.c_int, [ctypes.POINTER(ColsumJob), _I32, _P]),
    "vit_copy2d": (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _I64, _I64, _I64, _I64, _F, _P]),
    "vit_dropout_bwd": (ctypes.c_int, [_P, _P, _I32, _I64, _F, _U32, _F, _P]),
    "vit_mask4_apply": (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _P, _I64, _I64, _F, _P]),
    "vit_relu_bwd": (ctypes.c_int, [_P, _P, _P, _I32, _I64, _P]),
    "vit_gelu_fwd": (ctypes.c_int, [_P, _P, _I64, _P]),
    "vit_gelu_bwd": (ctypes.c_int, [_P, _P, _P, _I64, _P]),
    "vit_softmax_xent": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P, _P, _P]),
    "vit_resize_ksize": (ctypes.c_int, [_I64, _I64]),
    "vit_resize_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64]),
    "vit_resize_to_tensor": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _I64, _P, _I32, _P, _I64, _P]),
    "vit_adamw": (ctypes.c_int, [_P, _I64, _F, _F, _F, _F, _F, _F, _F, _F, _I32, _P]),
    "vit_pack": (ctypes.c_int, [_P, _I64, _I32, _P]),
    "vit_grad_sumsq": (ctypes.c_int, [_P, _I64, _F, _P, _P]),
    "vit_grad_clip_finish": (ctypes.c_int, [_P, _I64, _F, _P, _P]),
    "vit_adamw_clipped": (ctypes.c_int, [_P, _I64, _F, _F, _F, _F, _F, _F, _F, _F, _I32, _P, _P]),
    "vit_adamw_ema": (ctypes.c_int, [_P, _P, _I64, _F, _F, _F, _F, _F, _F, _F, _F, _I32, _F, _P, _P]),
    "vit_ema_swap": (ctypes.c_int, [_P, _P, _I64, _I32, _P]),
    # added under ABI 18 (purely added entry points do not change the version, vit_hip.h)
    "vit_softmax_xent_mixed": (ctypes.c_int, [_P, _P, _P, _P, _F, _I64, _I64, _P, _P, _P, _P]),
    "vit_mix_batch": (ctypes.c_int, [_P, _P, _I32, _I64, _I64, _I64, _I64, _P, _P]),
    "vit_augment_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64]),
    "vit_augment_to_tensor": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _F, _P, _I32, _P, _I64, _P]),
    "vit_drop_path_rows": (ctypes.c_int, [_P, _U32, _I64, _I64, _I64, ctypes.POINTER(ctypes.c_float), _P]),
    "vit_gemm_rowscale": (ctypes.c_int, [ctypes.POINTER(GemmDesc), _P, _P]),
    "vit_gemm_kernel_choice": (ctypes.c_int, [ctypes.POINTER(GemmDesc), _P, ctypes.POINTER(_I32),
                                              ctypes.POINTER(_I32)]),
    "vit_lamb_moments": (ctypes.c_int, [_P, _I64, _F, _F, _F, _F, _F, _F, _F, _P, _P, _P]),
    "vit_lamb_trust": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _P]),
    "vit_lamb_update": (ctypes.c_int, [_P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _I32, _F, _P, _P]),
    "vit_adamw_groups": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(OptGroup), _I32, _F, _I32, _F, _P, _P]),
    "vit_lamb_moments_groups": (ctypes.c_int, [_P, _P, _I64, ctypes.POINTER(OptGroup), _I32, _F, _P, _P, _P]),
    "vit_lamb_trust_groups": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(OptGroup), _I32, _P, _P, _P]),
    "vit_lamb_update_groups": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, ctypes.POINTER(OptGroup), _I32, _I32, _F,
                                              _P, _P]),
    "vit_eval_update": (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "vit_augment_to_u8": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _I64, _P]),
    "vit_randaug_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "vit_randaug_to_tensor": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _I32, _I32, _P, _P, _P, _F, _P, _I32, _P, _I64,
                                             _P]),
    "vit_attn_rollout_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64, _I32, _I32]),
    "vit_attn_rollout_step": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _F, _I32, _I32, _P, _P]),
    "vit_attn_rollout_step_form": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _F, _I32, _I32, _I32, _P, _P]),
    "vit_patch_keep": (ctypes.c_int, [_U32, _I64, _I64, _I64, _I64, _P, _P, _P]),
    "vit_im2col_gather": (ctypes.c_int, [_P, _I32, _P, _I32, _P, _I64, _I64, _I64, _I64, _I64, _I64, _P]),
    "vit_gather_pos": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "vit_pos_grad_gather": (ctypes.c_int, [_P, _I32, _P, _P, _I64, _I64, _I64, _I64, _F, _P]),
    "vit_col2im_scatter": (ctypes.c_int, [_P, _I32, _P, _P, _I32, _I64, _I64, _I64, _I64, _I64, _I64, _P]),
    "vit_softmax_xent_distill": (ctypes.c_int, [_P, _P, _P, _P, _P, _F, _I32, _F, _F, _I64, _I64, _P, _P, _P, _P]),
}

EPI_BDR, EPI_SLAB, EPI_GENERAL, EPI_BDRS = 3, 4, 5, 8    # VIT_EPI_* (vit_hip.h): kinds vit_gemm_kernel_choice reports

DROP_PATH_MAX_LAYERS = 64    # VIT_DROP_PATH_MAX_LAYERS (vit_hip.h)
EVAL_MAXK = 16               # VIT_EVAL_MAXK (vit_hip.h)
PATCH_KEEP_MAX_N = 4096      # VIT_PATCH_KEEP_MAX_N (vit_hip.h)
ROLLOUT_MEAN, ROLLOUT_MAX, ROLLOUT_MIN = 0, 1, 2             # VIT_ROLLOUT_* (vit_hip.h)
DISTILL_SOFT, DISTILL_HARD = 0, 1                            # VIT_DISTILL_* (vit_hip.h)
ROLLOUT_FORM_AUTO, ROLLOUT_FORM_VALU, ROLLOUT_FORM_MFMA = 0, 1, 2   # `form` of vit_attn_rollout_step_form

EXPORTED_SYMBOLS = tuple(_SIGS.keys())

_lib = None


class HipLibraryError(RuntimeError):
    pass


def load():
    """Load libvit_hip.so (once).  Raises HipLibraryError when it is missing or its ABI does not match."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(f"{LIB_PATH} not found: build it with `make -C vision-transformer_amd/csrc` or "
                              "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = lib.vit_abi_version()
    if v != ABI_VERSION:
        raise HipLibraryError(f"libvit_hip ABI version {v} != expected {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().vit_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")


def call(name, *args):
    lib = load()
    check(getattr(lib, name)(*args), name)


def set_option(name, value):
    """vit_set_option (vit_hip.h): process-wide launch option of the library (kernel-variant choice for A/B runs and
    tests; defaults are the shipped configuration).  Returns the previous value."""
    lib = load()
    prev = lib.vit_get_option(name.encode())
    check(lib.vit_set_option(name.encode(), int(value)), f"vit_set_option({name!r})")
    return prev


def get_option(name):
    v = load().vit_get_option(name.encode())
    if v == -(1 << 63):
        raise KeyError(f"unknown libvit_hip option {name!r}")
    return v


class option:
    """Context manager: `with _lib.option("gemm_persist", 0): ...` sets an option and restores it on exit."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.prev)
        return False
