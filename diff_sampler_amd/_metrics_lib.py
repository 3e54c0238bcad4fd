"""ctypes binding of csrc/metrics/libdsmetrics.so (the C ABI declared in csrc/metrics/ds_metrics.h): the evaluation metrics that run
on the engine next to, not inside, libdsamd.so.

As with ``_lib``: no CPU fallback behind a device call -- a missing library or a failing call raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DS_METRICS_LIB_PATH') or os.path.join(_HERE, 'csrc', 'metrics', 'libdsmetrics.so')

vp = C.c_void_p
DSM_VERSION = 2
DSM_MAX_K = 8
DS_OK, DS_E_ARG, DS_E_ALIGN, DS_E_SHAPE = 0, -1, -2, -3
DSM_ACT_NONE, DSM_ACT_GELU, DSM_ACT_QUICK_GELU = 0, 1, 2          # dsm_gemm_split_args.act


class DsmAttnArgs(C.Structure):
    """dsm_attn_args: ds_attn_args' fields, its three trailing switches reserved (0)."""
    _fields_ = [('q', vp), ('k', vp), ('v', vp), ('out', vp), ('ldq', C.c_int), ('ldk', C.c_int), ('ldv', C.c_int), ('ldo', C.c_int),
                ('q_bs', C.c_longlong), ('k_bs', C.c_longlong), ('v_bs', C.c_longlong), ('o_bs', C.c_longlong), ('batch', C.c_int),
                ('heads', C.c_int), ('sq', C.c_int), ('skv', C.c_int), ('d', C.c_int), ('scale', C.c_float), ('reserved', C.c_int * 3)]


class DsmGemmSplitArgs(C.Structure):
    """dsm_gemm_split_args: out = act(x W^T 2^-shift + bias) + res with split-fp16 weights (ops.pack_linear_weight_split)."""
    _fields_ = [('x', vp), ('ldx', C.c_int), ('rows', C.c_longlong), ('k', C.c_int), ('w_split', vp), ('shift', C.c_int), ('cout', C.c_int),
                ('bias', vp), ('res', vp), ('res_ld', C.c_int), ('act', C.c_int), ('out', vp), ('out_ld', C.c_int), ('reserved', C.c_int * 3)]


class DsmFirArgs(C.Structure):
    """dsm_fir_args: out = (fir(x) + bias + res) * out_scale, fir = the depthwise 4-tap down (up = 0; pad 0 / 1) or up (up = 1, pad = 1) filter."""
    _fields_ = [('x', vp), ('ld_x', C.c_int), ('n', C.c_int), ('h', C.c_int), ('w', C.c_int), ('c', C.c_int), ('up', C.c_int), ('pad', C.c_int),
                ('taps', C.c_float * 4), ('bias', vp), ('res', vp), ('res_ld', C.c_int), ('out_scale', C.c_float), ('out', vp),
                ('out_ld', C.c_int), ('reserved', C.c_int * 3)]


class DsmZeroBorderArgs(C.Structure):
    """The by-value arguments of dsm_zero_border as a record (tools/plan_dump.py reads launches field by field)."""
    _fields_ = [('x', vp), ('out', vp), ('outer', C.c_longlong), ('h', C.c_int), ('w', C.c_int), ('inner', C.c_int), ('p', C.c_int)]


_SIGNATURES = {
    'dsm_version': (C.c_int, []),
    'dsm_error_string': (C.c_char_p, [C.c_int]),
    'dsm_prdc_workspace_bytes': (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    'dsm_prdc_splits': (C.c_int, [C.c_int, C.c_int]),
    'dsm_knn_radii_sq': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_longlong, vp]),
    'dsm_prdc_cross': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp,
                                 C.c_longlong, vp]),
    'dsm_attention': (C.c_int, [C.POINTER(DsmAttnArgs), vp]),
    'dsm_attention_supported': (C.c_int, [C.c_int]),
    'dsm_gelu_rows': (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_longlong, C.c_int, vp]),
    'dsm_vit_patch_rows': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), vp, C.c_int, vp]),
    'dsm_vit_tokens': (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    'dsm_gather_rows': (C.c_int, [vp, C.c_int, C.c_longlong, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    'dsm_clip_score': (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    'dsm_resize_crop_u8': (C.c_int, [vp, C.c_longlong, C.c_int] + [C.c_int] * 8 + [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp]),
    'dsm_gemm_split': (C.c_int, [C.POINTER(DsmGemmSplitArgs), vp]),
    'dsm_gemm_split_supported': (C.c_int, [C.c_longlong, C.c_int, C.c_int]),
    'dsm_fir_resample': (C.c_int, [C.POINTER(DsmFirArgs), vp]),
    'dsm_fir_resample_supported': (C.c_int, [C.c_int] * 5),
    'dsm_zero_border': (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    'dsm_dynamic_threshold_large': (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_float, vp]),
    'dsm_traj_gram': (C.c_int, [vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, vp, vp, C.c_longlong, vp]),
    'dsm_traj_gram_workspace_bytes': (C.c_longlong, [C.c_int, C.c_longlong, C.c_int]),
    'dsm_traj_gram_splits': (C.c_int, [C.c_int, C.c_longlong]),
    'dsm_row_sqdist': (C.c_int, [vp, vp, C.c_longlong, C.c_longlong, vp, vp]),
}

EXPORTS = tuple(_SIGNATURES)
_lib = None


class DsMetricsError(RuntimeError):
    pass


def load():
    """Load libdsmetrics.so (once).  Raises if it has not been built or reports another ABI version."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401      (first: the library then binds to the HIP runtime torch ships, as _lib.load explains)
    if not os.path.exists(LIB_PATH):
        raise DsMetricsError(f'{LIB_PATH} is missing: build it with `python diff_sampler_amd/build.py` (or __graft_entry__.build()).  '
                             f'The device metrics have no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise DsMetricsError(f'{LIB_PATH} does not export {name}: it was built from older sources, rebuild it '
                                 f'(python diff_sampler_amd/build.py)') from None
        fn.restype, fn.argtypes = res, args
    if lib.dsm_version() != DSM_VERSION:
        raise DsMetricsError(f'{LIB_PATH} reports ABI version {lib.dsm_version()}, this binding is written for {DSM_VERSION}: rebuild it '
                             f'(python diff_sampler_amd/build.py)')
    _lib = lib
    return lib


def check(code, what=''):
    if code != 0:
        msg = load().dsm_error_string(code)
        raise DsMetricsError(f'{what or "libdsmetrics call"} failed with code {code}: {msg.decode() if msg else "?"}')
