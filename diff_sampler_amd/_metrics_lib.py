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
DSM_VERSION = 1
DSM_MAX_K = 8
DS_OK, DS_E_ARG, DS_E_ALIGN, DS_E_SHAPE = 0, -1, -2, -3

_SIGNATURES = {
    'dsm_version': (C.c_int, []),
    'dsm_error_string': (C.c_char_p, [C.c_int]),
    'dsm_prdc_workspace_bytes': (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    'dsm_prdc_splits': (C.c_int, [C.c_int, C.c_int]),
    'dsm_knn_radii_sq': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_longlong, vp]),
    'dsm_prdc_cross': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp,
                                 C.c_longlong, vp]),
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
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
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
