"""The resize and centre crop of the CLIP-score transform on the device, bit for bit what ``clip_score.preprocess`` (PIL) computes.

Pillow's 8-bit resampler is integer arithmetic once its coefficient tables exist: per axis a table of (first tap, taps) and of weights
rounded to 22 fractional bits; each of the two separable passes (horizontal first) accumulates ``pixel * weight`` in int32 from
``1 << 21``, shifts right by 22 and clamps to uint8.  ``resample_coeffs`` restates the tables (Resample.c: precompute_coeffs +
normalize_coeffs_8bpc, bicubic a = -0.5) in Python floats in Pillow's order of operations, ``resize_reference`` the two passes in numpy,
``dsm_resize_crop_u8`` (csrc/metrics/image_prep.hip) runs them on the device for the cropped window only.

    resize_center_crop(images_u8 [B, H, W, 3], size) -> device uint8 [B, 3, size, size]

No fallback behind the device call: a geometry the kernel refuses raises, naming the geometry.
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import torch

PRECISION_BITS = 22           # Pillow: 32 - 8 - 2
COEFF_LIMIT = 1 << 23         # the kernel multiplies with the 24-bit multiplier: every weight lies in (-2^23, 2^23)


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=64)
def _coeffs(in_size: int, out_size: int):
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            k = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
            if abs(k) >= COEFF_LIMIT:
                raise ValueError(f'resample_coeffs({in_size}, {out_size}): weight {k} of output {i} leaves the 24-bit range')
            coeffs[i, x] = k
        bounds[i] = (xmin, xmax)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


def resample_coeffs(in_size: int, out_size: int):
    """Pillow's bicubic tables for one axis: ``bounds`` int32 [out, 2] = (first source index, number of taps) per output index and
    ``coeffs`` int32 [out, ksize], the weights times 2^22 rounded half away from zero, zeros behind the taps.  Read-only, cached."""
    if in_size < 1 or out_size < 1:
        raise ValueError(f'resample_coeffs: sizes must be positive, got {in_size} -> {out_size}')
    return _coeffs(int(in_size), int(out_size))


def crop_geometry(h: int, w: int, size: int):
    """(nh, nw, top, left) of ``clip_score.preprocess``: the shorter side becomes `size`, the longer ``int(size * long / short)``, the
    crop starts at ``int(round((n - size) / 2.0))`` (Python's round: halves go to even)."""
    if (w, h) == (size, size):
        return size, size, 0, 0
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    return nh, nw, int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))


def _pass(a, bounds, coeffs, first, count):
    """One pass along axis 1 of int32 `a` [rows, in, ch] for the output indices first ... first + count - 1."""
    out = np.empty((a.shape[0], count, a.shape[2]), dtype=np.uint8)
    for j in range(count):
        xmin, n = (int(v) for v in bounds[first + j])
        acc = np.full((a.shape[0], a.shape[2]), 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for k in range(n):
            acc += a[:, xmin + k, :] * coeffs[first + j, k]
        out[:, j, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_reference(array_hwc_u8, size: int) -> np.ndarray:
    """What the kernel must compute, in numpy: uint8 [h, w, 3] -> uint8 [3, size, size].  Horizontal pass, then vertical, a pass whose
    size does not change skipped, the intermediate rounded to uint8, only the cropped window evaluated."""
    a = np.asarray(array_hwc_u8)
    if a.ndim != 3 or a.dtype != np.uint8:
        raise ValueError(f'resize_reference takes a uint8 [h, w, channels] array, got {a.shape} {a.dtype}')
    h, w = a.shape[:2]
    nh, nw, top, left = crop_geometry(h, w, size)
    x = a.astype(np.int32)
    x = _pass(x, *resample_coeffs(w, nw), left, size) if nw != w else x[:, left:left + size]
    x = x.astype(np.int32).transpose(1, 0, 2)                  # [size, h, ch]: the vertical pass runs along axis 1 as well
    x = _pass(x, *resample_coeffs(h, nh), top, size) if nh != h else x[:, top:top + size]
    return np.ascontiguousarray(x.astype(np.uint8).transpose(2, 1, 0))


# ---- device ------------------------------------------------------------------------------------------------------------------------------
_tables = {}          # (h, w, size, device) -> (nh, nw, top, left, [hbounds, hcoeffs, hk, vbounds, vcoeffs, vk])


def device_tables(h: int, w: int, size: int, device):
    """The geometry and the uploaded tables of one source size, built once per (h, w, size, device).  A skipped pass has no table."""
    key = (h, w, size, str(device))
    if key not in _tables:
        nh, nw, top, left = crop_geometry(h, w, size)
        t = []
        for n_in, n_out in ((w, nw), (h, nh)):
            if n_in == n_out:
                t += [None, None, 0]
            else:
                b, c = resample_coeffs(n_in, n_out)
                t += [torch.from_numpy(b.copy()).to(device), torch.from_numpy(c.copy()).to(device), c.shape[1]]
        _tables[key] = (nh, nw, top, left, t)
    return _tables[key]


def resize_center_crop(images_u8, size: int, device='cuda') -> torch.Tensor:
    """uint8 [B, H, W, 3] (host or device; any row pitch and image stride, pixels interleaved and contiguous) -> device uint8
    [B, 3, size, size]: ``torch.stack([clip_score.preprocess(image, size) for image in images])`` to the last bit."""
    from . import _lib, _metrics_lib
    x = torch.as_tensor(images_u8)
    if x.dim() != 4 or x.shape[3] != 3 or x.dtype != torch.uint8 or x.shape[0] < 1:
        raise ValueError(f'resize_center_crop takes uint8 images [B, H, W, 3], got {tuple(x.shape)} {x.dtype}')
    if not x.is_cuda:
        x = x.to(device)
    B, h, w = (int(v) for v in x.shape[:3])
    if x.stride(3) != 1 or x.stride(2) != 3 or x.stride(1) < 3 * w:
        x = x.contiguous()
    nh, nw, top, left, (hb, hc, hk, vb, vc, vk) = device_tables(h, w, int(size), x.device)
    out = torch.empty(B, 3, size, size, dtype=torch.uint8, device=x.device)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
    code = _metrics_lib.load().dsm_resize_crop_u8(p(x), x.stride(0), x.stride(1), B, h, w, nh, nw, top, left, int(size), p(hb), p(hc), hk,
                                                  p(vb), p(vc), vk, p(out), _lib.stream_ptr())
    _metrics_lib.check(code, f'dsm_resize_crop_u8 ({B} images {h}x{w} -> {nh}x{nw}, crop {size} at ({top}, {left}))')
    return out
