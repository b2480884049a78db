"""The detection stage on a caller's image: what ``dog`` and ``dom`` run once their image is
stored -- InteractiveIntegral.findPeaks (InteractiveIntegral.java:360-468), the
``x % ij_threads`` order, and Localization (Localization.java:19-88) -- through
``spim_detect_peaks`` / ``spim_detect_interest_points``.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import check
from .dog import IP_DTYPE

__all__ = ["peaks", "interest_points", "tiles", "Tiles", "PEAK_DTYPE", "IP_DTYPE", "ROUTE_AUTO", "ROUTE_WAVE",
           "ROUTE_APPEND"]

ROUTE_AUTO, ROUTE_WAVE, ROUTE_APPEND = 0, 1, 2    # SPIM_DETECT_ROUTE_*

# spim_peak as a numpy record
PEAK_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("intensity", "<f4"), ("is_min", "<i4"),
                       ("is_max", "<i4")])


class Tiles(NamedTuple):
    """spim_detect_tiles: the stage's tile sizes, from the constants in the code."""
    columns: int      # columns tested per wave
    rows: int         # rows per lane
    planes: int       # centre planes per chunk
    buffer: int       # entries of a wave's candidate buffer
    cap_floor: int    # the least capacity of the candidate lists


def tiles() -> Tiles:
    """Needs no GPU."""
    sizes = (C.c_int32 * 5)()
    _lib.load().spim_detect_tiles(sizes)
    return Tiles(*(int(v) for v in sizes))


def _image(img, device):
    """(pointer, dims, keep-alive, device) of a [z, y, x] numpy array or GPU tensor."""
    if hasattr(img, "is_cuda") and img.is_cuda:
        import torch
        if img.dtype != torch.float32 or not img.is_contiguous():
            img = img.contiguous().float()
        if img.dim() != 3:
            raise ValueError("img must be 3D [z, y, x]")
        torch.cuda.synchronize(img.device)   # the library runs on its own stream
        if device is None:
            device = img.device.index
        ptr = C.c_void_p(img.data_ptr())
    else:
        img = np.ascontiguousarray(img, np.float32)
        if img.ndim != 3:
            raise ValueError("img must be 3D [z, y, x]")
        if device is None:
            device = 0
        ptr = C.c_void_p(img.ctypes.data)
    return ptr, (C.c_int64 * 3)(img.shape[2], img.shape[1], img.shape[0]), img, int(device)


def _cap(img, capacity):
    n = img.size if isinstance(img, np.ndarray) else img.numel()
    return int(capacity) if capacity is not None else max(1024, n // 64)


def _capacity(call, dtype, ctype, cap):
    """The capacity rule: a second call with the exact capacity when the first was short."""
    n = C.c_int64(0)
    while True:
        buf = np.empty(max(cap, 1), dtype)
        check(call(buf.ctypes.data_as(C.POINTER(ctype)), cap, C.byref(n)))
        if int(n.value) <= cap:
            return buf[:int(n.value)]
        cap = int(n.value)


def peaks(img, min_peak: float, find_min: bool = False, find_max: bool = True, ij_threads: int = 8,
          route: int = ROUTE_AUTO, device: int | None = None, capacity: int | None = None) -> np.ndarray:
    """InteractiveIntegral.findPeaks over ``img`` ([z, y, x] float32, a numpy array or a GPU
    tensor read in place; not modified): a PEAK_DTYPE record array of the extrema of the
    wanted kinds that are not skipped by ``|v| < min_peak``, in the reference's order.
    ``route``: ROUTE_AUTO, or one of the two candidate kernels.  ``capacity``: the room of
    the first call (default: a sixty-fourth of the voxels); a longer list takes a second call."""
    lib = _lib.load()
    ptr, dims, keep, device = _image(img, device)
    return _capacity(lambda out, cap, n: lib.spim_detect_peaks(ptr, dims, float(min_peak), int(bool(find_min)),
                                                               int(bool(find_max)), int(ij_threads), int(route),
                                                               device, out, cap, n),
                     PEAK_DTYPE, _lib.Peak, _cap(keep, capacity))


def interest_points(img, min_peak: float, localization: int = 0, keep_threshold: float = 0.0,
                    find_min: bool = False, find_max: bool = True, ij_threads: int = 8, route: int = ROUTE_AUTO,
                    device: int | None = None, capacity: int | None = None) -> np.ndarray:
    """``peaks`` after Localization: an IP_DTYPE record array.  ``localization`` 0 copies the
    candidates; 1 fits them and keeps those with ``|fitted value| > keep_threshold`` (float
    against float), in candidate order."""
    lib = _lib.load()
    ptr, dims, keep, device = _image(img, device)
    return _capacity(lambda out, cap, n: lib.spim_detect_interest_points(
        ptr, dims, float(min_peak), int(bool(find_min)), int(bool(find_max)), int(ij_threads), int(route), device,
        int(localization), float(keep_threshold), out, cap, n),
                     IP_DTYPE, _lib.InterestPointC, _cap(keep, capacity))
