"""Host-side mirror of the downsampling the reference runs around its bead detectors.

spim/fiji/plugin/interestpointdetection/DifferenceOf.java: ``openAndDownsample`` (:446-535)
in front of the detector -- every x level, then every y level, then every z level of
``Downsample.simple2x`` (spim/process/interestpointdetection/Downsample.java:65-162), each
level a float image; ``correctForDownsampling`` (:402-428) behind it; ``limitList``
(:286-351), the "Maximum_number of detections" option; ``downsampleFactor`` (:430-444), the
"Match Z Resolution" choices of "Downsample_XY".  The image runs on the GPU in
``spim_downsample`` (bit-exact against the reference's arithmetic); the rest is host
arithmetic on the detections.  Not restated: ``preSmooth`` and the multi-resolution loader.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

__all__ = ["out_dims", "downsample", "downsample_factor", "correct_for_downsampling", "limit_detections",
           "FACTORS", "LIMIT_KINDS"]

FACTORS = (1, 2, 4, 8)                                   # DifferenceOf.java:46 (ds)
LIMIT_KINDS = {"brightest": 0, "median": 1, "weakest": 2}   # limitDetectionChoice, :48


def _factor(xy, z):
    return (C.c_int32 * 3)(int(xy), int(xy), int(z))


def out_dims(shape, xy: int = 1, z: int = 1):
    """The downsampled shape (z, y, x) of a (z, y, x) shape: each axis halved (integer
    division) once per level.  ValueError for a factor outside 1, 2, 4, 8 or an axis shorter
    than 4 at one of its levels.  Needs no GPU."""
    if len(shape) != 3:
        raise ValueError("shape must be (z, y, x)")
    dims = (C.c_int64 * 3)(int(shape[2]), int(shape[1]), int(shape[0]))
    od = (C.c_int64 * 3)()
    lib = _lib.load()
    if lib.spim_downsample_dims(dims, _factor(xy, z), od) != 0:
        raise ValueError(_lib.last_error())
    return int(od[2]), int(od[1]), int(od[0])


def downsample(img, xy: int = 1, z: int = 1, device: int | None = None):
    """openAndDownsample's image: ``img`` ([z, y, x] float32, not modified) downsampled ``xy``
    times in x and y and ``z`` times in z (each 1, 2, 4 or 8).  A numpy array gives a numpy
    array; a torch tensor on the GPU is read in place and gives a tensor on its GPU.
    ``device``: the GPU that runs the pass; default the tensor's own (0 for a host array)."""
    lib = _lib.load()
    on_dev = hasattr(img, "is_cuda") and img.is_cuda
    if device is None:
        device = img.device.index if on_dev else 0
    if on_dev:
        import torch
        img = img.contiguous().float()
        if img.dim() != 3:
            raise ValueError("img must be 3D [z, y, x]")
        shape = out_dims(tuple(img.shape), xy, z)
        torch.cuda.synchronize(img.device)   # the library runs on its own stream
        out = torch.empty(shape, dtype=torch.float32, device=img.device)
        iptr, optr = img.data_ptr(), out.data_ptr()
    else:
        img = np.ascontiguousarray(img, np.float32)
        if img.ndim != 3:
            raise ValueError("img must be 3D [z, y, x]")
        shape = out_dims(img.shape, xy, z)
        out = np.empty(shape, np.float32)
        iptr, optr = img.ctypes.data, out.ctypes.data
    dims = (C.c_int64 * 3)(img.shape[2], img.shape[1], img.shape[0])
    check(lib.spim_downsample(C.c_void_p(iptr), dims, _factor(xy, z), int(device), C.c_void_p(optr)))
    return out


def downsample_factor(choice, ds_z: int = 1, voxel_size=None) -> int:
    """The xy factor of the "Downsample_XY" choice: an int is itself (1, 2, 4 or 8);
    'match_z_less' / 'match_z_more' are "Match Z Resolution (less / more downsampling)",
    downsampleFactor over ``voxel_size`` (x, y, z) and the z factor ``ds_z``.  Below 1 (a z
    step finer than xy, where the reference would scale every coordinate by 0) is 1; above 8
    raises ValueError."""
    if isinstance(choice, str):
        if choice not in ("match_z_less", "match_z_more"):
            raise ValueError(f"downsample choice must be an int, 'match_z_less' or 'match_z_more', not {choice!r}")
        if voxel_size is None or len(voxel_size) != 3:
            raise ValueError("matching the z resolution needs voxel_size (x, y, z)")
        lib = _lib.load()
        v = (C.c_double * 3)(*(float(s) for s in voxel_size))
        f = C.c_int32(0)
        if lib.spim_downsample_factor_xy(int(choice == "match_z_more"), int(ds_z), v, C.byref(f)) != 0:
            raise ValueError(_lib.last_error())
        return int(f.value)
    if int(choice) != choice or int(choice) not in FACTORS:
        raise ValueError(f"a downsampling factor must be 1, 2, 4 or 8, not {choice!r}")
    return int(choice)


def correct_for_downsampling(points, xy: int = 1, z: int = 1) -> np.ndarray:
    """correctForDownsampling: (n, 3) positions (x, y, z) of the downsampled view in pixels
    of the full view -- AffineTransform3D.apply of diag(xy, xy, z) with its zero terms, in
    double (output voxel p is centred on input voxel factor * p: no translation)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    x, y, zz = p[:, 0], p[:, 1], p[:, 2]
    fx, fz = float(xy), float(z)
    return np.stack([x * fx + y * 0.0 + zz * 0.0 + 0.0,
                     x * 0.0 + y * fx + zz * 0.0 + 0.0,
                     x * 0.0 + y * 0.0 + zz * fz + 0.0], axis=1)


def limit_detections(points, intensities, max_detections: int, kind: str = "brightest"):
    """limitList: (points, intensities) cut to the "Maximum_number of detections".  A list
    not longer than the limit is returned unchanged; otherwise it is stably sorted by
    |intensity| descending and 'brightest' takes the first ``max_detections``, 'weakest' the
    last ones starting from the end, 'median' the inclusive range median +- max / 2 (integer
    divisions) indexed from the end -- max + 1 entries for an even limit, as written."""
    if kind not in LIMIT_KINDS:
        raise ValueError(f"kind must be 'brightest', 'median' or 'weakest', not {kind!r}")
    pts = np.asarray(points)
    inten = np.asarray(intensities)
    n, mx = len(inten), int(max_detections)
    if mx < 0 or len(pts) != n:
        raise ValueError("max_detections must be >= 0 and points, intensities of one length")
    if n <= mx:
        return pts, inten
    order = np.argsort(-np.abs(inten.astype(np.float64)), kind="stable")
    if kind == "brightest":
        sel = order[:mx]
    elif kind == "weakest":
        sel = order[n - 1 - np.arange(mx)]
    else:
        median = n // 2
        sel = order[n - 1 - np.arange(median - mx // 2, median + mx // 2 + 1)]
    return pts[sel], inten[sel]
