"""Test helper: NumPy restatement of the downsampling the reference runs around its bead
detectors (TEST INFRASTRUCTURE ONLY, like ``oracle/`` and ``tests/dom_ref.py``).

    spim/process/interestpointdetection/Downsample.java:65-162            simple2x along one axis
    spim/fiji/plugin/interestpointdetection/DifferenceOf.java:446-535     openAndDownsample (:525-532 the order)
    spim/fiji/plugin/interestpointdetection/DifferenceOf.java:430-444     downsampleFactor
    spim/fiji/plugin/interestpointdetection/DifferenceOf.java:402-428     correctForDownsampling
    spim/fiji/plugin/interestpointdetection/DifferenceOf.java:286-351     limitList

Volumes are [z, y, x] float32; positions (x, y, z) doubles.
"""
from __future__ import annotations

import math

import numpy as np


def simple2x(img, axis: int) -> np.ndarray:
    """Downsample.java:65-162 along numpy axis ``axis``: double arithmetic in Java's
    left-to-right order, one rounding to float (setReal) per output."""
    a = np.moveaxis(np.asarray(img, np.float32), axis, -1).astype(np.float64)
    n = a.shape[-1]
    m = n // 2                                     # :52
    if n < 4:
        raise ValueError("the reference reads and writes out of bounds for a line shorter than 4")
    out = np.empty(a.shape[:-1] + (m,), np.float64)
    with np.errstate(all="ignore"):
        out[..., 0] = (a[..., 0] + a[..., 1] * 0.5) / 1.5                                  # :119-122
        p = np.arange(1, m - 1)                                                            # :125-134
        out[..., 1:m - 1] = (a[..., 2 * p - 1] * 0.5 + a[..., 2 * p] + a[..., 2 * p + 1] * 0.5) / 2.0
        out[..., m - 1] = (a[..., 2 * m - 2] + a[..., 2 * m - 3] * 0.5) / 1.5              # :137-140
        out = out.astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def simple2x_literal(line) -> np.ndarray:
    """The loop of Downsample.java:115-140 on one line, access by access."""
    v = [float(np.float32(x)) for x in line]
    m = len(v) // 2
    size = m - 1
    out = []
    i = 0
    v1 = v[i]
    i += 1
    v0 = v2 = v[i]
    out.append(np.float32((v1 + v2 * 0.5) / 1.5))
    for _ in range(1, size):
        v0 = v2
        i += 1
        v1 = v[i]
        i += 1
        v2 = v[i]
        out.append(np.float32((v0 * 0.5 + v1 + v2 * 0.5) / 2.0))
    i += 1
    v1 = v[i]
    out.append(np.float32((v1 + v2 * 0.5) / 1.5))
    return np.array(out, np.float32)


def levels(f: int) -> int:
    if f not in (1, 2, 4, 8):
        raise ValueError("a factor must be 1, 2, 4 or 8")
    return {1: 0, 2: 1, 4: 2, 8: 3}[f]


def out_dims(shape, xy=1, z=1):
    """(z, y, x) after repeated / 2 (DifferenceOf.java:525-532 over Downsample.java:52)."""
    out = []
    for n, f in zip(shape, (z, xy, xy)):
        for _ in range(levels(f)):
            if n < 4:
                raise ValueError("axis too short")
            n //= 2
        out.append(n)
    return tuple(out)


def downsample(img, xy=1, z=1, fy=None) -> np.ndarray:
    """openAndDownsample's chain (DifferenceOf.java:525-532): every x level, then every y
    level, then every z level, each stored as float.  ``fy``: a y factor other than ``xy``."""
    a = np.ascontiguousarray(img, np.float32)
    for axis, f in ((2, xy), (1, xy if fy is None else fy), (0, z)):
        for _ in range(levels(f)):
            a = simple2x(a, axis)
    return a


def downsample_factor(more: bool, ds_z: int, voxel) -> int:
    """DifferenceOf.java:430-444, unclamped (0 for a z step finer than xy)."""
    cal_xy = min(voxel[0], voxel[1])
    cal_z = voxel[2] * ds_z
    log2ratio = math.log(cal_z / cal_xy) / math.log(2)
    exp2 = math.pow(2, math.ceil(log2ratio) if more else math.floor(log2ratio))
    return int(math.floor(exp2 + 0.5))             # Math.round


def correct_for_downsampling(points, xy=1, z=1) -> np.ndarray:
    """DifferenceOf.java:402-428 with the transform of :521-523 (a pure scale):
    AffineTransform3D.apply, a row of three products and the translation summed in order."""
    m = np.diag([float(xy), float(xy), float(z)])
    out = []
    for p in np.asarray(points, np.float64).reshape(-1, 3):
        out.append([p[0] * m[r, 0] + p[1] * m[r, 1] + p[2] * m[r, 2] + 0.0 for r in range(3)])
    return np.array(out, np.float64).reshape(-1, 3)


def limit_list(points, intensities, max_detections: int, type_index: int):
    """limitList (DifferenceOf.java:286-351) with Collections.sort's stable merge sort and
    the comparator of :306-318; type_index 0 brightest, 1 median, 2 weakest.  Returns the
    kept indices into the given list, in output order."""
    n = len(intensities)
    if n <= max_detections:
        return list(range(n))
    import functools

    def cmp(i, j):
        v1, v2 = abs(float(intensities[i])), abs(float(intensities[j]))
        return 1 if v1 < v2 else 0 if v1 == v2 else -1
    lst = sorted(range(n), key=functools.cmp_to_key(cmp))     # (sorted is stable, as Collections.sort)
    if type_index == 0:
        return [lst[i] for i in range(max_detections)]
    if type_index == 2:
        return [lst[n - 1 - i] for i in range(max_detections)]
    median = n // 2
    return [lst[n - 1 - i] for i in range(median - max_detections // 2, median + max_detections // 2 + 1)]
