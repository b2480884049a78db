"""Thin out detections by the distance to their nearest neighbour, on the GPU.

The reference's "Thin out detections" step (spim/fiji/plugin/ThinOut_Detections.java:73-166,
:238-299; spim/fiji/plugin/thinout/Histogram.java:56-90), which users of sample-feature
registration run between detection and registration: per detection of a view the distance to its
nearest other detection in calibrated units (``l[d] * voxel_size[d]``), a 100-bin histogram of
those distances to pick a range from, and a new list without -- or with only -- the detections
whose distance lies in ``[min_distance, max_distance]``.  It strips the dense clutter (clumps
of nuclei, debris, doubled detections of one bead) that slows the descriptor matchers and makes
their RANSAC fragile.

Beside the four user calls (``nn_distances``, ``thin_out``, ``distance_histogram``,
``tile_sizes``) the module exports their pieces -- ``histogram`` (one
``spim_distance_histogram`` call over given distances), ``subsampling_mask`` (the draw) and
``check_range`` (the dialog's min < max rule, shared with the pipeline) -- for the tests and the
pipeline.

``nn_distances`` / ``thin_out`` / ``distance_histogram`` run ``spim_nn_distances`` /
``spim_thin_out`` / ``spim_distance_histogram`` (csrc/thinout.hip): an all-pairs self-join in
double, bit-exact against the reference's arithmetic; there is no CPU path.

Stated deviations and unpinned points:

  * The reference searches with imglib2's ``KDTree`` / ``KNearestNeighborSearchOnKDTree``, whose
    jar is not in its tree: the squared distance as the sum over x, y, z from left to right and
    ``Math.sqrt`` of it are restated, not pinned; among equal sums the lower index is the nearest.
  * Its result for a list of one point is unknown; here the distance is ``+inf`` and the nearest
    ``-1``: kept by remove-range, dropped by keep-range.  Such a distance cannot be binned:
    ``distance_histogram`` leaves views of fewer than two points out of the pool.
  * The histogram's subsampling: the reference seeds ``java.util.Random`` with the clock, so its
    draw cannot be reproduced; here the mask is ``numpy.random.default_rng(seed).random(n) <
    1.0 / subsampling`` over the pooled list.
  * The parameter string of the new list (:147-150) is not produced; the thinned list is
    written with the existing ``.ip.txt`` writer.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .registration import _points, _tiles

__all__ = ["nn_distances", "thin_out", "distance_histogram", "histogram", "tile_sizes", "subsampling_mask",
           "check_range"]


def tile_sizes():
    """(points per block, points per LDS tile) of the self-join kernel."""
    return _tiles(_lib.load().spim_thinout_tiles)


def check_range(min_distance, max_distance):
    """ThinOut_Detections.java:220-225: the lower threshold must be below the upper one."""
    if not float(min_distance) < float(max_distance):
        raise ValueError(f"thin out: min_distance ({min_distance}) must be smaller than max_distance "
                         f"({max_distance})")


def _params(lib, min_distance, max_distance, keep_range, device, t_split=0):
    p = _lib.ThinOutParams()
    lib.spim_thinout_params_default(C.byref(p))
    p.min_distance, p.max_distance = float(min_distance), float(max_distance)
    p.keep_range, p.t_split, p.device = int(bool(keep_range)), int(t_split), int(device)
    return p


def _voxel(voxel_size):
    v = np.ascontiguousarray(np.asarray(voxel_size, np.float64).reshape(-1))
    if v.shape != (3,):
        raise ValueError("voxel_size must be (x, y, z)")
    return v


def _count(points) -> int:
    if hasattr(points, "is_cuda"):
        return int(points.shape[0])
    return len(np.asarray(points, np.float64).reshape(-1, 3))


def nn_distances(points, voxel_size=(1.0, 1.0, 1.0), device: int = 0, t_split: int = 0):
    """Per point of the (n, 3) list (a numpy array or a CUDA torch tensor, x, y, z in pixels)
    the distance to its nearest other point after scaling by ``voxel_size``: (dist float64,
    nearest int32).  An exact duplicate is a neighbour at distance 0; one point alone has
    (+inf, -1).  ``t_split`` is for the tests: it forces the partitions of the list (0 = auto, what
    every other caller wants; the result does not depend on it)."""
    lib = _lib.load()
    p = _params(lib, 0.0, 5.0, False, device, t_split)
    v = _voxel(voxel_size)
    ptr, n, _keep = _points(points)
    dist, nearest = np.empty(n, np.float64), np.empty(n, np.int32)
    check(lib.spim_nn_distances(ptr, n, v.ctypes.data_as(_lib._pd), C.byref(p), C.c_void_p(dist.ctypes.data),
                                C.c_void_p(nearest.ctypes.data)))
    return dist, nearest


def thin_out(points, voxel_size=(1.0, 1.0, 1.0), min_distance: float = 0.0, max_distance: float = 5.0,
             keep_range: bool = False, device: int = 0, return_all: bool = False, t_split: int = 0):
    """ThinOut_Detections.thinOut over one view's (n, 3) detections (a numpy array or a CUDA
    torch tensor): ``points[kept]`` -- the original, unscaled coordinates, copied, in list
    order (row k is the detection with the new id k) --, where ``kept`` are the points whose
    nearest-neighbour distance d is outside ``[min_distance, max_distance]`` (d < min or d >
    max) or, with ``keep_range``, inside it (min <= d <= max).  With ``return_all`` also kept
    (int32), dist (float64) and nearest (int32) over every point.  ``t_split`` is for the tests, as
    in ``nn_distances``."""
    lib = _lib.load()
    p = _params(lib, min_distance, max_distance, keep_range, device, t_split)
    v = _voxel(voxel_size)
    ptr, n, owner = _points(points)
    dist, nearest = np.empty(n, np.float64), np.empty(n, np.int32)
    kept = np.empty(max(n, 1), np.int32)
    count = C.c_int64(0)
    check(lib.spim_thin_out(ptr, n, v.ctypes.data_as(_lib._pd), C.byref(p), C.c_void_p(dist.ctypes.data),
                            C.c_void_p(nearest.ctypes.data), C.c_void_p(kept.ctypes.data), n, C.byref(count)))
    kept = kept[:count.value].copy()
    if isinstance(owner, np.ndarray):
        out = owner[kept].copy()
    else:
        import torch
        out = owner[torch.from_numpy(kept.astype(np.int64)).to(owner.device)].clone()
    return (out, kept, dist, nearest) if return_all else out


def histogram(dist, select=None, bins: int = 100, device: int = 0):
    """Histogram.getMinMax and binData over the distances (those with a non-zero ``select``):
    (centres float64 (bins,), counts int64 (bins,), min, max)."""
    lib = _lib.load()
    d = np.ascontiguousarray(np.asarray(dist, np.float64).reshape(-1))
    sel = None
    if select is not None:
        sel = np.ascontiguousarray(np.asarray(select).reshape(-1) != 0).astype(np.uint8)
        if sel.shape != d.shape:
            raise ValueError("select must have one entry per distance")
    nb = max(int(bins), 0)
    counts, centres = np.zeros(nb, np.int64), np.zeros(nb, np.float64)
    lo, hi = C.c_double(0.0), C.c_double(0.0)
    check(lib.spim_distance_histogram(C.c_void_p(d.ctypes.data), len(d),
                                      None if sel is None else C.c_void_p(sel.ctypes.data), int(bins), int(device),
                                      C.byref(lo), C.byref(hi), counts.ctypes.data_as(_lib._pi64),
                                      centres.ctypes.data_as(_lib._pd)))
    return centres, counts, float(lo.value), float(hi.value)


def subsampling_mask(n: int, subsampling: int, seed=None):
    """the selection of ``distance_histogram``: None for subsampling 1, else the 0/1 mask
    ``default_rng(seed).random(n) < 1.0 / subsampling`` (:285, with NumPy's generator)"""
    if int(subsampling) < 1:
        raise ValueError("subsampling must be >= 1")
    if int(subsampling) == 1:
        return None
    return (np.random.default_rng(seed).random(int(n)) < 1.0 / float(int(subsampling))).astype(np.uint8)


def distance_histogram(points_per_view, voxel_sizes, bins: int = 100, subsampling: int = 1, seed=None,
                       device: int = 0):
    """ThinOut_Detections.plotHistogram over the views of a channel: the nearest-neighbour
    distances of every view (``nn_distances`` under its own voxel size; ``voxel_sizes`` is one
    (x, y, z) per view, or one for all) pooled in view order, every point -- or with
    ``subsampling`` n > 1 about every n-th, drawn by ``subsampling_mask`` -- binned as
    ``Histogram`` does.  Returns (centres, counts, min, max).  Views of fewer than two points
    have no finite distance and are left out."""
    if int(bins) <= 0:
        raise ValueError("bins must be >= 1")
    views = list(points_per_view)
    vs = np.asarray(voxel_sizes, np.float64)
    vs = np.broadcast_to(vs, (len(views), 3)) if vs.ndim == 1 else vs
    if vs.shape != (len(views), 3):
        raise ValueError("voxel_sizes must be (x, y, z) or one (x, y, z) per view")
    mask_len = sum(_count(p) for p in views)
    mask = subsampling_mask(mask_len, subsampling, seed)
    dists, sels, o = [], [], 0
    for p, v in zip(views, vs):
        n = _count(p)
        if n >= 2:
            dists.append(nn_distances(p, v, device)[0])
            if mask is not None:
                sels.append(mask[o:o + n])
        o += n
    pooled = np.concatenate(dists) if dists else np.zeros(0)
    return histogram(pooled, np.concatenate(sels) if mask is not None and sels else None, bins, device)
