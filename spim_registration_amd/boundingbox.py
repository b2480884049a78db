"""The fusion bounding box estimated from the data: the reference's "Estimate automatically
(experimental)" beside "Define manually" and "BigDataViewer".

spim/process/fusion/boundingbox/AutomaticBoundingBox.java:36-131 and
automatic/MinFilterThreshold.java:76-308: the maximal box of all views is fused at a
downsampling (nearest neighbour, no blending), a threshold is put at ``background`` percent of
the fused image's range, a separable minimum filter of radius
``discarded_object_size / 2 / downsampling`` erodes beads and debris, and the box of what is
still above the threshold is scaled back and padded by ``3 * (discarded_object_size / 2)``.
The fused image never leaves the GPU; every image-sized step is a kernel of
``csrc/autobbox.hip`` and bit-exact against the reference's arithmetic (Math.min / Math.max:
a NaN spreads, -0 < +0).  Not restated: "Load input images sequentially" (ProcessSequential's
float accumulation).

"Automatically reorientate and estimate based on sample features"
(boundingbox/AutomaticReorientation.java) takes the box from the interest points instead:
``reorient_bounding_box`` finds the rotation under which the detections' axis-aligned box is
smallest (the farthest pair over all pairs, then a search over 8 x 27 axes; ``csrc/reorient.hip``,
all double and bit-exact against the reference's arithmetic) and returns it with the models it
is preconcatenated to and the padded box.

Images are [z, y, x] float32, numpy arrays or torch tensors on the GPU (read in place; image
results come back as what went in); boxes, dims and positions are (x, y, z).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

__all__ = ["max_bounding_box", "min_max", "min_filter", "min_filter_tiles", "threshold_bounds", "segment_bounds",
           "auto_bounding_box", "release_workspace", "MAX_RADIUS", "farthest_pair", "axis_boxes",
           "points_min_max", "preconcatenate", "reorient_bounding_box", "reorient_tile",
           "release_reorient_workspace"]

MAX_RADIUS = 64      # SPIM_MIN_FILTER_MAX_RADIUS


def _on_gpu(a) -> bool:
    return hasattr(a, "is_cuda") and a.is_cuda


def _image(img, device):
    """(the image kept alive, its address, dims (x, y, z), device, on_gpu)"""
    if _on_gpu(img):
        import torch
        img = img.contiguous().float()
        if img.dim() != 3:
            raise ValueError("img must be 3D [z, y, x]")
        torch.cuda.synchronize(img.device)   # the library runs on its own stream
        dev = img.device.index or 0 if device is None else int(device)
        return img, img.data_ptr(), (C.c_int64 * 3)(img.shape[2], img.shape[1], img.shape[0]), dev, True
    img = np.ascontiguousarray(img, np.float32)
    if img.ndim != 3:
        raise ValueError("img must be 3D [z, y, x]")
    dims = (C.c_int64 * 3)(img.shape[2], img.shape[1], img.shape[0])
    return img, img.ctypes.data, dims, 0 if device is None else int(device), False


def _like(img, on_gpu):
    if on_gpu:
        import torch
        out = torch.empty_like(img)
        return out, out.data_ptr()
    out = np.empty_like(img)
    return out, out.ctypes.data


def max_bounding_box(dims, models, downsampling: int = 1):
    """The maximal box that holds all views (computeMaxBoundingBoxDimensions, rounded as
    AutomaticBoundingBox does): ``dims`` per view (x, y, z), ``models`` per view 3x4 (view ->
    world).  Returns (bb_min, bb_max, bb_dims, fused_dims), tuples of ints; fused_dims =
    bb_dims // downsampling.  Needs no GPU."""
    lib = _lib.load()
    d = np.ascontiguousarray(np.asarray(dims, np.int64).reshape(-1, 3))
    m = np.ascontiguousarray(np.asarray(models, np.float64).reshape(-1, 12))
    if len(d) < 1 or len(d) != len(m):
        raise ValueError("need one model per view")
    out = [(C.c_int64 * 3)() for _ in range(4)]
    if lib.spim_max_bounding_box(len(d), d.ctypes.data_as(_lib._pi64), m.ctypes.data_as(_lib._pd),
                                 int(downsampling), *out) != 0:
        raise ValueError(_lib.last_error())
    return tuple(tuple(int(x) for x in o) for o in out)


def min_max(img, device: int | None = None):
    """FusionHelper.minMax: (min, max) as numpy float32, Math.min / Math.max from
    +-Float.MAX_VALUE (a NaN voxel makes both NaN)."""
    lib = _lib.load()
    img, ptr, dims, dev, _ = _image(img, device)
    mn, mx = C.c_float(), C.c_float()
    check(lib.spim_min_max(C.c_void_p(ptr), dims, dev, C.byref(mn), C.byref(mx)))
    return np.float32(mn.value), np.float32(mx.value)


def min_filter(img, radius: int, device: int | None = None, out=None):
    """computeLazyMinFilter: the minimum over 2 * radius + 1 voxels along x, then y, then z, over a
    zero extension.  radius 1 .. MAX_RADIUS.  ``out``: where the result goes (same kind and
    shape as ``img``; ``img`` itself filters in place); default a new image."""
    lib = _lib.load()
    img, ptr, dims, dev, on_gpu = _image(img, device)
    if out is None:
        out, optr = _like(img, on_gpu)
    else:
        if _on_gpu(out) != on_gpu or tuple(out.shape) != tuple(img.shape):
            raise ValueError("out must be of img's kind and shape")
        if on_gpu:
            if not out.is_contiguous() or str(out.dtype) != "torch.float32":
                raise ValueError("out must be a contiguous float32 tensor")
            optr = out.data_ptr()
        else:
            if out.dtype != np.float32 or not out.flags.c_contiguous:
                raise ValueError("out must be a contiguous float32 array")
            optr = out.ctypes.data
    check(lib.spim_min_filter(C.c_void_p(ptr), dims, int(radius), dev, C.c_void_p(optr)))
    return out


def min_filter_tiles():
    """(lines per block, outputs per line and block along the pass axis for a small radius, the
    same for a large one, the largest small radius, threads per reduction block, reduction
    blocks) of the minimum filter and min / max kernels.  Needs no GPU."""
    sizes = (C.c_int32 * 6)()
    _lib.load().spim_min_filter_tiles(sizes)
    return tuple(int(s) for s in sizes)


def threshold_bounds(img, threshold: float, device: int | None = None):
    """computeBoundingBox: (bounds_min, bounds_max, found) of the voxels with double(v) >
    threshold, (x, y, z).  Nothing above it: found False and the reference's integers
    (bounds_min = dims, bounds_max = 0)."""
    lib = _lib.load()
    img, ptr, dims, dev, _ = _image(img, device)
    lo, hi, found = (C.c_int64 * 3)(), (C.c_int64 * 3)(), C.c_int32()
    check(lib.spim_threshold_bounds(C.c_void_p(ptr), dims, float(threshold), dev, lo, hi, C.byref(found)))
    return tuple(int(x) for x in lo), tuple(int(x) for x in hi), bool(found.value)


def _segment_dict(r) -> dict:
    return {"min": np.float32(r.min), "max": np.float32(r.max), "threshold": float(r.threshold),
            "bounds_min": tuple(int(x) for x in r.bounds_min), "bounds_max": tuple(int(x) for x in r.bounds_max),
            "found": bool(r.found)}


def segment_bounds(img, background: float = 5.0, radius: int = 1, device: int | None = None,
                   return_filtered: bool = False):
    """min / max -> threshold at ``background`` percent of the range -> min_filter -> box, in one
    call.  Returns a dict (min, max, threshold, bounds_min, bounds_max, found); with
    ``return_filtered`` also "filtered", the image the box was taken from -- without it the
    filter's last pass writes no image."""
    lib = _lib.load()
    img, ptr, dims, dev, on_gpu = _image(img, device)
    filt, fptr_ = _like(img, on_gpu) if return_filtered else (None, None)
    res = _lib.SegmentResult()
    check(lib.spim_segment_bounds(C.c_void_p(ptr), dims, float(background), int(radius), dev, C.c_void_p(fptr_),
                                  C.byref(res)))
    d = _segment_dict(res)
    if return_filtered:
        d["filtered"] = filt
    return d


def auto_bounding_box(views, models, background: float = 5.0, discarded_object_size: int = 25,
                      downsampling: int = 4, device: int = 0, return_details: bool = False):
    """The estimated bounding box of ``views`` (numpy arrays, or torch tensors on the GPU) under
    ``models`` (3x4, view -> world): (bb_min, bb_dims), (x, y, z) tuples ready for
    ``prepare_inputs`` / ``fuse_weighted_average`` / ``process_timepoint``.  Defaults are the
    dialog's (5 %, 25, 4).  ValueError when nothing lies above the threshold (the reference
    goes on with an inverted box).  ``return_details``: (bb_min, bb_dims, details) instead, with
    found, bb_max, the maximal box, the fused dims, radius_min, eff_radius and the fused image's
    min, max, threshold, bounds_min, bounds_max -- and no exception for found False."""
    lib = _lib.load()
    V = len(views)
    if V < 1 or len(models) != V:
        raise ValueError("need one model per view")
    on_gpu = all(_on_gpu(v) for v in views)
    if on_gpu:
        import torch
        views = [v.contiguous().float() for v in views]
        torch.cuda.synchronize(views[0].device)   # the library runs on its own stream
    else:
        views = [np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v, np.float32) for v in views]
    vs = (_lib.ViewSource * V)()
    for i, (v, m) in enumerate(zip(views, models)):
        if len(v.shape) != 3:
            raise ValueError("views must be 3D [z, y, x]")
        vs[i].img = C.cast(C.c_void_p(v.data_ptr() if on_gpu else v.ctypes.data), _lib._pf)
        vs[i].dims[:] = [v.shape[2], v.shape[1], v.shape[0]]
        vs[i].model[:] = [float(x) for x in np.asarray(m, np.float64).reshape(12)]
    p = _lib.AutoBBoxParams()
    lib.spim_autobbox_params_default(C.byref(p))
    p.background = float(background)
    p.discarded_object_size = int(discarded_object_size)
    p.downsampling = int(downsampling)
    p.device = int(device)
    p.src_on_device = int(on_gpu)
    r = _lib.AutoBBoxResult()
    check(lib.spim_auto_bounding_box(V, vs, C.byref(p), C.byref(r)))
    t = lambda a: tuple(int(x) for x in a)
    bb_min, bb_dims = t(r.bb_min), t(r.bb_dims)
    if return_details:
        return bb_min, bb_dims, {"bb_max": t(r.bb_max), "max_min": t(r.max_min), "max_max": t(r.max_max),
                                 "max_dims": t(r.max_dims), "fused_dims": t(r.fused_dims),
                                 "radius_min": int(r.radius_min), "eff_radius": int(r.eff_radius),
                                 **_segment_dict(r.seg)}
    if not r.found:
        raise ValueError(f"automatic bounding box: no voxel of the fused image (min {r.seg.min}, max {r.seg.max}) "
                         f"stays above the threshold {r.seg.threshold} after the minimum filter of radius "
                         f"{r.eff_radius}")
    return bb_min, bb_dims


def release_workspace(device: int = 0) -> None:
    """Frees the device's scratch volumes of this module (the next call allocates them again)."""
    check(_lib.load().spim_bbox_release_workspace(int(device)))


# ---------------------------------------------------------------- the box from the interest points
def _points(x):
    """(pointer, n, the object that owns the memory) of an (n, 3) double array: a numpy array
    or a CUDA torch tensor (read in place)."""
    if _on_gpu(x):
        import torch
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError("points must be (n, 3)")
        x = x.contiguous().double()
        torch.cuda.synchronize(x.device)   # the library runs on its own stream
        return C.c_void_p(x.data_ptr()), int(x.shape[0]), x
    a = np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, 3))
    return C.c_void_p(a.ctypes.data), len(a), a


def reorient_tile() -> int:
    """Row points per block = column points per LDS tile of the farthest-pair kernel."""
    t = C.c_int32(0)
    _lib.load().spim_reorient_tile(C.byref(t))
    return int(t.value)


def farthest_pair(points, device: int = 0):
    """AutomaticReorientation.determineOptimalBoundingBox :316-343 over (n, 3) points (a numpy
    array or a CUDA torch tensor): (i, j, d2), the indices of the reference's p1 and p2 and
    their squared distance.  Among the pairs at the largest distance the first in (i, j) scan
    order wins; it is ordered so that p1.x <= p2.x unless it is the start pair (0, 1)."""
    lib = _lib.load()
    ptr, n, _keep = _points(points)
    i, j, d2 = C.c_int32(-1), C.c_int32(-1), C.c_double(0.0)
    check(lib.spim_farthest_pair(ptr, n, int(device), C.byref(i), C.byref(j), C.byref(d2)))
    return int(i.value), int(j.value), float(d2.value)


def axis_boxes(points, matrices, device: int = 0):
    """testAxis :429-442 under up to 27 transforms at once: ``matrices`` (m, 3, 4); returns
    (m, 6) float64, per matrix min x, y, z, max x, y, z of the transformed points by Math.min /
    Math.max (a matrix of NaNs gives NaNs for that matrix only)."""
    lib = _lib.load()
    ptr, n, _keep = _points(points)
    mats = np.ascontiguousarray(np.asarray(matrices, np.float64).reshape(-1, 12))
    out = np.empty((len(mats), 6), np.float64)
    check(lib.spim_axis_boxes(ptr, n, mats.ctypes.data_as(_lib._pd), len(mats), int(device),
                              out.ctypes.data_as(_lib._pd)))
    return out


def points_min_max(points, device: int = 0):
    """determineSizeSimple :488-512: (6,) float64, min x, y, z, max x, y, z of the points."""
    lib = _lib.load()
    ptr, n, _keep = _points(points)
    out = np.empty(6, np.float64)
    check(lib.spim_points_min_max(ptr, n, int(device), out.ctypes.data_as(_lib._pd)))
    return out


def preconcatenate(transform, model):
    """transform o model, both 3x4: what ``ViewRegistration.preconcatenateTransform`` leaves as
    the view's model.  Every element is the left-to-right sum t0 * m0 + t1 * m1 + t2 * m2 (+ t3
    in the last column)."""
    t = np.asarray(transform, np.float64).reshape(3, 4)
    m = np.asarray(model, np.float64).reshape(3, 4)
    out = np.empty((3, 4))
    for r in range(3):
        for c in range(4):
            s = t[r, 0] * m[0, c] + t[r, 1] * m[1, c] + t[r, 2] * m[2, c]
            out[r, c] = s + t[r, 3] if c == 3 else s
    return out


def reorient_bounding_box(points, models, corresponding=None, percent: float = 10.0, reorientate: bool = True,
                          device: int = 0, return_details: bool = False, far_split: int = 0):
    """"Automatically reorientate and estimate based on sample features"
    (AutomaticReorientation.java): ``points`` per view (n, 3) detections in view pixels (numpy
    arrays or CUDA torch tensors), ``models`` per view 3x4 (view -> world); ``corresponding``:
    per view the indices of the detections to use (the dialog's "only corresponding
    detections"), None = all.  The world points' axis-aligned box has minimal volume under the
    rotation returned; it is padded by ``percent`` of its largest extent (half on each side).
    Returns (transform, new_models, bb_min, bb_dims): the 3x4 rotation, ``new_models[v] =
    transform o models[v]`` (``preconcatenate``) and the box, (x, y, z) tuples ready for
    ``prepare_inputs`` / ``process_timepoint`` with the new models.  ``reorientate=False``: the
    identity and the plain min / max of the world points.  ``return_details``: a fifth value, a
    dict with min_f, max_f, bb_max, n_points, far_pair (i, j into the concatenated world points),
    far_d2, start_volume, min_volume and axis.  Fewer than two points (one without reorientate)
    are an error.  ``far_split`` forces the farthest-pair kernel's column partitions (0 = auto;
    the result does not depend on it)."""
    lib = _lib.load()
    V = len(points)
    if V < 1 or len(models) != V or (corresponding is not None and len(corresponding) != V):
        raise ValueError("need one model (and one index list) per view")
    staged = [_points(p) for p in points]
    lists = (C.c_void_p * V)(*[s[0] for s in staged])
    counts = (C.c_int64 * V)(*[s[1] for s in staged])
    m = np.ascontiguousarray(np.stack([np.asarray(x, np.float64).reshape(12) for x in models]))
    corr = cc = None
    if corresponding is not None:
        idx = [np.ascontiguousarray(np.asarray(c.cpu() if hasattr(c, "cpu") else c).reshape(-1), np.int64)
               for c in corresponding]
        corr = (C.c_void_p * V)(*[C.c_void_p(i.ctypes.data) for i in idx])
        cc = (C.c_int64 * V)(*[len(i) for i in idx])
    p = _lib.ReorientParams()
    lib.spim_reorient_params_default(C.byref(p))
    p.use_corresponding = int(corresponding is not None)
    p.reorientate = int(bool(reorientate))
    p.percent = float(percent)
    p.device = int(device)
    p.far_split = int(far_split)
    r = _lib.ReorientResult()
    check(lib.spim_reorient_bounding_box(V, lists, counts, corr, cc, m.ctypes.data_as(_lib._pd), C.byref(p),
                                         C.byref(r)))
    transform = np.array(r.transform[:], np.float64).reshape(3, 4)
    new_models = [preconcatenate(transform, x) for x in models]
    t = lambda a: tuple(int(x) for x in a)
    out = (transform, new_models, t(r.bb_min), t(r.bb_dims))
    if return_details:
        out += ({"min_f": np.array(r.min_f[:]), "max_f": np.array(r.max_f[:]), "bb_max": t(r.bb_max),
                 "n_points": int(r.n_points), "far_pair": (int(r.far_i), int(r.far_j)), "far_d2": float(r.far_d2),
                 "start_volume": float(r.start_volume), "min_volume": float(r.min_volume),
                 "axis": np.array(r.axis[:])},)
    return out


def release_reorient_workspace(device: int = 0) -> None:
    """Frees the device's scratch of the interest-point box (the next call allocates it again)."""
    check(_lib.load().spim_reorient_release_workspace(int(device)))
