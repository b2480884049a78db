"""Host-side mirror of the Difference-of-Mean bead-detection pass (ProcessDOM.compute).

spim/process/interestpointdetection/ProcessDOM.java:36-117 over
mpicbg/spim/segmentation/DOM.java:29-171 and IntegralImage3d.java:60-210: the mean of a
small box minus the mean of a larger one around every voxel (integer sums, two float
divisions), then the peak test and Localization of the DoG detector.  The whole pass runs
on the GPU in ``spim_dom_interest_points``; the image is bit-exact against the reference's
arithmetic (the integral image it uses is a device of the reference, not of the result).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, fptr
from .dog import IP_DTYPE, InterestPoint

__all__ = ["compute", "interest_points_array", "simple_peaks", "box_diameters", "InterestPoint", "IP_DTYPE"]


def _params(lib, radius1, radius2, threshold, localization, image_sigma, find_min, find_max, min_intensity,
            max_intensity, device, ij_threads):
    p = _lib.DomParams()
    lib.spim_dom_params_default(C.byref(p))
    p.radius1, p.radius2 = int(radius1), int(radius2)
    p.threshold, p.localization = float(threshold), int(localization)
    for d in range(3):
        p.image_sigma[d] = float(image_sigma[d])
    p.find_min, p.find_max = int(bool(find_min)), int(bool(find_max))
    p.min_intensity, p.max_intensity = float(min_intensity), float(max_intensity)
    p.ij_threads, p.device = int(ij_threads), int(device)
    return p


def box_diameters(radius1: int = 2, radius2: int = 3, image_sigma=(0.5, 0.5, 0.5)):
    """ProcessDOM.java:71-78: ((s1x, s1y, s1z), (s2x, s2y, s2z)), the box diameters per
    axis -- max(3 | 5, round(radius * 0.5 / image_sigma) * 2 + 1).  Needs no GPU."""
    lib = _lib.load()
    p = _params(lib, radius1, radius2, 0.02, 0, image_sigma, False, True, float("nan"), float("nan"), 0, 8)
    s1, s2 = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    check(lib.spim_dom_diameters(C.byref(p), s1, s2))
    return tuple(s1), tuple(s2)


def _points(lib, iptr, shape, size, p, dptr, cap):
    """spim_dom_interest_points with the capacity rule: a numpy IP_DTYPE record array."""
    dims = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
    n = C.c_int64(0)
    while True:
        buf = np.empty(cap, IP_DTYPE)
        check(lib.spim_dom_interest_points(iptr, dims, C.byref(p), dptr,
                                           buf.ctypes.data_as(C.POINTER(_lib.InterestPointC)), cap, C.byref(n)))
        if int(n.value) <= cap:
            return buf[:int(n.value)]
        cap = int(n.value)   # rerun with the exact capacity


def _run(img, p, return_dom, device):
    """(records, DOM image or None) for a numpy array or a GPU tensor."""
    lib = _lib.load()
    fp = C.POINTER(C.c_float)
    if hasattr(img, "is_cuda") and img.is_cuda:
        import torch
        img = img.contiguous().float()
        if img.dim() != 3:
            raise ValueError("img must be 3D [z, y, x]")
        torch.cuda.synchronize(img.device)   # the library runs on its own stream
        dom = torch.empty_like(img) if return_dom else None
        dptr = C.cast(C.c_void_p(dom.data_ptr()), fp) if dom is not None else None
        rec = _points(lib, C.cast(C.c_void_p(img.data_ptr()), fp), img.shape, img.numel(), p, dptr,
                      max(1 << 16, img.numel() // 512))
        return rec, dom
    img = np.ascontiguousarray(img, np.float32)
    if img.ndim != 3:
        raise ValueError("img must be 3D [z, y, x]")
    dom = np.empty_like(img) if return_dom else None
    rec = _points(lib, fptr(img), img.shape, img.size, p, fptr(dom) if dom is not None else None,
                  max(1024, img.size // 64))
    return rec, dom


def compute(img, radius1: int = 2, radius2: int = 3, threshold: float = 0.02, localization: int = 0,
            image_sigma=(0.5, 0.5, 0.5), find_min: bool = False, find_max: bool = True,
            min_intensity: float = float("nan"), max_intensity: float = float("nan"),
            keep_intensity: bool = False, device: int | None = None, ij_threads: int = 8,
            return_dom: bool = False, max_peaks: int | None = None, downsample_xy: int = 1,
            downsample_z: int = 1):
    """ProcessDOM.compute: returns the list of InterestPoint (and the DOM image when
    ``return_dom``).  ``img`` is a [z, y, x] float32 volume (not modified, not
    normalised): a numpy array, or a torch tensor on the GPU -- a view already resident in
    HBM is read in place (the returned DOM image is then a torch tensor too).  ``device``:
    the GPU that runs the pass; default the tensor's own GPU (device 0 for a host array).
    The threshold is used as given with either localization (ProcessDOM.java:104).
    ``downsample_xy`` / ``downsample_z`` (1, 2, 4 or 8): detect on the downsampled view
    (``downsample.downsample``; min, max and the returned DOM image are the downsampled
    view's) and return positions in pixels of the full view."""
    if (downsample_xy, downsample_z) != (1, 1):
        from . import downsample as ds
        from .dog import _correct_points
        res = compute(ds.downsample(img, downsample_xy, downsample_z, device=device), radius1, radius2,
                      threshold, localization, image_sigma, find_min, find_max, min_intensity, max_intensity,
                      keep_intensity, device, ij_threads, return_dom, max_peaks)
        _correct_points(res[0] if return_dom else res, downsample_xy, downsample_z)
        return res
    on_dev = hasattr(img, "is_cuda") and img.is_cuda
    if device is None:
        device = img.device.index if on_dev else 0
    p = _params(_lib.load(), radius1, radius2, threshold, localization, image_sigma, find_min, find_max,
                min_intensity, max_intensity, device, ij_threads)
    rec, dom = _run(img, p, return_dom, device)
    if max_peaks is not None:
        rec = rec[:int(max_peaks)]
    out = [InterestPoint(i, tuple(r["pos"].tolist()), float(r["intensity"]) if keep_intensity else None)
           for i, r in enumerate(rec)]
    return (out, dom) if return_dom else out


def interest_points_array(img, radius1: int = 2, radius2: int = 3, threshold: float = 0.02, localization: int = 0,
                          image_sigma=(0.5, 0.5, 0.5), find_min: bool = False, find_max: bool = True,
                          min_intensity: float = float("nan"), max_intensity: float = float("nan"),
                          device: int | None = None, ij_threads: int = 8, downsample_xy: int = 1,
                          downsample_z: int = 1):
    """ProcessDOM.compute as arrays: (positions (n, 3) x, y, z; intensities (n,)) in the
    reference's order -- no per-point Python objects.  ``device``, ``downsample_xy`` and
    ``downsample_z`` as in ``compute``."""
    if (downsample_xy, downsample_z) != (1, 1):
        from . import downsample as ds
        pos, inten = interest_points_array(ds.downsample(img, downsample_xy, downsample_z, device=device), radius1,
                                           radius2, threshold, localization, image_sigma, find_min, find_max,
                                           min_intensity, max_intensity, device, ij_threads)
        return ds.correct_for_downsampling(pos, downsample_xy, downsample_z), inten
    on_dev = hasattr(img, "is_cuda") and img.is_cuda
    if device is None:
        device = img.device.index if on_dev else 0
    p = _params(_lib.load(), radius1, radius2, threshold, localization, image_sigma, find_min, find_max,
                min_intensity, max_intensity, device, ij_threads)
    rec, _ = _run(img, p, False, device)
    return np.ascontiguousarray(rec["pos"]), np.ascontiguousarray(rec["intensity"])


def simple_peaks(img, radius1: int = 2, radius2: int = 3, threshold: float = 0.02, localization: int = 0,
                 image_sigma=(0.5, 0.5, 0.5), find_min: bool = False, find_max: bool = True,
                 min_intensity: float = float("nan"), max_intensity: float = float("nan"),
                 device: int = 0, ij_threads: int = 8, return_dom: bool = False):
    """InteractiveIntegral.findPeaks over the DOM image: [(x, y, z, |v|, is_min, is_max)]
    with |v| >= threshold (whatever ``localization``), of the wanted kinds; with
    ``return_dom`` also the DOM image.  ``img``: a numpy array."""
    lib = _lib.load()
    img = np.ascontiguousarray(img, np.float32)
    if img.ndim != 3:
        raise ValueError("img must be 3D [z, y, x]")
    p = _params(lib, radius1, radius2, threshold, localization, image_sigma, find_min, find_max, min_intensity,
                max_intensity, device, ij_threads)
    dims = (C.c_int64 * 3)(img.shape[2], img.shape[1], img.shape[0])
    dom = np.empty_like(img) if return_dom else None
    dptr = fptr(dom) if dom is not None else None
    n = C.c_int64(0)
    cap = max(1024, img.size // 64)
    while True:
        pk = (_lib.Peak * cap)()
        check(lib.spim_dom_compute(fptr(img), dims, C.byref(p), dptr, pk, cap, C.byref(n)))
        if int(n.value) <= cap:
            break
        cap = int(n.value)
    out = [(q.x, q.y, q.z, q.intensity, bool(q.is_min), bool(q.is_max)) for q in pk[:int(n.value)]]
    return (out, dom) if return_dom else out
