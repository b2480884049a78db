"""Host-side mirror of the deconvolution input preparation.

``ProcessForDeconvolution.fuseStacksAndGetPSFs``
(spim/process/fusion/deconvolution/ProcessForDeconvolution.java:159-384): each
view is resampled into the fused bounding box through the inverse of its
affine model, cosine blending weights are computed at the same source
positions, normalised across views (``WeightNormalizer``) and adjusted for the
OSEM speed-up -- all on the GPU in ``spim_prepare_inputs``.
"""
from __future__ import annotations

import ctypes as C
from enum import IntEnum

import numpy as np

from . import _lib
from ._lib import check, fptr


class WeightType(IntEnum):
    """ProcessForDeconvolution.WeightType members on the deconvolution path."""
    NO_WEIGHTS = 0
    PRECOMPUTED_WEIGHTS = 1
    VIRTUAL_WEIGHTS = 2


def prepare_inputs(srcs, models, bb_min, bb_dims, blending_border=(-8, -8, -8), blending_range=(12, 12, 12),
                   weight_type: WeightType = WeightType.VIRTUAL_WEIGHTS, osem_index: int = 0,
                   osem_speedup: float = 1.0, ij_threads: int = 8, device: int = 0):
    """srcs: [z, y, x] float32 stacks; models: 3x4 (source -> world) affine per
    view; bb_min / bb_dims: (x, y, z).  Returns (imgs, weights, info) with
    imgs/weights [z, y, x] float32 per view and info = {osem, min_overlap,
    avg_overlap}."""
    lib = _lib.load()
    V = len(srcs)
    if V < 1 or len(models) != V:
        raise ValueError("need one model per view")
    if all(hasattr(s, "is_cuda") and s.is_cuda for s in srcs):
        return _prepare_inputs_device(lib, srcs, models, bb_min, bb_dims, blending_border, blending_range,
                                      weight_type, osem_index, osem_speedup, ij_threads, device)
    srcs = [np.ascontiguousarray(s, np.float32) for s in srcs]
    views = (_lib.ViewSource * V)()
    for v, (s, m) in enumerate(zip(srcs, models)):
        if s.ndim != 3:
            raise ValueError("sources must be 3D [z, y, x]")
        views[v].img = fptr(s)
        views[v].dims[:] = [s.shape[2], s.shape[1], s.shape[0]]
        views[v].model[:] = [float(x) for x in np.asarray(m, np.float64).reshape(12)]
    p = _lib.InputParams()
    lib.spim_input_params_default(C.byref(p))
    p.bb_min[:] = [int(x) for x in bb_min]
    p.bb_dims[:] = [int(x) for x in bb_dims]
    p.blending_border[:] = [float(x) for x in blending_border]
    p.blending_range[:] = [float(x) for x in blending_range]
    p.weight_type = int(weight_type)
    p.osem_index = int(osem_index)
    p.osem_speedup = float(osem_speedup)
    p.ij_threads = int(ij_threads)
    p.device = int(device)
    shape = (int(bb_dims[2]), int(bb_dims[1]), int(bb_dims[0]))
    imgs = [np.empty(shape, np.float32) for _ in range(V)]
    ws = [np.empty(shape, np.float32) for _ in range(V)]
    ip = (_lib._pf * V)(*[fptr(a) for a in imgs])
    wp = (_lib._pf * V)(*[fptr(a) for a in ws])
    osem, mn, av = C.c_double(), C.c_int(), C.c_double()
    check(lib.spim_prepare_inputs(V, views, C.byref(p), ip, wp, C.byref(osem), C.byref(mn), C.byref(av)))
    return imgs, ws, {"osem": osem.value, "min_overlap": mn.value, "avg_overlap": av.value}


def _prepare_inputs_device(lib, srcs, models, bb_min, bb_dims, blending_border, blending_range, weight_type,
                           osem_index, osem_speedup, ij_threads, device):
    """prepare_inputs for torch tensors on the GPU: read in place, results as torch
    tensors on the same device (no host round trip)."""
    import torch
    V = len(srcs)
    srcs = [s.contiguous().float() for s in srcs]
    torch.cuda.synchronize(srcs[0].device)   # the library runs on its own stream
    views = (_lib.ViewSource * V)()
    for v, (s, m) in enumerate(zip(srcs, models)):
        if s.dim() != 3:
            raise ValueError("sources must be 3D [z, y, x]")
        views[v].img = C.cast(C.c_void_p(s.data_ptr()), _lib._pf)
        views[v].dims[:] = [s.shape[2], s.shape[1], s.shape[0]]
        views[v].model[:] = [float(x) for x in np.asarray(m, np.float64).reshape(12)]
    p = _lib.InputParams()
    lib.spim_input_params_default(C.byref(p))
    p.bb_min[:] = [int(x) for x in bb_min]
    p.bb_dims[:] = [int(x) for x in bb_dims]
    p.blending_border[:] = [float(x) for x in blending_border]
    p.blending_range[:] = [float(x) for x in blending_range]
    p.weight_type = int(weight_type)
    p.osem_index = int(osem_index)
    p.osem_speedup = float(osem_speedup)
    p.ij_threads = int(ij_threads)
    p.device = int(device)
    p.src_on_device = 1
    p.out_on_device = 1
    shape = (int(bb_dims[2]), int(bb_dims[1]), int(bb_dims[0]))
    imgs = [torch.empty(shape, dtype=torch.float32, device=srcs[0].device) for _ in range(V)]
    ws = [torch.empty(shape, dtype=torch.float32, device=srcs[0].device) for _ in range(V)]
    ip = (_lib._pf * V)(*[C.cast(C.c_void_p(a.data_ptr()), _lib._pf) for a in imgs])
    wp = (_lib._pf * V)(*[C.cast(C.c_void_p(a.data_ptr()), _lib._pf) for a in ws])
    osem, mn, av = C.c_double(), C.c_int(), C.c_double()
    check(lib.spim_prepare_inputs(V, views, C.byref(p), ip, wp, C.byref(osem), C.byref(mn), C.byref(av)))
    return imgs, ws, {"osem": osem.value, "min_overlap": mn.value, "avg_overlap": av.value}


def content_based_sigmas(voxel_size, sigma1=(20, 20, 20), sigma2=(40, 40, 40), adjust: bool = True):
    """ProcessFusion.getContentBased (spim/process/fusion/weightedavg/ProcessFusion.java:89-107):
    with ``adjust`` (defaultAdjustContentBasedSigmaForAnisotropy) the sigmas of axes 0 and 1
    -- the reference's loop stops at 2 -- are divided by voxel_size[d] / min(voxel_size).
    voxel_size, sigmas: (x, y, z).  Returns (sigma1, sigma2) as lists of floats."""
    vs = [float(v) for v in voxel_size]
    s1, s2 = [float(s) for s in sigma1], [float(s) for s in sigma2]
    if len(vs) != 3 or len(s1) != 3 or len(s2) != 3:
        raise ValueError("voxel_size, sigma1 and sigma2 take 3 values (x, y, z)")
    min_res = min(vs)
    if adjust:
        for d in range(2):
            s1[d] /= vs[d] / min_res
            s2[d] /= vs[d] / min_res
    return s1, s2


def _sigma3(sigma, count=1):
    a = np.ascontiguousarray(np.asarray(sigma, np.float64))
    if a.size == 3 and count > 1:
        a = np.ascontiguousarray(np.tile(a.reshape(1, 3), (count, 1)))
    if a.size != 3 * count:
        raise ValueError(f"sigma needs 3 values (x, y, z){' per view' if count > 1 else ''}")
    return a


def content_based_weights(img, sigma1=(20, 20, 20), sigma2=(40, 40, 40), device: int = 0):
    """Content-based fusion weights of one view (ContentBased.approximateEntropy,
    spim/process/fusion/weights/ContentBased.java:60-98): the [z, y, x] float32 image
    normalise(G(sigma2) * (G(sigma1) * img - img)^2), Gaussians over extendMirrorSingle,
    sigmas (x, y, z).  A torch tensor on the GPU is read in place and the weights come
    back as a tensor on the same device; anything else goes through numpy."""
    lib = _lib.load()
    s1, s2 = _sigma3(sigma1), _sigma3(sigma2)
    pd = lambda a: a.ctypes.data_as(_lib._pd)
    if hasattr(img, "is_cuda") and img.is_cuda:
        import torch
        if img.dim() != 3:
            raise ValueError("img must be 3D [z, y, x]")
        img = img.contiguous().float()
        torch.cuda.synchronize(img.device)   # the library runs on its own stream
        dims = (C.c_int64 * 3)(img.shape[2], img.shape[1], img.shape[0])
        out = torch.empty_like(img)
        check(lib.spim_content_based_weights(img.data_ptr(), dims, pd(s1), pd(s2), out.data_ptr(),
                                             img.device.index or 0))
        return out
    img = np.ascontiguousarray(img, np.float32)
    if img.ndim != 3:
        raise ValueError("img must be 3D [z, y, x]")
    dims = (C.c_int64 * 3)(img.shape[2], img.shape[1], img.shape[0])
    out = np.empty_like(img)
    check(lib.spim_content_based_weights(img.ctypes.data, dims, pd(s1), pd(s2), out.ctypes.data, int(device)))
    return out


def content_tile_sizes():
    """(outputs per line and block along the pass axis, lines per block, taps per register-
    window step, the tap limit, threads per reduction block, reduction blocks) of the
    content-weight kernels."""
    sizes = (C.c_int32 * 6)()
    _lib.load().spim_content_tiles(sizes)
    return tuple(int(s) for s in sizes)


def fuse_weighted_average(srcs, models, bb_min, bb_dims, downsampling: float = 1.0, interpolation: int = 1,
                          use_blending: bool = True, blending_borders=None, blending_ranges=None,
                          device: int = 0, use_content_based: bool = False, content_sigma1=None,
                          content_sigma2=None) -> np.ndarray:
    """Weighted-average fusion (spim/process/fusion/weightedavg/ProcessParalell*.java):
    [z, y, x] float32 fused volume.  blending_borders / ranges: (x, y, z) per view.
    use_content_based: every view's content-based weight (content_based_weights with
    content_sigma1 / content_sigma2, (x, y, z) for all views or one triple per view;
    default 20 / 40) is multiplied into its blending weight, or used alone."""
    lib = _lib.load()
    V = len(srcs)
    srcs = [np.ascontiguousarray(s, np.float32) for s in srcs]
    views = (_lib.ViewSource * V)()
    for v, (s, m) in enumerate(zip(srcs, models)):
        views[v].img = fptr(s)
        views[v].dims[:] = [s.shape[2], s.shape[1], s.shape[0]]
        views[v].model[:] = [float(x) for x in np.asarray(m, np.float64).reshape(12)]
    p = _lib.FusionParams()
    lib.spim_fusion_params_default(C.byref(p))
    p.bb_min[:] = [int(x) for x in bb_min]
    p.bb_dims[:] = [int(x) for x in bb_dims]
    p.downsampling = float(downsampling)
    p.interpolation = int(interpolation)
    p.use_blending = int(bool(use_blending))
    p.device = int(device)
    b = r = None
    if use_blending:
        b = np.ascontiguousarray(np.asarray(blending_borders, np.float32).reshape(V, 3))
        r = np.ascontiguousarray(np.asarray(blending_ranges, np.float32).reshape(V, 3))
    out = np.empty((int(bb_dims[2]), int(bb_dims[1]), int(bb_dims[0])), np.float32)
    if use_content_based:
        s1 = _sigma3((20, 20, 20) if content_sigma1 is None else content_sigma1, V)
        s2 = _sigma3((40, 40, 40) if content_sigma2 is None else content_sigma2, V)
        check(lib.spim_fuse_weighted_average_content(
            V, views, C.byref(p), fptr(b) if b is not None else None, fptr(r) if r is not None else None,
            s1.ctypes.data_as(_lib._pd), s2.ctypes.data_as(_lib._pd), fptr(out)))
        return out
    check(lib.spim_fuse_weighted_average(V, views, C.byref(p), fptr(b) if b is not None else None,
                                         fptr(r) if r is not None else None, fptr(out)))
    return out
