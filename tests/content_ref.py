"""Test helper: CPU restatement of the content-based fusion weights, composed from
the oracle (TEST INFRASTRUCTURE ONLY, like ``oracle/``).

``spim/process/fusion/weights/ContentBased.java:60-98`` (approximateEntropy), per
view and in the view's own voxel grid, float32 images:

    c = G(sigma1) (*) I        FFTConvolution over extendMirrorSingle, kernel
                               float(kx[x] * ky[y] * kz[z]) (:121-153)
    c = (c - I)^2              float difference, then float square (:86-87)
    c = G(sigma2) (*) c
    normalizeImage(c)          (c - min) / (max - min) in float; skipped when the
                               range is NaN, infinite or 0 (FusionHelper.java:159-184)

and the fusion with those weights (``weightedavg/ProcessParalellPortionWeights.java:
93-119``): w = product of the enabled weights, the content weight sampled n-linearly
over extendZero at the image's position t (``ContentBased.java:104-110``).
"""
from __future__ import annotations

import numpy as np

from oracle import input_ref as ir
from oracle import fusion_ref as fr
from oracle.dog_ref import gaussian_kernel_1d
from oracle.mvdecon_ref import convolve


def gaussian_kernel_3d(sigma_xyz) -> np.ndarray:
    """ContentBased.createGaussianKernel: [z, y, x] float32, value = ((1 * kx) * ky) * kz
    in double, cast to float."""
    kx, ky, kz = (gaussian_kernel_1d(float(s), True) for s in sigma_xyz)
    k = (1.0 * kx[None, None, :]) * ky[None, :, None] * kz[:, None, None]
    return k.astype(np.float32)


def normalize_image(c: np.ndarray) -> np.ndarray:
    """FusionHelper.normalizeImage (Math.min / Math.max propagate NaN, as ndarray.min does)."""
    c = np.asarray(c, np.float32)
    mn, mx = np.float32(c.min()), np.float32(c.max())
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.float32(mx - mn)
    if np.isnan(diff) or np.isinf(diff) or diff == 0:
        return c
    return ((c - mn).astype(np.float32) / diff).astype(np.float32)


def content_weights(img, s1, s2, precision: str = "f64", workers=8) -> np.ndarray:
    """img [z, y, x]; s1 / s2 (x, y, z).  ``precision`` is that of the FFT convolutions
    ("f32" stands in for the reference's own float FFT)."""
    img = np.ascontiguousarray(img, np.float32)
    c = convolve(img, gaussian_kernel_3d(s1), "mirror", precision, workers)
    d = (c - img).astype(np.float32)
    c = (d * d).astype(np.float32)
    c = convolve(c, gaussian_kernel_3d(s2), "mirror", precision, workers)
    return normalize_image(c)


def content_based_sigmas(voxel_size, sigma1=(20, 20, 20), sigma2=(40, 40, 40), adjust=True):
    """ProcessFusion.getContentBased (ProcessFusion.java:89-107); the loop bound of 2 is
    the reference's."""
    s1, s2 = [float(s) for s in sigma1], [float(s) for s in sigma2]
    min_res = min(float(v) for v in voxel_size)
    if adjust:
        for d in range(2):
            s1[d] /= float(voxel_size[d]) / min_res
            s2[d] /= float(voxel_size[d]) / min_res
    return s1, s2


def fuse(srcs, models, content_ws, bb_min, bb_dims, downsampling=1.0, interpolation=1,
         use_blending=False, borders=None, ranges=None) -> np.ndarray:
    """Weighted-average fusion with per-view content weight images ``content_ws``
    (source grids), multiplied into the blending weight or used alone."""
    shape = (int(bb_dims[2]), int(bb_dims[1]), int(bb_dims[0]))
    acc = np.zeros(shape)
    wsum = np.zeros(shape)
    for v, (src, m) in enumerate(zip(srcs, models)):
        src = np.asarray(src, np.float32)
        sz, sy, sx = src.shape
        t = ir.image_positions(m, bb_min, bb_dims, downsampling)
        inside = ((t[..., 0] >= 0) & (t[..., 1] >= 0) & (t[..., 2] >= 0)
                  & (t[..., 0] < sx) & (t[..., 1] < sy) & (t[..., 2] < sz))
        val = (ir.nlinear(src, t) if interpolation == 1 else fr.nearest(src, t)).astype(np.float64)
        w = np.ones(shape)
        if use_blending:
            w = w * ir.blending_weight(t, (sx, sy, sz), borders[v], ranges[v]).astype(np.float64)
        w = w * ir.nlinear(np.asarray(content_ws[v], np.float32), t, "zero").astype(np.float64)
        acc = np.where(inside, acc + val * w, acc)
        wsum = np.where(inside, wsum + w, wsum)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(wsum > 0, acc / wsum, 0.0).astype(np.float32)
