"""Restatement of the reference's automatic bounding box estimation ("Estimate automatically
(experimental)"), operation by operation in NumPy.  TEST INFRASTRUCTURE ONLY.

Paths under the reference's src/main/java/spim/process/fusion/:
  boundingbox/AutomaticBoundingBox.java:36-131          queryParameters: the maximal box, rounded
  boundingbox/BoundingBoxGUI.java:340-399               getDimensions, computeMaxBoundingBoxDimensions
  boundingbox/automatic/MinFilterThreshold.java:76-308  run, computeBoundingBox, computeLazyMinFilter
  FusionHelper.java:87-138                              minMax

Images are [z, y, x] float32; boxes, dims and positions are (x, y, z).

Java's Math.min / Math.max on floats: a NaN operand is the result, and -0.0 < +0.0.  On values
that are not NaN they are the minimum / maximum of a total order, so they are exact,
commutative and associative: the minimum of a window has the same bits whatever the order of
evaluation (doubling, van Herk, a sliding window, a tree).  That is what lets the GPU filter
be bit-exact with a different algorithm.  With a NaN the result is a NaN whatever the order;
its payload is the one of the first NaN met, so the bits are pinned only for images whose NaNs
all carry one payload (the tests use numpy's).

Fusion variant: the dialog's default "Load input images sequentially" runs ProcessSequential,
which accumulates value and weight sums in float images view after view.  Restated here, as
in ``oracle/fusion_ref.py`` and on the GPU, is ProcessParalell (double sums per voxel).
PARITY UNPINNED for ProcessSequential: with two or more overlapping views its fused values
can differ in the last bit.
"""
from __future__ import annotations

import numpy as np

from oracle import fusion_ref

FLOAT_MAX = np.float32(3.4028234663852886e38)
DEFAULT_BACKGROUND = 5.0          # AutomaticBoundingBox.defaultBackgroundIntensity
DEFAULT_DISCARDED_SIZE = 25       # defaultDiscardedObjectSize
DEFAULT_DOWNSAMPLING = 4          # defaultDownsamplingAutomatic


def java_round(x) -> int:
    """Math.round(double): floor(x + 0.5); -2.5 -> -2."""
    return int(np.floor(np.float64(x) + 0.5))


def jmin(a, b):
    """Math.min(float, float), elementwise."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.where(a <= b, a, b)                       # b when b is NaN
        r = np.where((a == 0) & (b == 0) & np.signbit(b), b, r)   # -0 wins over +0
        r = np.where(a != a, a, r)                       # a NaN a is the result
    return r.astype(np.float32)


def jmax(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.where(a >= b, a, b)
        r = np.where((a == 0) & (b == 0) & ~np.signbit(b), b, r)  # +0 wins over -0
        r = np.where(a != a, a, r)
    return r.astype(np.float32)


def max_bounding_box(dims, models, downsampling: int = 1):
    """computeMaxBoundingBoxDimensions + AutomaticBoundingBox.java:55-60 + getDimensions.
    dims: per view (x, y, z); models: per view 3x4.  Returns (bb_min, bb_max, bb_dims,
    fused_dims), lists of ints."""
    lo = [np.finfo(np.float64).max] * 3
    hi = [-np.finfo(np.float64).max] * 3
    for d, m in zip(dims, models):
        m = np.asarray(m, np.float64).reshape(3, 4)
        for c in range(8):        # AffineTransform3D.estimateBounds: the corners of [0, dim - 1]
            p = [float(d[a] - 1) if (c >> a) & 1 else 0.0 for a in range(3)]
            for a in range(3):
                t = m[a, 0] * p[0] + m[a, 1] * p[1] + m[a, 2] * p[2] + m[a, 3]
                lo[a] = min(lo[a], t)
                hi[a] = max(hi[a], t)
    bb_min = [java_round(v) for v in lo]
    bb_max = [java_round(v) for v in hi]
    bb_dims = [b - a + 1 for a, b in zip(bb_min, bb_max)]
    return bb_min, bb_max, bb_dims, [d // int(downsampling) for d in bb_dims]


def min_max(img):
    """FusionHelper.minMax: from +-Float.MAX_VALUE over every voxel (uncovered ones, 0, too)."""
    mn, mx = FLOAT_MAX, np.float32(-FLOAT_MAX)
    for v in np.asarray(img, np.float32).ravel():
        mn = jmin(mn, v)[()]
        mx = jmax(mx, v)[()]
    return np.float32(mn), np.float32(mx)


def min_max_fast(img):
    """min_max by a tree over the flat image (the same bits: see the module docstring)."""
    a = np.asarray(img, np.float32).ravel()
    lo = np.concatenate([[FLOAT_MAX], a]).astype(np.float32)
    hi = np.concatenate([[-FLOAT_MAX], a]).astype(np.float32)
    while len(lo) > 1:
        if len(lo) % 2:
            lo = np.concatenate([lo, lo[-1:]])
            hi = np.concatenate([hi, hi[-1:]])
        lo = jmin(lo[0::2], lo[1::2])
        hi = jmax(hi[0::2], hi[1::2])
    return np.float32(lo[0]), np.float32(hi[0])


def threshold(mn, mx, background: float = DEFAULT_BACKGROUND) -> float:
    """MinFilterThreshold.java:90: the difference in float, the rest in double."""
    with np.errstate(invalid="ignore", over="ignore"):
        rng = np.float32(np.float32(mx) - np.float32(mn))
    return float(np.float64(rng) * (np.float64(background) / 100.0) + np.float64(np.float32(mn)))


def min_filter_axis(img, radius: int, axis: int):
    """One pass of computeLazyMinFilter: min from Float.MAX_VALUE over the 2r + 1 voxels
    i - r .. i + r along ``axis`` of Views.extendZero(img), in that order."""
    img = np.asarray(img, np.float32)
    n = img.shape[axis]
    pad = [(0, 0)] * 3
    pad[axis] = (radius, radius)
    ext = np.pad(img, pad, constant_values=np.float32(0.0))
    out = np.full(img.shape, FLOAT_MAX, np.float32)
    for i in range(2 * radius + 1):
        sl = [slice(None)] * 3
        sl[axis] = slice(i, i + n)
        out = jmin(out, ext[tuple(sl)])
    return out


def min_filter(img, radius: int):
    """computeLazyMinFilter: dimension 0 (x), then 1 (y), then 2 (z)."""
    out = np.asarray(img, np.float32)
    for axis in (2, 1, 0):
        out = min_filter_axis(out, radius, axis)
    return out


def threshold_bounds(img, thr: float):
    """computeBoundingBox: (min, max, found), (x, y, z); min starts at the dims, max at 0.
    The reference returns the inverted box silently when nothing is above the threshold;
    ``found`` is added."""
    img = np.asarray(img, np.float32)
    dims = img.shape[::-1]
    lo, hi = list(dims), [0, 0, 0]
    with np.errstate(invalid="ignore"):
        idx = np.nonzero(img.astype(np.float64) > np.float64(thr))
    found = len(idx[0]) > 0
    if found:
        for a in range(3):
            lo[a] = min(lo[a], int(idx[2 - a].min()))
            hi[a] = max(hi[a], int(idx[2 - a].max()))
    return lo, hi, found


def segment(img, background: float = DEFAULT_BACKGROUND, radius: int = 1):
    """min / max -> threshold -> filter -> box of one image: a dict."""
    mn, mx = min_max_fast(img)
    thr = threshold(mn, mx, background)
    filt = min_filter(img, radius)
    lo, hi, found = threshold_bounds(filt, thr)
    return {"min": mn, "max": mx, "threshold": thr, "filtered": filt, "bounds_min": lo, "bounds_max": hi,
            "found": found}


def radii(discarded_object_size: int = DEFAULT_DISCARDED_SIZE, downsampling: int = DEFAULT_DOWNSAMPLING):
    """(radiusMin, effR): MinFilterThreshold.java:68, :89 (integer divisions)."""
    radius_min = int(discarded_object_size) // 2
    return radius_min, max(radius_min // int(downsampling), 1)


def auto_bounding_box(views, models, background: float = DEFAULT_BACKGROUND,
                      discarded_object_size: int = DEFAULT_DISCARDED_SIZE,
                      downsampling: int = DEFAULT_DOWNSAMPLING, fused=None):
    """AutomaticBoundingBox.queryParameters + MinFilterThreshold.run.  ``fused``: the fused
    image, when the caller already has it.  Returns a dict (bb_min, bb_max, bb_dims, found and
    the intermediate numbers); no clamping to the maximal box."""
    dims = [np.asarray(v).shape[::-1] for v in views]
    mb_min, mb_max, mb_dims, fdims = max_bounding_box(dims, models, downsampling)
    if fused is None:
        fused = fusion_ref.fuse_weighted_average(views, models, mb_min, fdims, downsampling=float(downsampling),
                                                 interpolation=0, use_blending=False)
    radius_min, eff_r = radii(discarded_object_size, downsampling)
    seg = segment(fused, background, eff_r)
    bb_min = [seg["bounds_min"][a] * downsampling + mb_min[a] - 3 * radius_min for a in range(3)]
    bb_max = [seg["bounds_max"][a] * downsampling + mb_min[a] + 3 * radius_min for a in range(3)]
    return {"bb_min": bb_min, "bb_max": bb_max, "bb_dims": [b - a + 1 for a, b in zip(bb_min, bb_max)],
            "found": seg["found"], "max_min": mb_min, "max_max": mb_max, "max_dims": mb_dims,
            "fused_dims": fdims, "radius_min": radius_min, "eff_radius": eff_r, "fused": fused, **{
                k: seg[k] for k in ("min", "max", "threshold", "filtered", "bounds_min", "bounds_max")}}


# ---------------------------------------------------------------- the end-to-end scene
def scene():
    """Three small views of one sample for the end-to-end tests: a bright ellipsoid, beads
    smaller than the discarded size (one far from the ellipsoid), low background.  The views
    are translated copies of one world volume sampled on integer offsets, so nearest-neighbour
    fusion at downsampling 2 reads exact voxels.  Returns (views, models, params, truth)."""
    rng = np.random.default_rng(20)
    nz, ny, nx = 36, 48, 40
    world = (rng.random((nz + 8, ny + 8, nx + 12)) * 0.008).astype(np.float32)     # background <= 1 % of 1.0
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in world.shape], indexing="ij")
    centre, semi = (22.0, 28.0, 24.0), (9.0, 12.0, 10.0)                        # (z, y, x)
    inside = ((z - centre[0]) / semi[0]) ** 2 + ((y - centre[1]) / semi[1]) ** 2 + ((x - centre[2]) / semi[2]) ** 2 <= 1
    world[inside] = (0.6 + 0.4 * rng.random(int(inside.sum()))).astype(np.float32)   # >= 50 % of the range
    beads = [(6, 8, 44), (30, 10, 8), (12, 44, 40), (36, 50, 46)]                 # (z, y, x); 3 voxels wide
    for bz, by, bx in beads:
        world[bz - 1:bz + 2, by - 1:by + 2, bx - 1:bx + 2] = 1.0
    offsets = [(0, 0, 0), (12, 4, 2), (6, 8, 8)]                                    # (x, y, z) of each view's origin
    views, models = [], []
    for ox, oy, oz in offsets:
        views.append(np.ascontiguousarray(world[oz:oz + nz, oy:oy + ny, ox:ox + nx]))
        models.append(np.array([[1, 0, 0, ox], [0, 1, 0, oy], [0, 0, 1, oz]], np.float64))
    params = {"background": 5.0, "discarded_object_size": 8, "downsampling": 2}      # radiusMin 4, effR 2
    truth = {"ellipsoid_min": [int(np.ceil(centre[2 - a] - semi[2 - a])) for a in range(3)],
             "ellipsoid_max": [int(np.floor(centre[2 - a] + semi[2 - a])) for a in range(3)],
             "far_bead": (46, 50, 36)}                                                # (x, y, z), world
    return views, models, params, truth
