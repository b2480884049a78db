"""Test helper: NumPy restatement of the reference's Difference-of-Mean detector (TEST
INFRASTRUCTURE ONLY, like ``oracle/`` and ``tests/content_ref.py``).

    spim/process/interestpointdetection/ProcessDOM.java:36-117   diameters, min / max, peaks
    mpicbg/spim/segmentation/IntegralImage3d.java:60-210         (long)(int) voxel, three prefix passes
    mpicbg/spim/segmentation/DOM.java:29-171                     sixteen corner reads, the value

Two forms of the DOM image: ``dom_image`` (vectorised) and ``dom_image_literal`` (the
reference's loops, voxel by voxel).  Volumes are [z, y, x] float32.  Peaks and the
quadratic fit are the oracle's (``oracle.dog_ref.find_peaks`` / ``quadratic_localization``).
"""
from __future__ import annotations

import math

import numpy as np

from oracle import dog_ref

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def box_diameters(radius1=2, radius2=3, image_sigma=(0.5, 0.5, 0.5)):
    """ProcessDOM.java:71-78 (double arithmetic, Math.round = floor(x + 0.5)): per axis
    x, y, z the diameters ((s1x, s1y, s1z), (s2x, s2y, s2z))."""
    s1 = tuple(max(3, int(math.floor(radius1 * (0.5 / s) + 0.5)) * 2 + 1) for s in image_sigma)
    s2 = tuple(max(5, int(math.floor(radius2 * (0.5 / s) + 0.5)) * 2 + 1) for s in image_sigma)
    return s1, s2


def java_int(img) -> np.ndarray:
    """(long)(int) of a float (IntegralImage3d.java:102,110): toward zero, NaN -> 0,
    saturating at Integer.MIN_VALUE / MAX_VALUE.  int64."""
    a = np.asarray(img, np.float32).astype(np.float64)
    t = np.trunc(np.where(np.isnan(a), 0.0, a))
    return np.clip(t, I32_MIN, I32_MAX).astype(np.int64)


def min_max(img, min_intensity=float("nan"), max_intensity=float("nan")):
    """ProcessDOM.java:54-66: the caller's range as float, or FusionHelper.minMax of the
    image (FusionHelper.java:87-141: Math.min / Math.max from +-Float.MAX_VALUE, so a NaN
    voxel makes both NaN)."""
    if (math.isnan(min_intensity) or math.isnan(max_intensity) or math.isinf(min_intensity)
            or math.isinf(max_intensity) or min_intensity == max_intensity):
        a = np.asarray(img, np.float32)
        if np.isnan(a).any():
            return np.float32("nan"), np.float32("nan")
        fmax = np.finfo(np.float32).max
        return np.float32(min(fmax, a.min())), np.float32(max(-fmax, a.max()))
    return np.float32(min_intensity), np.float32(max_intensity)


def integral_image(img) -> np.ndarray:
    """IntegralImage3d.compute: [nz + 1, ny + 1, nx + 1] int64, zero first planes; sums
    wrap modulo 2^64 as Java's long does."""
    v = java_int(img)
    nz, ny, nx = v.shape
    out = np.zeros((nz + 1, ny + 1, nx + 1), np.int64)
    out[1:, 1:, 1:] = v.cumsum(2).cumsum(1).cumsum(0)
    return out


def box_sums(integral, s, hm) -> np.ndarray:
    """DOM.java:97-153: the 8-corner sums of the box of diameters s = (sx, sy, sz) centred
    on every voxel hm <= p < n - hm (hm: the half sizes (x, y, z) of the support)."""
    nz, ny, nx = (n - 1 for n in integral.shape)
    w, h, d = nx - 2 * hm[0], ny - 2 * hm[1], nz - 2 * hm[2]
    lo = [hm[a] - s[a] // 2 for a in range(3)]          # first corner of the first voxel

    def c(ix, iy, iz):   # corner block: 0 = low, 1 = high (low + s)
        x0, y0, z0 = lo[0] + ix * s[0], lo[1] + iy * s[1], lo[2] + iz * s[2]
        return integral[z0:z0 + d, y0:y0 + h, x0:x0 + w]
    # -r11 + r12 - r13 + r14 - r15 + r16 - r17 + r18 (DOM.java:152)
    return -c(0, 0, 0) + c(1, 0, 0) - c(1, 1, 0) + c(0, 1, 0) - c(0, 1, 1) + c(1, 1, 1) - c(1, 0, 1) + c(0, 0, 1)


def _half_max(s1, s2):
    return tuple(max(s1[a], s2[a]) // 2 for a in range(3))


def dom_value(sum1, sum2, s1, s2, mn, mx) -> np.ndarray:
    """DOM.java:31-37,155 in float32: (float) s2 / d2 - (float) s1 / d1."""
    diff = np.float32(np.float32(mx) - np.float32(mn))
    with np.errstate(all="ignore"):
        d1 = np.float32(np.float32(np.int32(s1[0] * s1[1] * s1[2])) * diff)
        d2 = np.float32(np.float32(np.int32(s2[0] * s2[1] * s2[2])) * diff)
        a = (np.asarray(sum2, np.int64).astype(np.float32) / d2).astype(np.float32)
        b = (np.asarray(sum1, np.int64).astype(np.float32) / d1).astype(np.float32)
        return (a - b).astype(np.float32)


def dom_image(img, s1, s2, mn, mx) -> np.ndarray:
    """The DOM image (vectorised): zero outside the support (ProcessDOM.java:89-94), all
    zero when an axis is not longer than twice its half size."""
    img = np.asarray(img, np.float32)
    nz, ny, nx = img.shape
    out = np.zeros(img.shape, np.float32)
    hm = _half_max(s1, s2)
    if nx <= 2 * hm[0] or ny <= 2 * hm[1] or nz <= 2 * hm[2]:
        return out
    integral = integral_image(img)
    v = dom_value(box_sums(integral, s1, hm), box_sums(integral, s2, hm), s1, s2, mn, mx)
    out[hm[2]:nz - hm[2], hm[1]:ny - hm[1], hm[0]:nx - hm[0]] = v
    return out


def _wrap(v: int) -> int:
    """Java long arithmetic on a Python int."""
    return (v + 2 ** 63) % 2 ** 64 - 2 ** 63


def integral_image_literal(img) -> np.ndarray:
    """IntegralImage3d.computeArray's three passes (:84-209), as written."""
    f = np.asarray(img, np.float32)
    nz, ny, nx = f.shape
    w, h, d = nx + 1, ny + 1, nz + 1
    data = [0] * (w * h * d)
    data_f = f.ravel()
    iv = java_int(data_f).tolist()
    index = lambda x, y, z, ww, hh: (z * hh + y) * ww + x
    for z in range(1, d):                        # sum over x (:92-115)
        for y in range(1, h):
            i_in = index(0, y - 1, z - 1, nx, ny)
            i_out = index(1, y, z, w, h)
            s = iv[i_in]
            data[i_out] = s
            for x in range(2, w):
                i_in += 1
                i_out += 1
                s = _wrap(s + iv[i_in])
                data[i_out] = s
    for z in range(1, d):                        # sum over y (:137-157)
        for x in range(1, w):
            i = index(x, 1, z, w, h)
            s = data[i]
            for y in range(2, h):
                i += w
                s = _wrap(s + data[i])
                data[i] = s
    inc = w * h
    for y in range(1, h):                        # sum over z (:180-205)
        for x in range(1, w):
            i = index(x, y, 1, w, h)
            s = data[i]
            for z in range(2, d):
                i += inc
                s = _wrap(s + data[i])
                data[i] = s
    return np.array(data, np.int64).reshape(d, h, w)


def dom_image_literal(img, s1, s2, mn, mx) -> np.ndarray:
    """DOM.computeDifferencOfMean3d (:29-171) as written: sixteen cursors set per row and
    moved forward along x, one float32 value per voxel."""
    img = np.asarray(img, np.float32)
    nz, ny, nx = img.shape
    out = np.zeros(img.shape, np.float32)
    integral = integral_image_literal(img)
    f32 = np.float32
    diff = f32(f32(mx) - f32(mn))
    sx1, sy1, sz1 = s1
    sx2, sy2, sz2 = s2
    with np.errstate(all="ignore"):
        d1 = f32(f32(np.int32(sx1 * sy1 * sz1)) * diff)
        d2 = f32(f32(np.int32(sx2 * sy2 * sz2)) * diff)
    hxm, hym, hzm = max(sx1 // 2, sx2 // 2), max(sy1 // 2, sy2 // 2), max(sz1 // 2, sz2 // 2)
    w = nx - (max(sx1, sx2) // 2) * 2
    h = ny - (max(sy1, sy2) // 2) * 2
    d = nz - (max(sz1, sz2) // 2) * 2

    def cursors(x0, y0, z0, sx, sy, sz):
        """r_1 .. r_8 as [x, y, z] (:101-123)."""
        p = [x0, y0, z0]
        rs = [list(p)]
        for axis, step in ((0, sx), (1, sy), (0, -sx), (2, sz), (0, sx), (1, -sy), (0, -sx)):
            p[axis] += step
            rs.append(list(p))
        return rs
    signs = (-1, 1, -1, 1, -1, 1, -1, 1)
    for z in range(d):
        for y in range(h):
            r1 = cursors(hxm - sx1 // 2, y + hym - sy1 // 2, z + hzm - sz1 // 2, sx1, sy1, sz1)
            r2 = cursors(hxm - sx2 // 2, y + hym - sy2 // 2, z + hzm - sz2 // 2, sx2, sy2, sz2)
            for x in range(w):
                sum1 = sum2 = 0
                for sg, r in zip(signs, r1):
                    sum1 = _wrap(sum1 + sg * int(integral[r[2], r[1], r[0] + x]))
                for sg, r in zip(signs, r2):
                    sum2 = _wrap(sum2 + sg * int(integral[r[2], r[1], r[0] + x]))
                with np.errstate(all="ignore"):
                    out[z + hzm, y + hym, x + hxm] = f32(f32(np.int64(sum2)) / d2) - f32(f32(np.int64(sum1)) / d1)
    return out


def direct_box_sums(img, s, hm) -> np.ndarray:
    """A plain triple loop over the box of every supported voxel (Python ints wrapped to
    long): what the integral image's corners must add up to."""
    v = java_int(img)
    nz, ny, nx = v.shape
    h = [s[a] // 2 for a in range(3)]
    out = np.zeros((nz - 2 * hm[2], ny - 2 * hm[1], nx - 2 * hm[0]), np.int64)
    for z in range(hm[2], nz - hm[2]):
        for y in range(hm[1], ny - hm[1]):
            for x in range(hm[0], nx - hm[0]):
                box = v[z - h[2]:z + h[2] + 1, y - h[1]:y + h[1] + 1, x - h[0]:x + h[0] + 1]
                out[z - hm[2], y - hm[1], x - hm[0]] = _wrap(sum(box.ravel().tolist()))
    return out


def process_dom(img, radius1=2, radius2=3, threshold=0.02, localization=0, image_sigma=(0.5, 0.5, 0.5),
                find_min=False, find_max=True, min_intensity=float("nan"), max_intensity=float("nan"),
                ij_threads=8):
    """ProcessDOM.compute (:36-117): (points [(x, y, z, intensity)], ordered peaks
    [(x, y, z, |v|, is_min, is_max)] of the wanted kinds, DOM image).  The peaks are taken
    at ``threshold`` itself with either localization (:104); localization 1 keeps the
    fitted values with |v| > threshold (Localization.java:47-88)."""
    s1, s2 = box_diameters(radius1, radius2, image_sigma)
    mn, mx = min_max(img, min_intensity, max_intensity)
    dom = dom_image(img, s1, s2, mn, mx)
    peaks = [p for p in dog_ref.find_peaks(dom, float(np.float32(threshold)), ij_threads)
             if (p[5] and find_max) or (p[4] and find_min)]
    pts = [(p[0], p[1], p[2], p[3]) for p in peaks]
    if localization == 1:
        pts = [(float(x), float(y), float(z), float(v)) for x, y, z, v in dog_ref.quadratic_localization(dom, pts)
               if abs(v) > np.float32(threshold)]
    return pts, peaks, dom


# ------------------------------------------------------------------ k_dom's z chunks
def z_chunks(nz, hm_z):
    """csrc/dom.hip, dom_tile's rule restated: a block walks max(64, 8 hm_z) output planes of
    the nz - 2 hm_z that the boxes reach, and starts its running z sums afresh.  Returns the
    chunks' lengths."""
    zc, inner = max(64, 8 * hm_z), nz - 2 * hm_z
    return [min(zc, inner - z0) for z0 in range(0, max(inner, 0), zc)]


def tile_columns(hm):
    """dom_tile's choice restated: among tiles of 16 / 32 / 64 x 1 .. 32 outputs whose columns
    (tile + halo) number at most 16 x 256 and whose two LDS tiles of 16-byte entries fit 64 KiB,
    the first with the highest outputs per column x min(blocks per 160 KiB, 4).  Returns its
    columns: more than 8 x 256 take the instantiation of 16 columns per thread."""
    best, ncol_best = -1.0, 0
    for lx in (4, 5, 6):
        for ty in range(1, 33):
            tx, hx, hy = 1 << lx, (1 << lx) + 2 * hm[0], ty + 2 * hm[1]
            ncol, lds = hx * hy, (hx * hy + tx * hy) * 16
            if ncol > 16 * 256 or lds > 64 * 1024:
                continue
            score = tx * ty / ncol * min(160 * 1024 // lds, 4)
            if score > best:
                best, ncol_best = score, ncol
    return ncol_best


# name -> ((nz, ny, nx), keywords of process_dom, the chunks' lengths)
Z_CHUNK_CASES = {
    "ragged": ((64 + 6 + 5, 20, 24), {}, [64, 5]),
    "two_full": ((2 * 64 + 6, 20, 24), {}, [64, 64]),
    "largest_box": ((128 + 32 + 3, 36, 40), {"radius1": 15, "radius2": 16}, [128, 3]),     # 16 columns per thread
    "anisotropic": ((96 + 24 + 5, 14, 20), {"image_sigma": (0.5, 0.5, 0.125)}, [96, 5]),   # hm_z 12, hm_x 3
}


def z_chunk_volume(name):
    shape = Z_CHUNK_CASES[name][0]
    img = (np.random.default_rng(len(name)).random(shape) * 4000).astype(np.float32)
    img.setflags(write=False)
    return img


def sparse_integer_volume(shape=(75, 20, 24), seed=17):
    """Zeros with a few small integers: the box sums tie over wide regions (plateaus of equal
    DOM values, exact zeros among them), across the chunk seam too."""
    rng = np.random.default_rng(seed)
    img = np.where(rng.random(shape) < 0.004, np.round(rng.random(shape) * 5) + 1, 0).astype(np.float32)
    img.setflags(write=False)
    return img
