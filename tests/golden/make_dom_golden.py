"""Generates tests/golden/dom.npz: a small bead volume, its Difference-of-Mean image and
its ordered peaks at the reference's defaults (radii 2 / 3, threshold 0.02, image sigma
0.5: boxes of 5 and 7), computed WITHOUT an integral image -- the box sums are plain sums
of shifted copies of the (int) volume -- so that tests/dom_ref.py (prefix sums and eight
corner reads, as the reference) is checked against an independent evaluation.

    python tests/golden/make_dom_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def bead_volume(shape=(24, 28, 32), nbeads=9, seed=31):
    """Gaussian beads on a noisy background, [z, y, x] float32 with fractional values."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    img = 100.0 + 6.0 * rng.standard_normal(shape)
    for _ in range(nbeads):
        c = [rng.uniform(4, n - 5) for n in shape]
        img += rng.uniform(600, 1500) * np.exp(-((z - c[0]) ** 2 / 5.0 + (y - c[1]) ** 2 / 3.0 + (x - c[2]) ** 2 / 3.0))
    return img.astype(np.float32)


def box_sum(v, size):
    """Sum of v over the box of `size` (z, y, x diameters) centred on each voxel that has
    the whole box: shifted copies added up, int64."""
    nz, ny, nx = v.shape
    sz, sy, sx = size
    out = np.zeros((nz - sz + 1, ny - sy + 1, nx - sx + 1), np.int64)
    for dz in range(sz):
        for dy in range(sy):
            for dx in range(sx):
                out += v[dz:dz + out.shape[0], dy:dy + out.shape[1], dx:dx + out.shape[2]]
    return out


def dom(img, s1=5, s2=7):
    v = np.trunc(img.astype(np.float64)).astype(np.int64)     # (in range, no NaN: a plain (int))
    h1, h2 = s1 // 2, s2 // 2
    hm = max(h1, h2)
    crop = lambda a, h: a[hm - h:a.shape[0] - (hm - h), hm - h:a.shape[1] - (hm - h), hm - h:a.shape[2] - (hm - h)]
    sum1, sum2 = crop(box_sum(v, (s1,) * 3), h1), crop(box_sum(v, (s2,) * 3), h2)
    diff = np.float32(img.max()) - np.float32(img.min())
    d1, d2 = np.float32(s1 ** 3) * diff, np.float32(s2 ** 3) * diff
    out = np.zeros(img.shape, np.float32)
    out[hm:-hm, hm:-hm, hm:-hm] = sum2.astype(np.float32) / d2 - sum1.astype(np.float32) / d1
    return out


def main():
    from oracle import dog_ref
    img = bead_volume()
    d = dom(img)
    peaks = dog_ref.find_peaks(d, float(np.float32(0.02)), 8)
    pk = np.array([(p[0], p[1], p[2], int(p[4]), int(p[5])) for p in peaks], np.int32).reshape(-1, 5)
    np.savez_compressed(os.path.join(HERE, "dom.npz"), img=img, dom=d, peaks=pk,
                        intensity=np.float32([p[3] for p in peaks]))
    print(f"{len(peaks)} peaks ({int(pk[:, 4].sum())} maxima)")


if __name__ == "__main__":
    sys.exit(main())
