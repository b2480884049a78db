"""Generates tests/golden/content_based.npz: content-based fusion weights of a small
view computed WITHOUT the FFT oracle -- a direct float64 sum over the 3-D kernel
float(kx * ky * kz) with explicit extendMirrorSingle index tables -- so that
tests/content_ref.py (composed from the oracle's FFT convolution) is checked against
an independent evaluation of ContentBased.approximateEntropy.

    python tests/golden/make_content_golden.py
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def gauss1d(sigma):
    """Util.createGaussianKernel1DDouble(sigma, true)."""
    size = max(3, 2 * int(3 * sigma + 0.5) + 1)
    c = size // 2
    g = [0.0] * size
    for x in range(c + 1):
        g[c - x] = g[c + x] = math.exp(-(x * x) / (2 * sigma * sigma))
    s = 0.0
    for v in g:
        s += v
    return [v / s for v in g]


def mirror(i, n):
    if n == 1:
        return 0
    p = 2 * (n - 1)
    j = i % p
    return p - j if j >= n else j


def blur(img, sigma_xyz):
    """out[z, y, x] = sum_k E(img)[z + cz - kz, ...] * float(kx * ky * kz), float32 result."""
    kx, ky, kz = (gauss1d(s) for s in sigma_xyz)
    nz, ny, nx = img.shape
    a = img.astype(np.float64)
    acc = np.zeros(img.shape)
    for iz, vz in enumerate(kz):
        zi = [mirror(z + len(kz) // 2 - iz, nz) for z in range(nz)]
        for iy, vy in enumerate(ky):
            yi = [mirror(y + len(ky) // 2 - iy, ny) for y in range(ny)]
            for ix, vx in enumerate(kx):
                xi = [mirror(x + len(kx) // 2 - ix, nx) for x in range(nx)]
                tap = float(np.float32(1.0 * vx * vy * vz))
                acc += a[np.ix_(zi, yi, xi)] * tap
    return acc.astype(np.float32)


def weights(img, s1, s2):
    c = blur(img, s1)
    d = (c - img).astype(np.float32)
    c = blur((d * d).astype(np.float32), s2)
    mn, mx = np.float32(c.min()), np.float32(c.max())
    diff = np.float32(mx - mn)
    if np.isnan(diff) or np.isinf(diff) or diff == 0:
        return c
    return ((c - mn).astype(np.float32) / diff).astype(np.float32)


def main():
    rng = np.random.default_rng(20)
    z, y, x = np.meshgrid(np.arange(5), np.arange(9), np.arange(11), indexing="ij")
    img = (40 * np.exp(-((x - 7) ** 2 + (y - 3) ** 2 + (z - 2) ** 2) / 6.0) + 10 * rng.random((5, 9, 11)) + 1)
    img = img.astype(np.float32)
    s1, s2 = (1.2, 1.0, 0.8), (2.0, 1.5, 2.5)   # z: 17 taps on 5 planes, a multi-fold mirror
    flat = np.full((3, 4, 5), 7.25, np.float32)
    np.savez_compressed(os.path.join(HERE, "content_based.npz"), img=img, sigma1=np.array(s1), sigma2=np.array(s2),
                        weights=weights(img, s1, s2), flat=flat, flat_weights=weights(flat, s1, s2))


if __name__ == "__main__":
    sys.exit(main())
