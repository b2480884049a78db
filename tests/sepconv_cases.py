"""Cases and a plain reference shared by tests/test_gpu_sepconv_edges.py (the separable
convolution passes of csrc/sepconv.hip at their tile seams, at every tap count and on
every dispatch route) and tests/test_sepconv_premises_cpu.py (the properties of these
cases that the GPU tests rely on, proved on the CPU alone).

Conventions of the library: volumes [z, y, x] float32; ``axis`` 0 = x, 1 = y, 2 = z
(array axis 2 - axis); ``mode`` is the native out-of-bounds code (csrc/sepconv.hpp:
0 zero, 1 value, 2 border, 3 mirror single); kernels are listed (x, y, z).
"""
from __future__ import annotations

import functools

import numpy as np

ZERO, VALUE, BORDER, MIRROR = 0, 1, 2, 3
MODES = (ZERO, VALUE, BORDER, MIRROR)
MODE_NAMES = {ZERO: "zero", VALUE: "value", BORDER: "border", MIRROR: "mirror"}   # oracle/dog_ref.py's names
OOB_VALUE = 0.25
TAP_COUNTS = (7, 15, 31, 63, 127)
U = 2.0 ** -24    # unit roundoff of float32


# ------------------------------------------------------------------ the reference
def source_index(i, n, mode):
    """(src, outside) for positions ``i`` (any integers) of an axis of length ``n``:
    the index the pass reads, and where it takes the mode's constant instead.  Mirror
    single is the triangle wave of period 2 (n - 1), written as a distance from the
    far end so that it shares no formula with the kernels or the oracle."""
    i = np.asarray(i, np.int64)
    outside = (i < 0) | (i >= n)
    if mode == BORDER:
        return np.minimum(np.maximum(i, 0), n - 1), np.zeros_like(outside)
    if mode == MIRROR:
        if n == 1:
            return np.zeros_like(i), np.zeros_like(outside)
        return (n - 1) - np.abs(np.mod(i, 2 * (n - 1)) - (n - 1)), np.zeros_like(outside)
    assert mode in (ZERO, VALUE), mode
    return np.where(outside, 0, i), outside


def _operands(img, K, axis, mode, value, dtype):
    """Yields the K operand volumes v_j = in[ext(i + j - r)] as ``dtype``."""
    img = np.asarray(img, np.float32)
    ax = 2 - axis
    n = img.shape[ax]
    fill = dtype(value if mode == VALUE else 0.0)
    shape = [1, 1, 1]
    shape[ax] = n
    for j in range(K):
        src, outside = source_index(np.arange(n) + j - K // 2, n, mode)
        v = np.take(img, src, axis=ax).astype(dtype)
        if outside.any():
            v = np.where(outside.reshape(shape), fill, v)
        yield v


def ref_pass(img, taps, axis, mode, value=0.0):
    """out[i] = sum_j in[ext(i + j - r)] * k[j], r = K // 2: float32 products added in
    float32 in tap order j = 0 .. K - 1 onto +0, every tap visited (the zero ones too)."""
    taps = np.asarray(taps, np.float32)
    acc = np.zeros(np.shape(img), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for v, k in zip(_operands(img, len(taps), axis, mode, value, np.float32), taps):
            acc = acc + v * k
    assert acc.dtype == np.float32
    return acc


def ref_pass64(img, taps, axis, mode, value=0.0):
    """(the same sum in float64, sum_j |v_j k_j| in float64).  float32 operands have
    exact float64 products."""
    taps = np.asarray(taps, np.float32).astype(np.float64)
    acc = np.zeros(np.shape(img), np.float64)
    mag = np.zeros(np.shape(img), np.float64)
    for v, k in zip(_operands(img, len(taps), axis, mode, np.float32(value), np.float64), taps):
        acc += v * k
        mag += np.abs(v * k)
    return acc, mag


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u) for float32."""
    return k * U / (1 - k * U)


def pass_bound(K, mag):
    """|float32 sequential sum of K rounded products - exact| <= gamma_(K + 1) * sum |v k|:
    K - 1 effective additions (the first is onto 0) and one rounding per product, bounded by K + 1
    roundings per term."""
    return gamma(K + 1) * mag


def ref3d(img, kernels_xyz, mode, value=0.0, on=(True, True, True)):
    """The passes x, then y, then z, for the axes switched on."""
    out = np.asarray(img, np.float32)
    for axis in range(3):
        if on[axis]:
            out = ref_pass(out, kernels_xyz[axis], axis, mode, value)
    return out


# ------------------------------------------------------------------ inputs
def volume(shape, seed):
    """Uniform float32 noise in [-1, 1), [z, y, x], read-only.  Zero mean: under positive
    taps a mean would dominate every output and hide reversed taps behind it (rel-L2 of
    the reversed-tap reference at 31 taps: 0.008 on [0, 1) noise)."""
    img = np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(2) - np.float32(1)
    img.setflags(write=False)
    return img


def random_taps(K, seed):
    """Three kernels (x, y, z) of K positive taps, rng.random(K) + 0.05: asymmetric and
    different per axis, so reversed taps, swapped axes and swapped kernels all show."""
    rng = np.random.default_rng(seed)
    return [(rng.random(K) + 0.05).astype(np.float32) for _ in range(3)]


@functools.lru_cache(maxsize=None)
def expected(shape, seed, K, tap_seed, mode, on=(True, True, True)):
    """ref3d of volume(shape, seed) under random_taps(K, tap_seed), read-only, computed once."""
    out = ref3d(volume(shape, seed), random_taps(K, tap_seed), mode, OOB_VALUE, on)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ a. every tap count, every mode
# (nz, ny, nx) = (70, 9, 257): two 256-column x blocks (the last holds one column), two
# 8-row groups (the last holds one row), two 64-plane z tiles (the last holds 6 planes:
# cut inside the first thread's run of 16 outputs), five 64-column tiles of the y / z
# passes (the last holds one column)
ALL_TAPS_SHAPE, ALL_TAPS_SEED = (70, 9, 257), 101
ALL_TAPS_CASES = [(K, mode) for K in TAP_COUNTS for mode in MODES]


def all_taps_seed(K):
    return 1000 + K


# ------------------------------------------------------------------ b. the seams of each kernel
# x blocks of 256 columns: nx = 255, 256, 257, 513 with ny = 8 (one full row group) and
# ny = 17 (two and one row); y / z tiles of 64 positions: 63, 64, 65, 129 along y and
# along z; 64-column tiles: nx = 63, 64, 65.  Every value occurs in one of these volumes:
#   nx 255 (63, 64, 255)   256 (64, 63, 256)   257 (17, 17, 257)   513 (65, 8, 513)
#      63 (129, 17, 63)     64 (5, 65, 64)      65 (9, 129, 65)
#   ny 8 (65, 8, 513)   17 (129, 17, 63)   63 (64, 63, 256)   64 (63, 64, 255)
#      65 (5, 65, 64)   129 (9, 129, 65)
#   nz 63 (63, 64, 255)   64 (64, 63, 256)   65 (65, 8, 513)   129 (129, 17, 63)
# and ny = 8 and ny = 17 each meet a multi-block nx (513, 257)
SEAM_SHAPES = [(65, 8, 513), (9, 129, 65), (129, 17, 63), (64, 63, 256), (63, 64, 255), (5, 65, 64),
               (17, 17, 257)]
SEAM_TAPS = (15, 31)           # the register-window form and the loop form of k_sep_yz
SEAM_MODES = (BORDER, MIRROR)
SEAM_SEED = 202


# ------------------------------------------------------------------ c. axes shorter than the reach
SHORT_CASES = [((1, 2, 300), 127), ((2, 1, 3), 63), ((1, 1, 1), 7)]
SHORT_SEED = 303


# ------------------------------------------------------------------ d. the per-axis switches
SWITCH_SHAPE, SWITCH_SEED, SWITCH_TAPS, SWITCH_TAP_SEED = (9, 17, 65), 404, 15, 1404
SWITCHES = [(True, False, False), (False, True, False), (False, False, True), (True, True, False),
            (True, False, True), (False, True, True), (False, False, False)]
GAUSS_2D_DIM, GAUSS_1D_DIM = [300, 70], [300]      # (x, y) and (x): legacy.gauss's h = 1 / d = 1
GAUSS_2D_SIGMA, GAUSS_1D_SIGMA = [2.0, 4.5], [1.7]   # 31 taps, 15 taps
GAUSS_SEED = 405


# ------------------------------------------------------------------ e. the grid-stride fallback
# (w, h, d): nz = 65536 > 65535 sends the x and y passes to k_sep_pass<1> (z stays tiled:
# 1024 tiles); ny = 65536 sends the x pass (grid y) and the z pass (grid z) there (y tiled)
FALLBACK_WHD = [(2, 1, 65536), (1, 65536, 2)]
FALLBACK_TAPS = (15, 63)
FALLBACK_MODES = (VALUE, BORDER, MIRROR)
FALLBACK_SEED = 505
GRID_LIMIT = 65535


def tiled(whd, axis):
    """sep_pass's dispatch condition (csrc/sepconv.hip): the tiled kernels serve a pass
    whose grid y / z extents stay within 65535 (n < 2^31 here)."""
    w, h, d = whd
    tl = 1 if axis == 0 else -(-(h if axis == 1 else d) // 64)
    oth = d if axis in (0, 1) else h
    return (h if axis == 0 else tl) <= GRID_LIMIT and oth <= GRID_LIMIT


# ------------------------------------------------------------------ f. / g. the unfused DoG routes
# dog.hip fuses 7 / 15 / 31 taps unless nz > 65535 or ny > 65535 * 32
DOG_TALL_SHAPE, DOG_TALL_SEED = (65536, 3, 3), 626
DOG_TALL_SIGMAS = [(1.0, 7), (1.8, 15), (8.0, 63)]
DOG_LONG_SHAPE, DOG_LONG_SEED = (1, 65535 * 32 + 1, 1), 607
DOG_127_SHAPE, DOG_127_SEED, DOG_127_SIGMA = (70, 20, 150), 722, 12.0
DOG_REFUSED_SIGMA = 18.0


def dog_taps(sigma):
    """The padded length both Gaussians of a DoG at ``sigma`` run at."""
    from oracle import dog_ref
    s1, s2, _, _ = dog_ref.dog_sigmas(sigma, (0.5, 0.5, 0.5))
    k1, k2 = dog_ref.cuda_kernels(s1), dog_ref.cuda_kernels(s2)
    if k1 is None or k2 is None:
        return None
    return max(len(k1[0]), len(k2[0]))


# ------------------------------------------------------------------ h. non-finite input
NONFINITE_SHAPE, NONFINITE_SEED = (20, 22, 24), 809
NONFINITE_SIGMAS = [1.0, 1.7, 1.2]     # 7-, 11- and 9-tap Gaussians padded to 15: genuine zero taps
NONFINITE_NAN_AT, NONFINITE_INF_AT = (10, 11, 12), (4, 17, 5)


def nonfinite_volume():
    img = volume(NONFINITE_SHAPE, NONFINITE_SEED).copy()
    img[NONFINITE_NAN_AT] = np.nan
    img[NONFINITE_INF_AT] = np.inf
    img.setflags(write=False)
    return img
