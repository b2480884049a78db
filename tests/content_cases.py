"""Cases and an operation-order restatement shared by tests/test_gpu_content_edges.py (the
passes of csrc/content_weights.hip at their tile seams, at the edges of the tap chunking,
at the limits of the min / max reduction and on non-finite input) and
tests/test_content_premises_cpu.py (the properties of the restatement and of these cases
that the GPU tests rely on, proved on the CPU alone).

The restatement computes what the kernels compute, operation by operation, in float32:
six 1-D passes of correctly rounded fused multiply-adds in tap order over the mirror-single
extension, one subtraction and one multiplication between the two blurs, and
FusionHelper.normalizeImage (tests/content_ref.normalize_image: one subtraction, one
division).  It shares no code with the kernels and none with content_ref's FFT path.

Conventions of the library: volumes [z, y, x] float32; ``axis`` 0 = x, 1 = y, 2 = z (array
axis 2 - axis); sigmas are listed (x, y, z).
"""
from __future__ import annotations

import concurrent.futures
import functools
from typing import NamedTuple

import numpy as np

import content_ref as cr
from oracle.dog_ref import gaussian_kernel_1d

U = 2.0 ** -24    # unit roundoff of float32

# the tiling of csrc/content_weights.hip that the cases straddle
# (test_gpu_content_edges.test_tile_sizes_are_the_ones_the_cases_straddle holds the library to it)
TILE = 128         # kCwTile: outputs per line and block along the pass axis
LINES = 64         # kCwLines: lines per block
CHUNK = 16         # kCwChunk: taps per register-window step; taps are zero-padded to a multiple
MAX_TAPS = 463     # kCwMaxTaps
RED_BLOCK = 256    # kRedBlock
RED_ROUND = 1024 * RED_BLOCK    # kRedGrid * kRedBlock: voxels per round of the grid stride


# ------------------------------------------------------------------ the restatement
def fma32(a, b, c):
    """The correctly rounded float32 fused multiply-add round(a * b + c), elementwise.

    The float64 product of two float32 values is exact (48 bits).  It is added to c in
    float64 with the TwoSum error term; where the sum was inexact and its last mantissa bit
    is even, it is moved one float64 ulp towards the error: the sum rounded to odd.  53 >=
    2 * 24 + 2 bits, so rounding that to float32 rounds the exact value once."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.atleast_1d(a.astype(np.float64) * b.astype(np.float64))
        c64 = c.astype(np.float64)
        s = p + c64
        t = s - p                                  # TwoSum (Knuth): s + err == p + c exactly
        err = (p - (s - t)) + (c64 - t)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        if fix.any():
            np.copyto(s, np.nextafter(s, np.copysign(np.inf, err)), where=fix)
        return s.astype(np.float32).reshape(np.broadcast_shapes(a.shape, b.shape, c.shape))


def taps(sigma):
    """The float32 casts of Util.createGaussianKernel1DDouble(sigma, true): K = max(3,
    2 * int(3 sigma + 0.5) + 1) taps."""
    return gaussian_kernel_1d(float(sigma), True).astype(np.float32)


def sigma_for_taps(K):
    """A sigma whose kernel has exactly K (odd) taps: 3 sigma = (K - 1) / 2, in the middle
    of the interval that the rule int(3 sigma + 0.5) maps to (K - 1) / 2."""
    assert K % 2 == 1 and K >= 3
    return ((K - 1) / 2) / 3


def mirror_index(i, n):
    """The index extendMirrorSingle reads at positions ``i`` (any integers) of an axis of
    length ``n``: the triangle wave of period 2 (n - 1), written as a distance from the far
    end.  One sample: index 0."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    return (n - 1) - np.abs(np.mod(i, 2 * (n - 1)) - (n - 1))


_BLOCK = 1 << 15      # elements per block of lines: the float64 temporaries stay in cache


def _extended_lines(img, K, axis, source, dtype=np.float32):
    """(ext [n + K - 1, lines], n, the moved shape): the volume as lines along ``axis``,
    extended by the reach K // 2 at both ends through ``source``."""
    moved = np.moveaxis(np.asarray(img, dtype), 2 - axis, 0)
    n = moved.shape[0]
    lines = moved.reshape(n, -1)
    r = K // 2
    return lines[source(np.arange(-r, n + r), n)], n, moved.shape


def ref_pass(img, sigma, axis, *, k=None, fma=fma32, source=mirror_index, keep=None):
    """out[i] = sum_j in[mirror(i + j - K // 2)] * k[j] as the kernel forms it:
    acc = fma32(in[..], k[j], acc) for j = 0 .. K - 1, starting from +0.

    The keyword arguments are for the mutants of the premises: other taps ``k``, another
    multiply-add, another index rule, and ``keep(i, s)`` -> bool per output position i and
    unextended source position s = i + j - K // 2: operands it refuses count as 0."""
    k = taps(sigma) if k is None else np.asarray(k, np.float32)
    K = len(k)
    ext, n, moved_shape = _extended_lines(img, K, axis, source)
    out = np.empty((n, ext.shape[1]), np.float32)
    i = np.arange(n)
    step = max(1, _BLOCK // n)

    def block(c0):
        e = ext[:, c0:c0 + step]
        acc = np.zeros((n, e.shape[1]), np.float32)
        for j in range(K):
            v = e[j:j + n]
            if keep is not None:
                v = np.where(keep(i, i + j - K // 2)[:, None], v, np.float32(0))
            acc = fma(v, k[j], acc)
        out[:, c0:c0 + step] = acc

    starts = range(0, ext.shape[1], step)
    if len(starts) > 1:      # blocks of lines are independent: numpy releases the GIL
        with concurrent.futures.ThreadPoolExecutor(4) as pool:
            list(pool.map(block, starts))
    else:
        block(0)
    return np.ascontiguousarray(np.moveaxis(out.reshape(moved_shape), 0, 2 - axis))


def ref_pass64(img, sigma, axis):
    """(the same sum in float64, sum_j |v_j k_j| in float64) of one pass over ``img`` (cast
    to float64: float32 operands have exact float64 products)."""
    k = taps(sigma).astype(np.float64)
    K = len(k)
    ext, n, moved_shape = _extended_lines(img, K, axis, mirror_index, np.float64)
    acc = np.zeros((n, ext.shape[1]))
    mag = np.zeros((n, ext.shape[1]))
    for j in range(K):
        p = ext[j:j + n] * k[j]
        acc += p
        mag += np.abs(p)
    back = lambda a: np.ascontiguousarray(np.moveaxis(a.reshape(moved_shape), 0, 2 - axis))
    return back(acc), back(mag)


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u) for float32."""
    return k * U / (1 - k * U)


def pass_bound(K, mag):
    """|float32 tap-order sum of K terms - exact| <= gamma_(K + 1) * sum |v k|, as
    sepconv_cases.pass_bound derives for rounded products added in float32 (K + 1 roundings
    per term at most); fused multiply-adds round each term once less and stay inside."""
    return gamma(K + 1) * mag


def ref_raw(img, s1, s2, one_pass=ref_pass, trace=None):
    """The un-normalised weights: passes x, y, z with s1; d = c - img and c = d * d in
    float32; passes x, y, z with s2.  ``trace``: a list that receives every intermediate."""
    img = np.asarray(img, np.float32)
    note = (lambda a: None) if trace is None else trace.append
    c = img
    for axis in range(3):
        c = one_pass(c, s1[axis], axis)
        note(c)
    with np.errstate(invalid="ignore", over="ignore"):
        d = c - img
        c = d * d
    assert d.dtype == np.float32 and c.dtype == np.float32
    note(d)
    note(c)
    for axis in range(3):
        c = one_pass(c, s2[axis], axis)
        note(c)
    return c


def ref_weights(img, s1, s2, one_pass=ref_pass):
    """ref_raw, then normalizeImage: (c - min) / (max - min) in float32, skipped when the
    range is NaN, infinite or 0."""
    return cr.normalize_image(ref_raw(img, s1, s2, one_pass))


def ref_raw64(img, s1, s2):
    """(the same sums in float64 throughout, [sum |v k| of each of the six passes])."""
    img = np.asarray(img, np.float64)
    mags = []
    c = img
    for axis in range(3):
        c, m = ref_pass64(c, s1[axis], axis)
        mags.append(m)
    c = (c - img) ** 2
    for axis in range(3):
        c, m = ref_pass64(c, s2[axis], axis)
        mags.append(m)
    return c, mags


# ------------------------------------------------------------------ inputs
def volume(shape, seed, beads=3, bead_at=None):
    """Uniform float32 noise in [-1, 1) plus ``beads`` single-voxel beads of height 6, 7, ..
    at random places and, with ``bead_at``, one of height 40 there; [z, y, x], read-only.
    Zero mean: under positive taps a mean would dominate every blurred value and hide a
    wrong tap behind it.  Magnitudes of order 1 keep every intermediate (a second
    difference of the noise, squared, blurred) far above the subnormal range; the premises
    check that."""
    rng = np.random.default_rng(seed)
    img = rng.random(shape, dtype=np.float32) * np.float32(2) - np.float32(1)
    for b in range(beads):
        at = tuple(int(rng.integers(0, s)) for s in shape)
        img[at] += np.float32(6 + b)
    if bead_at is not None:
        img[bead_at] = np.float32(40)
    img.setflags(write=False)
    return img


class Case(NamedTuple):
    shape: tuple      # (nz, ny, nx)
    s1: tuple         # (x, y, z)
    s2: tuple
    seed: int
    bead_at: tuple = None


def _taps3(kx, ky, kz):
    return tuple(sigma_for_taps(K) for K in (kx, ky, kz))


CASES: dict = {}

# ---- a. the seams of each pass: 1, 2, one short of, exactly, one past and twice past the
# 128-output tile along one axis; the x pass over 13 * 5 = 65 rows (two 64-line blocks, the
# last holds one row), the y and z passes over nx = 65 (two 64-column blocks, the last
# holds one column) and 3 along the third axis.  Sigma 3 and 6: 19 taps (kpad 32: one loop
# turn, no tail) and 37 taps (kpad 48: one loop turn and the tail)
SEAM_LENGTHS = (1, 2, 127, 128, 129, 257)
SEAM_S1, SEAM_S2 = (3.0, 3.0, 3.0), (6.0, 6.0, 6.0)
SEAM_TAPS = (19, 37)


def seam_shape(axis, n):
    return [(5, 13, n), (3, n, 65), (n, 3, 65)][axis]


def seam_name(axis, n):
    return f"seam_{'xyz'[axis]}_{n}"


for _axis in range(3):
    for _n in SEAM_LENGTHS:
        CASES[seam_name(_axis, _n)] = Case(seam_shape(_axis, _n), SEAM_S1, SEAM_S2, 1000 + 10 * _n + _axis)
# all three axes past a seam at once: (nz, ny, nx) = (130, 131, 129)
CASES["seam_all"] = Case((130, 131, 129), SEAM_S1, SEAM_S2, 1999)

# ---- b. the tap chunking: 3 (the minimum) and 5 taps, and one tap short of / past 16, 32
# and 48 (kpad 16, 32, 32, 48, 48, 64: the tail alone; one turn; one turn and the tail; two
# turns).  Rotation r puts TAP_COUNTS[(r + slot) % 8] into slot (s1x, s1y, s1z, s2x, s2y, s2z):
# six different counts per case, every count once in every slot over the eight rotations.
# (21, 37, 140): two x tiles; the reach of 49 taps (24) folds over the 21 planes
TAP_COUNTS = (3, 5, 15, 17, 31, 33, 47, 49)
TAPS_SHAPE = (21, 37, 140)


def rotation_taps(r):
    return [TAP_COUNTS[(r + slot) % len(TAP_COUNTS)] for slot in range(6)]


for _r in range(len(TAP_COUNTS)):
    _K = rotation_taps(_r)
    CASES[f"taps_r{_r}"] = Case(TAPS_SHAPE, _taps3(*_K[:3]), _taps3(*_K[3:]), 2000 + _r)
# the longest kernel, 463 taps = 29 chunks (14 turns and the tail), the largest LDS request
# (x pass: 64 x 593 floats), on every axis of one blur; reach 231 over 6, 7 and 140 samples
MAX_SHAPE = (6, 7, 140)
CASES["taps_max_s2"] = Case(MAX_SHAPE, _taps3(3, 3, 3), _taps3(MAX_TAPS, MAX_TAPS, MAX_TAPS), 2100)
CASES["taps_max_s1"] = Case(MAX_SHAPE, _taps3(MAX_TAPS, MAX_TAPS, MAX_TAPS), _taps3(3, 3, 3), 2101)

# ---- c. the reduction: fewer voxels than one block of 256 (1: range 0, normalisation
# skipped); 266,175 = 262,144 + 4,031 voxels, 191 of them past the last whole block, the
# maximum among those; 528,320 voxels, the minimum in the second round of the grid stride
RED_SIGMA = _taps3(3, 3, 3)
CASES["red_1"] = Case((1, 1, 1), RED_SIGMA, RED_SIGMA, 3001)
CASES["red_2"] = Case((1, 1, 2), RED_SIGMA, RED_SIGMA, 3002)
CASES["red_30"] = Case((2, 3, 5), RED_SIGMA, RED_SIGMA, 3030)
CASES["red_tail"] = Case((63, 65, 65), RED_SIGMA, RED_SIGMA, 3100, (62, 64, 64))
CASES["red_second_round"] = Case((127, 65, 64), RED_SIGMA, RED_SIGMA, 3200)

# ---- d. non-finite input: one NaN or one +inf at the centre of 70^3, 3-tap kernels
# (R1 = R2 = 1).  Certainly non-finite: the box of half-width R1 + R2 around it.  Possibly
# NaN: up to CHUNK - 1 further positions per pass (zero padded taps times a non-finite
# value), so certainly clean: outside the box of half-width R1 + R2 + 2 (CHUNK - 1) = 32
NONFINITE_AT = (35, 35, 35)
NONFINITE_INNER = 2
NONFINITE_OUTER = NONFINITE_INNER + 2 * (CHUNK - 1)
CASES["nonfinite"] = Case((70, 70, 70), RED_SIGMA, RED_SIGMA, 4000)


def nonfinite_volume(value):
    img = image("nonfinite").copy()
    img[NONFINITE_AT] = value
    img.setflags(write=False)
    return img


def box(shape, at, half):
    """Boolean volume: the voxels within ``half`` of ``at`` along every axis."""
    grids = np.meshgrid(*[np.abs(np.arange(n) - a) <= half for n, a in zip(shape, at)], indexing="ij")
    return grids[0] & grids[1] & grids[2]


# ------------------------------------------------------------------ shared, computed once
@functools.lru_cache(maxsize=None)
def image(name):
    c = CASES[name]
    return volume(c.shape, c.seed, bead_at=c.bead_at)


@functools.lru_cache(maxsize=None)
def raw(name):
    c = CASES[name]
    out = ref_raw(image(name), c.s1, c.s2)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def weights(name):
    out = cr.normalize_image(raw(name))
    out.setflags(write=False)
    return out
