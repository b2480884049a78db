"""Cases and builders shared by tests/test_gpu_autobbox_edges.py (the minimum filter, the
min / max reduction and the box of csrc/autobbox.hip and csrc/minmax.hpp at their tile seams,
at the edges of the doubling scheme, on special values and over stale workspace buffers) and
tests/test_autobbox_premises_cpu.py (what those tests rely on, proved on the CPU alone).

Expected results are tests/autobbox_ref.py's throughout, bit for bit.  ``tiled_pass`` restates
one pass the way k_minfilter evaluates it (tiles with a halo, doubling, the 4-wide loop with
its remainder, the overlap shift); it is there for the premises' mutants only, never as an
expected value.

Conventions of the library: volumes [z, y, x] float32; ``axis`` 0 = x, 1 = y, 2 = z (array
axis 2 - axis); boxes, dims and positions are (x, y, z).
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import autobbox_ref as ar

# the tiling of csrc/autobbox.hip and csrc/minmax.hpp that the cases straddle
# (test_gpu_autobbox_edges.test_tile_sizes_are_the_ones_the_cases_straddle holds the library to it)
LINES = 64           # kMfLines: lines per block
TILE_SMALL = 64      # kMfTileSmall: outputs per line and block, radius <= SMALL_RADIUS
TILE_LARGE = 128     # kMfTileLarge: above it
SMALL_RADIUS = 16    # kMfSmallRadius
RED_BLOCK = 256      # kRedBlock
RED_GRID = 1024      # kRedGrid
ROUND = RED_GRID * RED_BLOCK        # voxels per round of the reduction's grid stride
BOX_ROUND = 2048 * RED_BLOCK        # the same of k_threshold_box (its launch in threshold_bounds)
UNROLL = 4           # the doubling levels' inner loop


def tile_of(r):
    return TILE_SMALL if r <= SMALL_RADIUS else TILE_LARGE


def doubling(r):
    """(levels, p, shift) of radius r: the window w = 2r + 1 is the union of two windows of
    p = 2^levels <= w, the second ``shift`` = w - p after the first."""
    w = 2 * r + 1
    levels = w.bit_length() - 1
    return levels, 1 << levels, w - (1 << levels)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ one pass, as the kernel tiles it
def tiled_pass(lines, r, tile=None, *, left_short=False, right_short=False, zero_halo=False, shift_off=0,
               skip_remainder=False):
    """The window minimum along axis 0 of ``lines`` [n] or [n, lines] as k_minfilter forms it:
    per tile of ``tile`` outputs the positions p0 - r .. p0 + tile + r - 1 are staged (zeros
    outside the image), m_2k[i] = min(m_k[i], m_k[i + k]) in place for i < cnt = P - 2k + 1 (the
    first cnt - cnt % 4 by the unrolled loop, the rest by the remainder loop), and
    out[i] = min(FLOAT_MAX, min(m_p[i], m_p[i + shift])).

    The keyword arguments are the premises' mutants: the first / last staged position of a
    tile dropped where it belongs to a neighbouring tile (a window one short on the left /
    right of a seam), the halo that belongs to neighbouring tiles replaced by zeros, the
    overlap shift moved by ``shift_off``, the remainder loop left out."""
    a = np.asarray(lines, np.float32)
    n = a.shape[0]
    tile = tile_of(r) if tile is None else tile
    _, p, sh = doubling(r)
    out = np.empty_like(a)
    for p0 in range(0, n, tile):
        t = min(tile, n - p0)
        P = t + 2 * r
        pos = np.arange(p0 - r, p0 + t + r)
        inside = (pos >= 0) & (pos < n)
        m = np.zeros((P,) + a.shape[1:], np.float32)
        m[inside] = a[pos[inside]]
        if zero_halo:
            m[(pos < p0) | (pos >= p0 + t)] = 0
        if left_short and p0 > 0:
            m[0] = ar.FLOAT_MAX
        if right_short and p0 + t < n:
            m[P - 1] = ar.FLOAT_MAX
        k = 1
        while 2 * k <= 2 * r + 1:
            cnt = P - 2 * k + 1
            done = cnt - cnt % UNROLL if skip_remainder else cnt
            if done > 0:          # ascending and in place: i + k is read before it is written
                m[:done] = ar.jmin(m[:done], m[k:k + done])
            k *= 2
        assert k == p
        s = sh + shift_off
        out[p0:p0 + t] = ar.jmin(ar.FLOAT_MAX, ar.jmin(m[:t], m[s:s + t]))
    return out


def window_min(line, r):
    """ar.min_filter_axis (whose axis is the array's) on one line"""
    return ar.min_filter_axis(np.asarray(line, np.float32).reshape(1, 1, -1), r, 2).reshape(-1)


# ------------------------------------------------------------------ additive images
# img[z, y, x] = a[x] + b[y] + c[z], every term a multiple of 2^-10 in [-1, -2^-10]: every sum is
# exact and negative, the zero extension never wins, and the filtered image is
# minwin(a)[x] + minwin(b)[y] + minwin(c)[z] (test_autobbox_premises_cpu.test_additive_*): every
# output voxel shows the window of every axis, so no pass hides behind another.
GRID = np.float32(2.0 ** -10)


def random_profile(n, rng):
    """n different multiples of 2^-10 in [-1, -2^-10] (n <= 1024), in random order"""
    return -(rng.permutation(1024)[:n] + 1).astype(np.float32) * GRID


def zigzag_profile(n, tile, rng, rising_first=False):
    """A triangle wave of period 2 * tile with its turning points in the middle of the tiles,
    strictly monotone between them and jittered: the first seam (position tile) lies on a
    falling slope, the second on a rising one, and so on (``rising_first``: the other way
    round).  On a falling slope the minimum of every window is its last element, on a rising
    one its first: a window that is one short, or that lost its halo, at a seam is wrong
    there for sure, not with probability 1 / w.  tile + 1 steps of 7 (tile 128) or 15 (tile
    64) levels of 2^-10 fit [-1, -2^-10]."""
    gain = 1024 // (tile + 1)
    i = np.arange(n) + (tile if rising_first else 0)
    tri = np.abs((i + tile // 2) % (2 * tile) - tile)            # 0 at 0.5 tile, tile at 1.5 tile
    depth = gain * tri + rng.integers(0, gain, n) + 1               # values fall from 0.5 to 1.5 tile
    assert depth.min() >= 1 and depth.max() <= 1024
    return -depth.astype(np.float32) * GRID


def additive(a, b, c):
    img = (c[:, None, None] + b[None, :, None]) + a[None, None, :]
    assert img.dtype == np.float32
    return img


class Sweep(NamedTuple):
    axis: int           # the pass whose seams the case straddles
    r: int
    n: int              # the length along that axis
    rising_first: bool = False

    @property
    def name(self):
        return f"{'xyz'[self.axis]}-r{self.r}-n{self.n}"

    @property
    def shape(self):
        """(nz, ny, nx): across the pass axis two line groups, the second partial -- 5 * 13 =
        65 rows for the x pass, nx = 66 for the y and z passes -- and 3 along the third axis"""
        return [(5, 13, self.n), (3, self.n, 66), (self.n, 3, 66)][self.axis]


RADII = (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64)
# r -> (tile, levels, shift): the shift's extremes 1 (r = 2^j) and p - 1 (r = 2^j - 1), a level
# more from 2^j - 1 to 2^j, the switch of the tile between 16 and 17
RADIUS_CLASSES = {1: (64, 1, 1), 2: (64, 2, 1), 3: (64, 2, 3), 4: (64, 3, 1), 7: (64, 3, 7), 8: (64, 4, 1),
                  15: (64, 4, 15), 16: (64, 5, 1), 17: (128, 5, 3), 31: (128, 5, 31), 32: (128, 6, 1),
                  33: (128, 6, 3), 63: (128, 6, 63), 64: (128, 7, 1)}
LENGTH_RADII = (3, 16, 17, 64)


def lengths_of(tile):
    """one tile short of, exactly and 1, 2, 3 past a tile (four consecutive lengths: every
    residue of the 4-wide loop's remainder in the ragged last tile), two tiles and one past"""
    return (tile - 1, tile, tile + 1, tile + 2, tile + 3, 2 * tile, 2 * tile + 1)


# the radius sweep: three tiles, the last of 3 outputs: one seam on a falling, one on a rising slope
RADIUS_SWEEP = [Sweep(axis, r, 2 * tile_of(r) + 3) for axis in range(3) for r in RADII]
# the length sweep: the one seam of tile + 1 and tile + 3 on a rising slope, of tile + 2 and 2 tile
# on a falling one; 2 tile + 1 has both
LENGTH_SWEEP = [Sweep(axis, r, n, n % tile_of(r) in (1, 3) and n < 2 * tile_of(r)) for axis in range(3)
                for r in LENGTH_RADII for n in lengths_of(tile_of(r))]
SWEEPS = {c.name: c for c in RADIUS_SWEEP + LENGTH_SWEEP}
assert len(SWEEPS) == len(RADIUS_SWEEP) + len(LENGTH_SWEEP)


def _seed(c):
    return 7000 + 1000 * c.axis + 10 * c.r + c.n


@functools.lru_cache(maxsize=None)
def sweep_profiles(name):
    """(a, b, c) of the case: the zigzag along its pass axis, random draws along the others"""
    c = SWEEPS[name]
    rng = np.random.default_rng(_seed(c))
    nz, ny, nx = c.shape
    prof = [random_profile(m, rng) for m in (nx, ny, nz)]
    prof[c.axis] = zigzag_profile(c.n, tile_of(c.r), rng, c.rising_first)
    return tuple(frozen(p) for p in prof)


@functools.lru_cache(maxsize=None)
def sweep_image(name):
    return frozen(additive(*sweep_profiles(name)))


@functools.lru_cache(maxsize=None)
def sweep_expected(name):
    return frozen(ar.min_filter(sweep_image(name), SWEEPS[name].r))


def seams(c):
    """[(position of the first output after the seam, 'falling' | 'rising')] of a sweep case"""
    tile = tile_of(c.r)
    return [(s, "falling" if (j % 2 == 0) != c.rising_first else "rising")
            for j, s in enumerate(range(tile, c.n, tile))]


def chain(img, r, axis=None, **mutant):
    """tiled_pass along x, y and z, with the mutant in the pass along ``axis``"""
    out = np.asarray(img, np.float32)
    for ax in range(3):
        res = tiled_pass(np.moveaxis(out, 2 - ax, 0), r, **(mutant if ax == axis else {}))
        out = np.ascontiguousarray(np.moveaxis(res, 0, 2 - ax))
    return out


# ------------------------------------------------------------------ positive images: the ragged last tile
# In the last tile of a line the end of the staged positions is the zero extension, which never
# wins in an additive image.  In a positive image it always does: the outputs within r of the end
# are 0, and a level that loses staged zeros there leaves a positive value -- which shows in the
# filtered image where the other two passes do not reach a border, so the other extents are 2r + 3
# (and 66 along x for the y and z passes).  One tile and 0 .. 3 outputs: every residue of the loop.
# Radii up to 3 only: the remainder is at most 3 positions, and at a larger radius every window
# that reads them holds further zeros (losing some of many zeros changes no output: nothing to pin).
POSITIVE_RADII = (1, 2, 3)


class Positive(NamedTuple):
    axis: int
    r: int
    n: int

    @property
    def name(self):
        return f"{'xyz'[self.axis]}-r{self.r}-n{self.n}"

    @property
    def shape(self):
        m = 2 * self.r + 3
        return [(m, m, self.n), (m, self.n, 66), (self.n, m, 66)][self.axis]


POSITIVES = {c.name: c for c in (Positive(axis, r, tile_of(r) + d) for axis in range(3) for r in POSITIVE_RADII
                                 for d in range(4))}


@functools.lru_cache(maxsize=None)
def positive_image(name):
    c = POSITIVES[name]
    return frozen((np.random.default_rng(7500 + _seed(c)).random(c.shape) + 0.5).astype(np.float32))


# ------------------------------------------------------------------ random volumes
def random_image(shape, seed):
    """[-1, 1], as tests/test_gpu_autobbox.py: the zero extension bites where a face is positive"""
    return (np.random.default_rng(seed).random(shape) * 2 - 1).astype(np.float32)


# (shape, r): more than one large tile along x and along z; one image on both sides of the switch
RANDOM_CASES = [((140, 9, 131), 17), ((140, 9, 131), 33), ((140, 9, 131), 64),
                ((5, 9, 260), 17), ((5, 9, 260), 33), ((5, 9, 260), 64),
                ((70, 45, 130), 16), ((70, 45, 130), 17)]


@functools.lru_cache(maxsize=None)
def random_volume(shape):
    return frozen(random_image(shape, 8000 + sum(shape)))


# ------------------------------------------------------------------ special values across a seam
class Special(NamedTuple):
    r: int
    side: int          # the image is side^3
    nan_at: tuple      # (z, y, x): the footprint straddles the first seam of every axis
    zero_at: tuple     # +0 here, the last voxel of the first x tile; -0 at x + 1
    ninf_at: tuple


SPECIALS = {"small": Special(2, 70, (63, 63, 63), (10, 10, 63), (66, 20, 62)),
            "large": Special(17, 132, (127, 127, 127), (20, 20, 127), (70, 70, 129))}
INF_CASES = {"small": ((9, 9, 70), 2), "large": ((40, 40, 170), 17)}      # (shape, r)


@functools.lru_cache(maxsize=None)
def special_image(name):
    """A positive image ([0.5, 1.5]: the rim of the result is the zero extension's +0) with one
    NaN, one +0 / -0 pair on the two sides of the first x seam and one -Inf, their footprints
    apart from each other."""
    s = SPECIALS[name]
    img = (np.random.default_rng(8100 + s.r).random((s.side,) * 3) + 0.5).astype(np.float32)
    img[s.nan_at] = np.nan
    z, y, x = s.zero_at
    img[z, y, x] = 0.0
    img[z, y, x + 1] = -0.0
    img[s.ninf_at] = -np.inf
    return frozen(img)


def inf_image(name):
    return np.full(INF_CASES[name][0], np.inf, np.float32)


# ------------------------------------------------------------------ min / max
MINMAX_LENGTHS = (1, 63, 64, 65, 255, 256, 257, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 257)
PLANT_AT = (0, 63, 64, 255, 256, ROUND - 1, ROUND)     # and n - 1


def factor3(n):
    """(nz, ny, nx) with two factors above 1 and nz * ny * nx = n, or None (n prime or 1)"""
    f = next((d for d in range(2, int(n ** 0.5) + 1) if n % d == 0), None)
    if f is None:
        return None
    m = n // f
    g = next((d for d in range(2, int(m ** 0.5) + 1) if m % d == 0), None)
    return (1, f, m) if g is None else (f, g, m // g)


def minmax_shapes(n):
    """dims (n, 1, 1) and one non-trivial factorisation, as [z, y, x] shapes"""
    return [(1, 1, n)] + ([factor3(n)] if factor3(n) else [])


def plant_indices(n):
    return sorted({i for i in PLANT_AT + (n - 1,) if 0 <= i < n})


def planted(n, at, value):
    """a constant 0.5 with one ``value``"""
    a = np.full(n, 0.5, np.float32)
    a[at] = value
    return a


def minmax_specials(n):
    """name -> flat image: a NaN, a -0 among +0, a +0 among -0 as the last element; all +Inf,
    all -Inf"""
    nan = np.full(n, 0.5, np.float32)
    nan[-1] = np.nan
    nzero = np.zeros(n, np.float32)
    nzero[-1] = -0.0
    pzero = np.full(n, -0.0, np.float32)
    pzero[-1] = 0.0
    return {"nan_last": nan, "negative_zero_last": nzero, "positive_zero_last": pzero,
            "all_pinf": np.full(n, np.inf, np.float32), "all_ninf": np.full(n, -np.inf, np.float32)}


def minmax_ref(a):
    """the literal loop where n is small, else the tree (equal: test_autobbox_premises_cpu)"""
    return ar.min_max(a) if a.size <= 300 else ar.min_max_fast(a)


# ------------------------------------------------------------------ the box
# k_threshold_box: min(2048, ceil(n / 256)) blocks of 256 threads over a grid stride.  (9, 301, 201)
# = 544,509 voxels is beyond one round of 524,288, and nx = 201 is no power of two.  Six voxels,
# each alone on one face of the box ((z, y, x); the last lies in the second round).
FACES_SHAPE = (9, 301, 201)
FACES = {"xmin": (4, 100, 3), "xmax": (2, 200, 197), "ymin": (6, 5, 100), "ymax": (3, 297, 50),
         "zmin": (0, 150, 120), "zmax": (8, 290, 150)}
FACES_THRESHOLD = 0.5


def faces_image(without=None):
    img = np.zeros(FACES_SHAPE, np.float32)
    for name, at in FACES.items():
        if name != without:
            img[at] = 1.0
    return img


def flat_index(shape, at):
    return int(np.ravel_multi_index(at, shape))


# the fused z pass in the large class: (150, 45, 84) at r = 17; low noise and a cuboid that
# survives the erosion as x 47 .. 65 (both groups of 64 lines), y 20 .. 24, z 107 .. 131 (both z tiles)
FUSED_SHAPE, FUSED_RADIUS, FUSED_BACKGROUND = (150, 45, 84), 17, 5.0
FUSED_CUBOID = (slice(90, 149), slice(3, 42), slice(30, 83))
FUSED_BOX = ([47, 20, 107], [65, 24, 131])


@functools.lru_cache(maxsize=None)
def fused_image():
    img = np.abs(random_image(FUSED_SHAPE, 8200)) * np.float32(0.02)
    img[FUSED_CUBOID] += np.float32(0.7)
    return frozen(img)


# a filtered value exactly on the threshold: min 0, max 1 and background 50 give the threshold
# 0.5; a region of 0.5 and a smaller one of nextafter(0.5, 1) survive the erosion, the single
# voxel of 1 does not.  Only the second region is above the threshold.
EXACT_BACKGROUND = 50.0
ABOVE = np.nextafter(np.float32(0.5), np.float32(1))
# r -> (shape, the region of 0.5, the region of ABOVE, its box after the erosion)
EXACT = {1: ((12, 12, 70), (slice(1, 7), slice(1, 7), slice(2, 21)), (slice(7, 11), slice(7, 11), slice(60, 69)),
             ([61, 8, 8], [67, 9, 9])),
         17: ((40, 40, 90), (slice(1, 39), slice(1, 39), slice(1, 41)), (slice(1, 38), slice(1, 38), slice(45, 89)),
              ([62, 18, 18], [71, 20, 20]))}


def exact_image(r):
    shape, at_threshold, above, _ = EXACT[r]
    img = np.zeros(shape, np.float32)
    img[at_threshold] = 0.5
    img[above] = ABOVE
    img[-1, -1, -1] = 1.0
    return img


# a NaN whose filtered footprint reaches beyond the surviving cuboid.  Through segment_bounds the
# NaN is also the image's min and max, so the threshold is NaN and nothing is above it; through
# threshold_bounds the filtered image meets the threshold of the image without the NaN, and the
# box is the cuboid's.  !(v <= thr) would take the whole image in the first call and the
# footprint in the second.
NAN_SHAPE, NAN_RADIUS, NAN_BACKGROUND = (20, 24, 70), 2, 5.0
NAN_CUBOID = (slice(4, 16), slice(5, 19), slice(40, 68))
NAN_AT = (9, 20, 39)         # footprint x 37 .. 41, y 18 .. 22, z 7 .. 11; the cuboid survives as x 42 .. 65, y 7 .. 16
NAN_BOX = ([42, 7, 6], [65, 16, 13])


@functools.lru_cache(maxsize=None)
def nan_images():
    """(the image without the NaN, with it)"""
    clean = np.abs(random_image(NAN_SHAPE, 8300)) * np.float32(0.02)
    clean[NAN_CUBOID] += np.float32(0.7)
    dirty = clean.copy()
    dirty[NAN_AT] = np.nan
    return frozen(clean), frozen(dirty)


def bounds_not_below(img, thr):
    """the mutant of the comparison: the box of the voxels with !(v <= thr)"""
    img = np.asarray(img, np.float32)
    with np.errstate(invalid="ignore"):
        idx = np.nonzero(~(img.astype(np.float64) <= np.float64(thr)))
    if len(idx[0]) == 0:
        return list(img.shape[::-1]), [0, 0, 0], False
    return [int(idx[2 - a].min()) for a in range(3)], [int(idx[2 - a].max()) for a in range(3)], True
