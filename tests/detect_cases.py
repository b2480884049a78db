"""Cases and references shared by tests/test_gpu_detect_edges.py (the detection stage of
csrc/detect.hip on a caller's image: the 26-neighbour test at the seams of its waves, the
per-wave candidate buffer, the capacity rerun, the x % T order, the quadratic fit and the
selection) and tests/test_detect_premises_cpu.py (the properties of these cases that the GPU
tests rely on, proved on the CPU from the references and the reported tile sizes alone).

Volumes are [z, y, x] float32; a candidate is (x, y, z, |v|, is_min, is_max) as
oracle/dog_ref.py lists them; ``t`` is spim_registration_amd.detect.tiles().
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import dog_ref

F32_MIN_NORMAL = np.float32(2.0 ** -126)


def frozen(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


def noise(shape, seed):
    """Uniform float32 noise in [-1, 1)."""
    return np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(2) - np.float32(1)


# ------------------------------------------------------------------ the references
def ref_peaks(img, min_peak, find_min=True, find_max=True, T=8):
    """dog_ref.find_peaks (the candidate rule literally ``not (|v| < min)``), then the wanted kinds."""
    return [p for p in dog_ref.find_peaks(img, min_peak, T) if (p[4] and find_min) or (p[5] and find_max)]


def literal_peaks(img, min_value, T):
    """InteractiveIntegral.findPeaks / isSpecialPoint (:360-468) walked voxel by voxel: thread
    ``t`` of T takes the positions with x % T == t in cursor (x fastest) order, skips the
    border and ``abs(v) < minValue``, compares the 26 neighbours as doubles with >= and <=,
    and "isMin" names a MAX first."""
    img = np.asarray(img, np.float32)
    nz, ny, nx = img.shape
    lists = [[] for _ in range(T)]
    with np.errstate(invalid="ignore"):
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    if x < 1 or x > nx - 2 or y < 1 or y > ny - 2 or z < 1 or z > nz - 2:
                        continue
                    c = img[z, y, x]
                    if abs(c) < np.float32(min_value):
                        continue
                    is_min = is_max = True
                    for dz in (-1, 0, 1):
                        for dy in (-1, 0, 1):
                            for dx in (-1, 0, 1):
                                if dz == dy == dx == 0:
                                    continue
                                v = float(img[z + dz, y + dy, x + dx])
                                is_min &= bool(v >= float(c))
                                is_max &= bool(v <= float(c))
                    if is_min:
                        lists[x % T].append((x, y, z, float(abs(c)), False, True))
                    elif is_max:
                        lists[x % T].append((x, y, z, float(abs(c)), True, False))
    return [p for lst in lists for p in lst]


def peaks_dropping_nan(img, min_peak, T=8):
    """What a 26-neighbour test through min / max of three gives: a NaN neighbour is dropped
    instead of failing the comparison.  Equals ref_peaks on a NaN-free image; the NaN cases
    need it to differ."""
    d = np.asarray(img, np.float32)
    lo = np.where(np.isnan(d), np.float32(np.inf), d)      # for "every neighbour >= c"
    hi = np.where(np.isnan(d), np.float32(-np.inf), d)     # for "every neighbour <= c"
    nz, ny, nx = d.shape
    c = d[1:-1, 1:-1, 1:-1]
    ge = np.ones(c.shape, bool)
    le = np.ones(c.shape, bool)
    with np.errstate(invalid="ignore"):
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dz == dy == dx == 0:
                        continue
                    sl = (slice(1 + dz, nz - 1 + dz), slice(1 + dy, ny - 1 + dy), slice(1 + dx, nx - 1 + dx))
                    ge &= lo[sl] >= c
                    le &= hi[sl] <= c
        cand = ~(np.abs(c) < np.float32(min_peak))
    zz, yy, xx = np.nonzero(cand & (ge | le))
    return {(int(x) + 1, int(y) + 1, int(z) + 1) for z, y, x in zip(zz, yy, xx)}


# ------------------------------------------------------------------ the wave mapping of k_dog_peaks
def wave_counts(shape, t):
    """(x strips, row blocks, z chunks, waves, blocks of 4 waves) of a [z, y, x] shape."""
    nz, ny, nx = shape
    if min(shape) < 3:
        return 0, 0, 0, 0, 0
    nsx, nyb, nzc = -(-(nx - 2) // t.columns), -(-(ny - 2) // t.rows), -(-(nz - 2) // t.planes)
    return nsx, nyb, nzc, nsx * nyb * nzc, -(-(nsx * nyb * nzc) // 4)


def wave_of(p, shape, t):
    """The wave that tests voxel p = (x, y, z): interior voxel (1, 1, 1) is the first of wave 0."""
    nsx, nyb, _, _, _ = wave_counts(shape, t)
    return (p[0] - 1) // t.columns + nsx * ((p[1] - 1) // t.rows + nyb * ((p[2] - 1) // t.planes))


def ring_residues(shape, t):
    """Planes loaded per z chunk, modulo the 3-plane load ring."""
    nz = shape[0]
    out = set()
    for tlo in range(1, nz - 1, t.planes):
        thi = min(nz - 1, tlo + t.planes)
        out.add((thi - tlo + 2) % 3)
    return out


def buffer_trace(peaks, shape, t):
    """The per-wave candidate buffer over a candidate list: each wave walks its centre planes
    upwards and its rows within a plane; a row's nb candidates are appended after a flush if
    ``count + nb > buffer``.  Returns {wave: (fills, flushes per plane step)}: ``fills`` the
    counts reached after each append, the second the flushes within each (wave, plane)."""
    rows = {}
    for p in peaks:
        rows.setdefault(wave_of(p, shape, t), {}).setdefault((p[2], p[1]), 0)
        rows[wave_of(p, shape, t)][(p[2], p[1])] += 1
    out = {}
    for w, byrow in rows.items():
        count, fills, flushes = 0, [], {}
        for (z, y) in sorted(byrow):
            nb = byrow[(z, y)]
            assert nb <= t.columns
            if count + nb > t.buffer:
                flushes[z] = flushes.get(z, 0) + 1
                count = 0
            count += nb
            fills.append(count)
        out[w] = (fills, flushes)
    return out


# ------------------------------------------------------------------ a. dense seams
# ((nz, ny, nx), T, seed): float noise at threshold 0, both kinds.  Every value of the three
# lists of the issue occurs; (69, 7, 127) is the one with two ragged z chunks, three x strips
# and two row blocks at once.  T = 64 meets nx = 3 (below) and nx = 65 (above).
DENSE_NX, DENSE_NY, DENSE_NZ = (3, 64, 65, 127), (3, 6, 7, 11), (3, 4, 5, 66, 67, 68, 69)
DENSE_T = (1, 3, 8, 64)
DENSE_CASES = [
    ((3, 3, 3), 1, 7),         # (seeds: the first at which test_detect_premises_cpu.py holds)
    ((4, 3, 64), 3, 300),
    ((5, 6, 65), 8, 4),
    ((66, 7, 3), 64, 9),
    ((67, 11, 65), 64, 1),
    ((68, 6, 127), 8, 1),
    ((69, 7, 127), 3, 1),
    ((66, 11, 64), 1, 1),
]


def dense_volume(shape, seed):
    return frozen(noise(shape, seed))


def seam_coordinates(n, tile):
    """Interior coordinates of an axis of n voxels next to a tile seam: the last of a tile and
    the first of the next (tiles start at 1)."""
    return [c for k in range(1, (n - 2) // tile + 1) for c in (k * tile, k * tile + 1) if c <= n - 2]


# ------------------------------------------------------------------ b. block counts
# full tiles, one chunk: (x strips, row blocks) -> waves -> blocks of 4 waves
BLOCK_GRIDS = [(1, 3), (5, 5), (5, 6), (5, 7), (3, 19)]
BLOCK_COUNTS = (1, 7, 8, 9, 15)
BLOCK_SEED = 21


def block_shape(grid, t):
    nsx, nyb = grid
    return (3, 2 + t.rows * nyb, 2 + t.columns * nsx)


# ------------------------------------------------------------------ c. the candidate buffer
# img = -1 at the chosen voxels, +0 elsewhere, min_peak 0.5: a -1 voxel has every neighbour
# >= it (a MAX), a 0 voxel is skipped -- the candidates are exactly the chosen voxels.
BUFFER_MIN_PEAK = 0.5


def mask_volume(shape, voxels):
    img = np.zeros(shape, np.float32)
    for x, y, z in voxels:
        img[z, y, x] = -1.0
    return frozen(img)


def buffer_cases(t):
    """name -> (volume, min_peak).  One x strip, one row block, one plane unless said."""
    one = (3, 2 + t.rows, 2 + t.columns)
    row = lambda y, n: [(x, y, 1) for x in range(1, 1 + n)]
    rest = t.buffer - t.columns                    # what a second row adds to reach the buffer size
    assert 0 < rest < t.columns and t.rows >= 3
    return {
        # every interior voxel a MAX: each row fills `columns` entries, each next row flushes
        "constant": (frozen(np.full((4, 2 + 2 * t.rows, 2 + t.columns + 1), 3.0, np.float32)), 0.0),
        # a full row, then `rest`: exactly `buffer` entries, flushed at the end only
        "exactly_full": (mask_volume(one, row(1, t.columns) + row(2, rest)), BUFFER_MIN_PEAK),
        # ... and one more in the third row: a flush with the buffer exactly full, then 1
        "one_more": (mask_volume(one, row(1, t.columns) + row(2, rest) + [(t.columns, 3, 1)]), BUFFER_MIN_PEAK),
        # ... the second row one short: buffer - 1, then 2 more do not fit
        "one_short_then_two": (mask_volume(one, row(1, t.columns) + row(2, rest - 1) + row(3, 2)), BUFFER_MIN_PEAK),
    }


# ------------------------------------------------------------------ d. capacity
# constant volume, maxima only: every interior voxel; lowering corner voxel (0, 0, 0) removes
# exactly (1, 1, 1) (its only interior neighbour), likewise the other corners
CAP_SHAPE = (22, 31, 115)
CAP_SMALL_SHAPE, CAP_SMALL_SEED = (9, 10, 11), 31


def capacity_volume(lowered):
    img = np.full(CAP_SHAPE, 1.0, np.float32)
    corners = [(z, y, x) for z in (0, CAP_SHAPE[0] - 1) for y in (0, CAP_SHAPE[1] - 1) for x in (0, CAP_SHAPE[2] - 1)]
    for c in corners[:lowered]:
        img[c] = 0.0
    return frozen(img)


# ------------------------------------------------------------------ e. values
VALUE_SHAPE = (68, 8, 66)    # two x strips, two row blocks, two z chunks
VALUE_SEED = 41


def seam_corner(t):
    """(x, y, z): the last column, row and plane of the first strip, block and chunk."""
    return t.columns, t.rows, t.planes


def zeros_volume():
    rng = np.random.default_rng(VALUE_SEED)
    return frozen(np.where(rng.random(VALUE_SHAPE) < 0.5, np.float32(0.0), np.float32(-0.0)))


def denormal_volume():
    """Random denormals of either sign with 40 normal values (+-2^-126 .. +-2^-120) among them."""
    rng = np.random.default_rng(VALUE_SEED + 1)
    bits = rng.integers(1, 1 << 23, VALUE_SHAPE, dtype=np.uint32) | (rng.integers(0, 2, VALUE_SHAPE, dtype=np.uint32) << 31)
    img = bits.view(np.float32).copy()
    flat = rng.choice(img.size, 40, replace=False)
    img.reshape(-1)[flat] = (np.float32(2.0) ** rng.integers(-126, -119, 40).astype(np.float32)) * \
        np.where(rng.random(40) < 0.5, np.float32(1), np.float32(-1))
    return frozen(img)


def inf_volume():
    img = noise(VALUE_SHAPE, VALUE_SEED + 2)
    rng = np.random.default_rng(VALUE_SEED + 3)
    for k in range(12):
        z, y, x = (int(rng.integers(0, n)) for n in VALUE_SHAPE)
        img[z, y, x] = np.inf if k % 2 else -np.inf
    img[10, 3, 20] = np.inf       # two interior ones for certain, well apart
    img[40, 5, 50] = -np.inf
    return frozen(img)


def plateau_volume(t):
    """Noise in [-1, 1) with equal-valued plateaus across the seams: +2 (above everything: each
    voxel has every neighbour <= it and not every neighbour >= it, a MIN by ``<=``) and -2
    (a MAX by ``>=``), and a 3 x 3 x 3 block of 0.5 whose centre passes both (the MAX wins).
    Returns (volume, {voxel: (is_min, is_max)})."""
    sx, sy, sz = seam_corner(t)
    img = noise(VALUE_SHAPE, VALUE_SEED + 4)
    want = {}

    def put(voxels, value, kind):
        for x, y, z in voxels:
            img[z, y, x] = value
            want[(x, y, z)] = kind
    cube = [(sx + a, sy + b, sz + c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    put(cube, 2.0, (True, False))                                        # 2 x 2 x 2 over all three seams
    put([(sx - 1 + a, 2, 10) for a in range(3)], 2.0, (True, False))      # 3 x 1 x 1 over the column seam
    put([(10, sy - 1 + a, 20) for a in range(3)], -2.0, (False, True))    # 1 x 3 x 1 over the row seam
    put([(20, 2, sz - 1 + a) for a in range(3)], -2.0, (False, True))     # 1 x 1 x 3 over the plane seam
    put([(30 + a, 5, 30 + c) for a in (0, 1) for c in (0, 1)], -2.0, (False, True))
    blk = [(40 + a, sy - 1 + b, 40 + c) for a in range(3) for b in range(3) for c in range(3)]
    for x, y, z in blk:
        img[z, y, x] = 0.5
    want[(41, sy, 41)] = (False, True)
    return frozen(img), want


# ------------------------------------------------------------------ f. NaN placement
NAN_SHAPE, NAN_SEED = VALUE_SHAPE, 51
BAIT = np.float32(5.0)    # above all noise: every neighbour of the NaN, a false MIN once the NaN is dropped


def nan_positions(t):
    """name -> (x, y, z) of the single NaN."""
    nz, ny, nx = NAN_SHAPE
    return {
        "halo_column": (t.columns + 1, 2, 10),       # lane 63 of strip 0, tested by strip 1
        "halo_row": (10, t.rows + 1, 12),            # the row under block 0, tested by block 1
        "halo_plane": (12, 2, t.planes + 1),         # loaded last by chunk 0, a centre plane of chunk 1
        "last_of_tiles": (t.columns, t.rows, t.planes),
        "face": (0, 3, 20),
        "corner": (0, 0, 0),
        "far_corner": (nx - 1, ny - 1, nz - 1),
        "mid_plane": (30, 3, 30),                    # with candidates on z - 2 .. z + 2
    }


def nan_volume(pos):
    img = noise(NAN_SHAPE, NAN_SEED)
    x, y, z = pos
    nz, ny, nx = NAN_SHAPE
    img[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = BAIT
    img[z, y, x] = np.nan
    return frozen(img)


# ------------------------------------------------------------------ g. localisation
LOC_INT_SHAPE, LOC_INT_SEED = (16, 15, 14), 5
LOC_FLOAT_SHAPE, LOC_FLOAT_SEED = (20, 22, 70), 62
LOC_CONST_SHAPE = (8, 8, 8)


def loc_int_volume():
    """round(6 u): small integers, so that differences tie, Hessians are singular and fits wander."""
    return frozen(np.round(np.random.default_rng(LOC_INT_SEED).random(LOC_INT_SHAPE) * 6))


def loc_float_volume():
    return frozen(noise(LOC_FLOAT_SHAPE, LOC_FLOAT_SEED))


def loc_const_volume():
    return frozen(np.full(LOC_CONST_SHAPE, 2.5, np.float32))


def loc_nonfinite_volume():
    img = np.array(loc_float_volume()[:, :, :30])
    img[5, 6, 7] = np.nan
    img[12, 10, 20] = np.inf
    img[8, 15, 12] = -np.inf
    return frozen(img)


SINGULAR, BORDER, EXHAUSTED = "singular", "border", "exhausted"     # else: the pass it was stable on


def fit_trace(img, peaks):
    """dog_ref.quadratic_localization's loop with the way each fit ended: (results, ends),
    ``ends`` one of SINGULAR / BORDER / EXHAUSTED or the number of the pass that was stable.
    (The premises test holds the results against dog_ref.quadratic_localization's.)"""
    d = np.asarray(img, np.float32)
    dims = d.shape[::-1]
    res, ends = [], []
    with np.errstate(all="ignore"):
        for pk in peaks:
            p = [int(pk[0]), int(pk[1]), int(pk[2])]
            out = (np.float32(pk[0]), np.float32(pk[1]), np.float32(pk[2]), np.float32(pk[3]))
            moves, end = 0, None
            while end is None:
                moves += 1
                H, g = dog_ref._hessian_and_gradient(d, *p)
                A = dog_ref._invert3(H)
                if A is None:
                    end = SINGULAR
                    break
                X = -np.array([A[3 * r] * g[0] + A[3 * r + 1] * g[1] + A[3 * r + 2] * g[2] for r in range(3)])
                moved = False
                for a in range(3):
                    if abs(X[a]) > 0.5 + moves * dog_ref.MAXIMA_TOLERANCE:
                        p[a] += 1 if X[a] > 0 else -1
                        moved = True
                if moved and any(p[a] <= 0 or p[a] >= dims[a] - 1 for a in range(3)):
                    end = BORDER
                elif not moved:
                    end = moves
                    fit = (X[0] * g[0] + X[1] * g[1] + X[2] * g[2]) / 2.0
                    out = (np.float32(p[0]) + np.float32(X[0]), np.float32(p[1]) + np.float32(X[1]),
                           np.float32(p[2]) + np.float32(X[2]), np.float32(d[p[2], p[1], p[0]]) + np.float32(fit))
                elif moves > dog_ref.MAX_NUM_MOVES:
                    end = EXHAUSTED
            res.append(out)
            ends.append(end)
    return res, ends


@functools.lru_cache(maxsize=None)
def _expected_points(key, min_peak, T):
    img = LOC_VOLUMES[key]()
    peaks = ref_peaks(img, min_peak, True, True, T)
    with np.errstate(all="ignore"):
        fitted = dog_ref.quadratic_localization(img, peaks)
    return peaks, fitted


LOC_VOLUMES = {"int": loc_int_volume, "float": loc_float_volume, "const": loc_const_volume,
               "nonfinite": loc_nonfinite_volume}


def expected_points(key, min_peak=0.0, T=8):
    """(candidates, their fits) of LOC_VOLUMES[key], computed once."""
    return _expected_points(key, float(min_peak), T)


def select(peaks, fitted, keep_threshold):
    """Localization.java:74: the float |value| > the float threshold, candidate order kept."""
    thr = np.float32(keep_threshold)
    with np.errstate(invalid="ignore"):
        return [(pk, f) for pk, f in zip(peaks, fitted) if abs(np.float32(f[3])) > thr]
