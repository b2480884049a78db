"""An independent NumPy float64 restatement of "Thin out detections"
(spim/fiji/plugin/ThinOut_Detections.java:73-166, :238-299; spim/fiji/plugin/thinout/
Histogram.java:56-90) and the cases the tests of csrc/thinout.hip share.

Every product and sum is an array operation of its own (NumPy never fuses a multiply and an
add), in the source order of the Java code: c = l * voxel, s = ((dx dx) + (dy dy)) + (dz dz),
sqrt of the smallest s over the other points -- the self pair left out by index, the lower
index among equal s --, the two range rules, and the histogram's bin arithmetic.
"""
import numpy as np

R_BLOCK = 256    # points per block of k_to_nn      (thinout.tile_sizes())
C_TILE = 512     # points per LDS tile
VOXELS = {"iso": (1.0, 1.0, 1.0), "aniso": (0.73, 0.73, 2.0)}
MIN_D, MAX_D = 1.5, 5.0    # the thresholds the cases are built around


# ---------------------------------------------------------------- the restatement
def scaled(points, voxel):
    """RealPoint(l[0] * voxel[0], l[1] * voxel[1], l[2] * voxel[2]) (:106-109)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return p * np.asarray(voxel, np.float64).reshape(1, 3)


def pair_sums(rows, c):
    """s[r, j] = ((dx dx) + (dy dy)) + (dz dz) of rows[r] - c[j]"""
    dx = rows[:, None, 0] - c[None, :, 0]
    dy = rows[:, None, 1] - c[None, :, 1]
    dz = rows[:, None, 2] - c[None, :, 2]
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    s = xx + yy
    return s + zz


def nn_sums(points, voxel=(1.0, 1.0, 1.0), chunk=128):
    """(the smallest s per point -- +inf for a list of one --, the index it belongs to -- -1)"""
    c = scaled(points, voxel)
    n = len(c)
    smin = np.full(n, np.inf)
    nearest = np.full(n, -1, np.int32)
    if n < 2:
        return smin, nearest
    for r0 in range(0, n, chunk):
        rows = c[r0:r0 + chunk]
        s = pair_sums(rows, c)
        assert np.isfinite(s).all()
        r = np.arange(len(rows))
        s[r, r0 + r] = np.inf            # the self pair, by index (every other s is finite)
        j = np.argmin(s, axis=1)         # the first of equal minima: the lower index
        smin[r0:r0 + chunk] = s[r, j]
        nearest[r0:r0 + chunk] = j
    return smin, nearest


def nn_distances(points, voxel=(1.0, 1.0, 1.0), chunk=128):
    """(dist float64, nearest int32): Math.sqrt of the smallest s"""
    smin, nearest = nn_sums(points, voxel, chunk)
    return np.sqrt(smin), nearest


def nn_distances_loop(points, voxel=(1.0, 1.0, 1.0)):
    """the same as a plain double loop over Python floats (IEEE doubles, one rounding per
    operation), the root taken per pair as the reference's search compares roots"""
    c = [[float(l) * float(v) for l, v in zip(p, voxel)] for p in np.asarray(points, np.float64).reshape(-1, 3)]
    dist, nearest = [], []
    for i, a in enumerate(c):
        best, arg = float("inf"), -1
        for j, b in enumerate(c):
            if j == i:
                continue
            dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
            d = float(np.sqrt(np.float64(((dx * dx) + (dy * dy)) + (dz * dz))))
            if arg < 0 or d < best:
                best, arg = d, j
        dist.append(best)
        nearest.append(arg)
    return np.array(dist, np.float64), np.array(nearest, np.int32)


def keep_flags(dist, min_distance, max_distance, keep_range):
    """:141"""
    d = np.asarray(dist, np.float64)
    if keep_range:
        return (d >= min_distance) & (d <= max_distance)
    return (d < min_distance) | (d > max_distance)


def thin_out(points, voxel=(1.0, 1.0, 1.0), min_distance=0.0, max_distance=5.0, keep_range=False):
    """(points[kept], kept int32 ascending, dist, nearest)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    dist, nearest = nn_distances(p, voxel)
    kept = np.nonzero(keep_flags(dist, min_distance, max_distance, keep_range))[0].astype(np.int32)
    return p[kept].copy(), kept, dist, nearest


def histogram(dist, select=None, bins=100):
    """Histogram.getMinMax and binData: (centres, counts int64, min, max); IndexError where Java
    throws ArrayIndexOutOfBoundsException"""
    v = np.asarray(dist, np.float64).reshape(-1)
    if select is not None:
        v = v[np.asarray(select).reshape(-1) != 0]
    assert len(v) and np.isfinite(v).all()
    lo, hi = v.min(), v.max()
    size = (hi - lo) + np.float64(0.000001)
    b = np.floor(((v - lo) / size) * np.float64(bins)).astype(np.int64)
    if (b < 0).any() or (b >= bins).any():
        raise IndexError("bin beyond the last")
    counts = np.bincount(b, minlength=bins).astype(np.int64)
    bin_size = size / np.float64(bins)
    centres = (lo + bin_size / np.float64(2.0)) + bin_size * np.arange(bins, dtype=np.float64)
    return centres, counts, float(lo), float(hi)


# ---------------------------------------------------------------- the cases
def make_case(seed, n, voxel):
    """n points (pixels): clusters (sigma 1.5 px) and sparse points in a box whose density puts
    the sparse nearest-neighbour distances around 6, both with random doubles as coordinates;
    from 16 points on also exact duplicates (n // 16 of them), a pair at exactly MIN_D and a
    pair at exactly MAX_D in the units of `voxel` (along z: MIN_D / voxel_z and MAX_D /
    voxel_z must be exact), all far from the rest; in a random order"""
    rng = np.random.default_rng(seed * 7919 + n)
    if n < 16:
        return np.ascontiguousarray(rng.uniform(0.0, 12.0, (n, 3)))
    ndup, nspecial = n // 16, 4
    nfree = n - ndup - nspecial
    side = 11.0 * nfree ** (1.0 / 3.0)
    ncl = nfree // 2
    centres = rng.uniform(0.0, side, (max(ncl // 6, 1), 3))
    clustered = centres[rng.integers(0, len(centres), ncl)] + rng.normal(0.0, 1.5, (ncl, 3))
    sparse = rng.uniform(0.0, side, (nfree - ncl, 3))
    free = np.concatenate([clustered, sparse])
    dup = free[rng.choice(nfree, ndup, replace=False)]
    vz = float(voxel[2])
    special = np.array([[-512.0, 64.0, 100.0], [-512.0, 64.0, 100.0 + MIN_D / vz],
                        [-1024.0, 32.0, 40.0], [-1024.0, 32.0, 40.0 + MAX_D / vz]])
    assert (MIN_D / vz) * vz == MIN_D and (MAX_D / vz) * vz == MAX_D
    pts = np.concatenate([free, dup, special])
    return np.ascontiguousarray(pts[rng.permutation(n)])


def lattice_case(side=6):
    """the integer lattice side^3 in index order (x slowest): an inner point ties on all six
    neighbours at s = 1, the nearest is the one at x - 1 (index - side^2)"""
    g = np.arange(side, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))


def seam_case():
    """2 * C_TILE points 100 apart on a grid, in index order, except: the points at R_BLOCK - 1
    and R_BLOCK are 0.5 from each other, the points at C_TILE - 1 and C_TILE too (the only near
    neighbour of each lies across the seam); the last point is an exact copy of the first (the
    first and the last index of a tile), and the points 300 and 700 are copies of point 100.
    Returns (points, {index: nearest index} of those points)."""
    n = 2 * C_TILE
    k = np.arange(n)
    pts = np.stack([100.0 * (k % 32), 100.0 * (k // 32), 37.0 * (k % 5)], axis=1).astype(np.float64)
    pts[R_BLOCK] = pts[R_BLOCK - 1] + [0.3, 0.4, 0.0]
    pts[C_TILE] = pts[C_TILE - 1] + [0.0, 0.3, 0.4]
    pts[n - 1] = pts[0]
    pts[300] = pts[100]
    pts[700] = pts[100]
    want = {R_BLOCK - 1: R_BLOCK, R_BLOCK: R_BLOCK - 1, C_TILE - 1: C_TILE, C_TILE: C_TILE - 1,
            0: n - 1, n - 1: 0, 100: 300, 300: 100, 700: 100}
    return np.ascontiguousarray(pts), want


SPLIT_N = 2500   # 10 blocks of rows, 5 tiles: the automatic split takes more than one partition
SIZE_CASES = [(1, n) for n in (2, 3, R_BLOCK - 1, R_BLOCK, R_BLOCK + 1, C_TILE - 1, C_TILE, C_TILE + 1, SPLIT_N)]
SPLIT_CASE = (2, 333)    # t_split 400: more partitions than points
